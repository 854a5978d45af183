"""CPU: tests/logistic_ref.py on hand-written cases (the semantics of eigenmat.cc's apply_sigmoid, apply_logistic_deriv,
apply_logistic_grad, get_logistic_correct_normalized and compute_cross_entropy), the host's choice of the new layer and loss classes,
and the two new models against the reference's own graph builder."""
import os

import numpy as np
import pytest

import logistic_ref as R
import ref_host

f32 = np.float32


def test_sigmoid_saturates_without_nan():
    x = np.array([0.0, -0.0, 88.0, 89.0, 100.0, -88.0, -89.0, -100.0, -1000.0, np.nan, np.inf, -np.inf])
    y = R.sigmoid_f64(x)
    assert y[0] == y[1] == 0.5
    assert y[4] == 1.0 and y[10] == 1.0                       # exactly 1 for large x
    assert 0 < y[5] < 1e-38 and 0 < y[6] < 1e-38               # below the smallest normal fp32: 0 or a denormal there
    assert y[8] == 0.0 and y[11] == 0.0                        # exp overflows to inf: 1 / inf, no NaN
    assert np.isnan(y[9]) and np.isnan(y).sum() == 1
    assert abs(y[2] + y[5] - 1.0) < 1e-15 and abs(R.sigmoid_f64(1.0) - 0.7310585786300049) < 1e-16
    assert f32(R.sigmoid_f64(18.0)) == f32(1.0) and f32(R.sigmoid_f64(17.0)) < f32(1.0)   # where fp32 reaches exactly 1


def test_logistic_deriv_rounds_every_product():
    d, y = np.array([3.0, -2.0, 1.0, 5.0], f32), np.array([0.5, 0.25, 1.0, 0.0], f32)
    assert np.array_equal(R.logistic_deriv(d, y), np.array([0.75, -0.375, 0.0, 0.0], f32))
    assert np.array_equal(R.logistic_deriv(d, y, 2.0), np.array([1.5, -0.75, 0.0, 0.0], f32))
    # (d*y)*(1-y) is not d*(y*(1-y)) in fp32: the order is part of the contract
    d1, y1 = f32(1.0000001), f32(0.3333333)
    want = f32(f32(d1 * y1) * f32(f32(1) - y1))
    assert R.logistic_deriv([d1], [y1])[0] == want
    rng = np.random.default_rng(3)
    dd, yy = rng.standard_normal(4096).astype(f32), rng.random(4096).astype(f32)
    other = dd * (yy * (f32(1) - yy))
    assert not np.array_equal(R.logistic_deriv(dd, yy), other)
    # the scale is applied to the derivative first, as Mult then ApplyDerivativeOfLogistic do
    s = f32(1.0 / (1 - 0.3))
    assert np.array_equal(R.logistic_deriv(dd, yy, s), R.logistic_deriv(dd * s, yy))
    # a dropped unit (state exactly 0) has derivative exactly 0: y (1 - y) at the SCALED state
    assert R.logistic_deriv([7.0], [0.0], s)[0] == 0


def test_logistic_grad_ignores_negative_targets():
    y = np.array([0.9, 0.2, 0.7, 0.5, 0.3], f32)
    t = np.array([1.0, 0.0, -1.0, 0.5, -0.001], f32)
    g = R.logistic_grad(y, t)
    assert np.array_equal(g, np.array([f32(0.9) - f32(1), f32(0.2), 0, 0, 0], f32))
    assert np.array_equal(R.logistic_grad(y, t, 0.5), g * f32(0.5))
    assert not np.signbit(R.logistic_grad(y, t)[2])


def test_logistic_correct_counts_only_non_negative_targets():
    # (cols, rows) = (4, 5): row i is [p[:, i]], [t[:, i]]
    p = np.array([[0.9, 0.5, 0.1, 0.7, 0.4999999],
                  [0.2, 0.5, 0.9, 0.7, 0.5],
                  [0.6, 0.4, 0.2, 0.7, 0.5],
                  [0.4, 0.6, 0.8, 0.7, 0.5]], f32)
    t = np.array([[1.0, 0.5, 1.0, -1.0, 0.5],
                  [0.0, 0.5, -1.0, -1.0, 0.5],
                  [1.0, 0.5, -1.0, -2.0, 0.4999999],
                  [1.0, 0.5, 0.0, -0.5, 1.0]], f32)
    got = R.logistic_correct_normalized(p, t)
    # row 0: all four counted, p >= .5 agrees with t >= .5 in entries 0, 1, 2 -> 3/4
    # row 1: t and p exactly 0.5 count as "yes" on both sides: entries 0, 1 agree, 2 (p = .4) does not, 3 does -> 3/4
    # row 2: two don't-care targets; entry 0 wrong (p = .1, t = 1), entry 3 wrong (p = .8, t = 0) -> 0/2
    # row 3: no counted entry -> 0, not NaN
    # row 4: p just below .5 against t = .5 is wrong; (.5, .5) right; (.5, just below .5) wrong; (.5, 1) right -> 2/4
    assert np.array_equal(got, np.array([0.75, 0.75, 0.0, 0.0, 0.5], f32)), got
    assert got.dtype == np.float32
    third = R.logistic_correct_normalized(np.array([[0.9], [0.9], [0.1]], f32), np.array([[1.0], [0.0], [0.0]], f32))
    assert third[0] == f32(2) / f32(3)


def test_cross_entropy_of_a_distribution():
    t = np.array([[0.0, 1.0], [0.25, 0.0], [0.75, 0.0]], f32)
    p = np.array([[0.0, 1.0], [0.5, 0.0], [0.5, 0.0]], f32)
    ce = R.cross_entropy_f64(t, p, 1e-10)
    assert ce[0, 0] == 0 and ce[1, 1] == 0 and ce[2, 1] == 0           # t = 0 contributes nothing, even at p = 0: log(tiny) is finite
    assert abs(ce[1, 0] - 0.25 * np.log(2.0)) < 1e-9 and abs(ce[2, 0] - 0.75 * np.log(2.0)) < 1e-9
    assert abs(ce[0, 1]) < 1e-6                                         # 1 + 1e-10 rounds to 1 in fp32
    assert abs(R.cross_entropy_f64([1.0], [0.0], 1e-10)[0] - 23.025850929940457) < 1e-6   # -log(1e-10 as fp32)
    assert abs(ce[:, 0].sum() - np.log(2.0)) < 1e-9


def test_softmax_rows_sum_to_one_per_row():
    x = np.array([[1.0, 1000.0, -5.0], [2.0, 1000.0, -5.0], [3.0, -1000.0, -5.0]])
    p = R.softmax_rows_f64(x)
    assert np.allclose(p.sum(axis=0), 1.0) and np.allclose(p[:, 2], 1 / 3) and np.allclose(p[:, 1], [0.5, 0.5, 0.0])
    assert np.allclose(p[:, 0], np.exp([1.0, 2.0, 3.0]) / np.exp([1.0, 2.0, 3.0]).sum())


# ---- the host's classes and models ----------------------------------------------------------------------------------------------------
def test_choose_layer_class_and_loss_function_return_the_new_classes():
    from convnet_amd import layer, loss_functions, pbtxt
    for act, cls in (("LOGISTIC", layer.LogisticLayer), ("SOFTMAX_DIST", layer.SoftmaxDistLayer)):
        l = layer.Layer.ChooseLayerClass(pbtxt.parse(f'name: "x"\nnum_channels: 3\nactivation: {act}\ndropprob: 0.5\n', cls=pbtxt.Layer))
        assert type(l) is cls
    assert l.store_dropout_noise_ and isinstance(l, layer.SoftmaxLayer)            # SoftmaxDistLayer(SoftmaxLayer)
    lg = layer.Layer.ChooseLayerClass(pbtxt.parse('name: "x"\nnum_channels: 3\nactivation: LOGISTIC\ndropprob: 0.5\n', cls=pbtxt.Layer))
    assert lg.store_dropout_noise_ is False
    for name in ("LINEAR_ERROR", "CROSS_ENTROPY_BINARY", "CLASSIFICATION_BINARY", "CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED"):
        f = loss_functions.LossFunction.ChooseLossFunction(name)
        assert type(f).__name__ == {"LINEAR_ERROR": "LinearError", "CROSS_ENTROPY_BINARY": "CrossEntropyBinary",
                                    "CLASSIFICATION_BINARY": "ClassificationBinary",
                                    "CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED": "CrossEntropyDistributed"}[name]
    assert loss_functions.CrossEntropyBinary().GetLoss(None, None) == 0       # the reference's "Not implemented" returns 0
    with pytest.raises(SystemExit):
        loss_functions.LossFunction.ChooseLossFunction("HINGE")
    with pytest.raises(SystemExit):
        layer.Layer.ChooseLayerClass(pbtxt.parse('name: "x"\nnum_channels: 3\nactivation: HINGE_LINEAR\n', cls=pbtxt.Layer))


@pytest.fixture(scope="module")
def cpu_host():
    if not os.path.exists(ref_host.CPU_SO):
        pytest.skip("oracle/_ref/libref_host_cpu.so not built (needs the reference tree at build time)")
    return ref_host.RefHost(ref_host.CPU_SO)


@pytest.mark.parametrize("which", ["multilabel_small", "softdist_small", "multilabel_small_dropout_gc", "softdist_small_dropout_gc"])
def test_new_models_build_the_same_graph_as_the_reference(cpu_host, tmp_path, which):
    from convnet_amd import models
    from convnet_amd.convnet import ConvNet
    from convnet_amd.layer import LogisticLayer, SoftmaxDistLayer
    fn = getattr(models, which[:which.index("_small") + 6])
    text = fn(dropprob=0.25, grad_check=True) if which.endswith("_gc") else fn()
    m, d = ref_host.write_configs(tmp_path, text, 2, 1, 1, which)
    layers, edges, total = cpu_host.describe(m, d)
    net = ConvNet(text)
    net.SetBatchsize(2)
    mine_layers = [(l.GetName(), l.GetSizeY(), l.GetSizeX(), l.GetNumChannels(), bool(l.IsInput()), bool(l.IsOutput())) for l in net.layers_]
    mine_edges = [(e.GetSource().GetName(), e.GetDest().GetName(), e.GetParameterMemoryRequirement()) for e in net.edges_]
    assert mine_layers == layers
    assert mine_edges == edges
    assert sum(((n + 127) // 128) * 128 for _, _, n in mine_edges) == total
    out = net.output_layers_[0]
    if which.startswith("multilabel"):
        assert type(out) is LogisticLayer and out.GetNumChannels() == 2
        assert [type(net.GetLayerByName(n)) for n in ("conv1", "fc2")] == [LogisticLayer, LogisticLayer]
        assert (out.loss_function_, out.performance_metric_) == ("CROSS_ENTROPY_BINARY", "CLASSIFICATION_BINARY")
    else:
        assert type(out) is SoftmaxDistLayer
        assert out.loss_function_ == out.performance_metric_ == "CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED"
    assert [e.GradCheck() for e in net.edges_ if hasattr(e, "weight_optimizer_")] == [which.endswith("_gc")] * 3
    assert net.GetLayerByName("conv1").dropprob_ == (0.25 if which.endswith("_gc") else 0.0)
