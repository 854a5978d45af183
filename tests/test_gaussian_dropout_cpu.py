"""CPU: Gaussian dropout on the host side — what is refused and how, the library calls a training step and a validation pass issue
per Gaussian layer in both modes (recorded without a GPU, tests/host_trace.py), the unchanged LayerPlan, and the reference module's
own arithmetic (tests/gaussian_dropout_ref.py) on hand-written cases."""
import numpy as np
import pytest

import gaussian_dropout_ref as ref
import host_trace
from convnet_amd import matrix, models
from convnet_amd.convnet import ConvNet, LayerPlan
from convnet_amd.matrix import Matrix
from fused_host_nets import pool_dropout

BATCH = 8
GAUSS = "  gaussian_dropout: true\n"


def _with(text, layer, extra):
    """The model text with ``extra`` added to the layer called ``layer``."""
    head = f'name: "{layer}"\n'
    assert text.count(head) == 1
    return text.replace(head, head + extra)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _exits(text, *words):
    with pytest.raises(SystemExit) as e:
        ConvNet(text, fused=True)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_the_supported_layers_are_accepted():
    for text in (models.gaussian_dropout_small(), models.gaussian_dropout_small(relu=False, pool="AVERAGE_POOL"),
                 models.gaussian_dropout_small(batch_normalize=True, pool="AVERAGE_POOL"),
                 _with(models.gaussian_dropout_small(), "input", "  dropprob: 0.1\n" + GAUSS)):
        for fused in (False, True):
            net = ConvNet(text, fused=fused)
            assert [l.GetName() for l in net.layers_ if l.gaussian_dropout_][-3:] == ["conv1", "fc2", "fc3"]
            assert all(l.TrainDropoutScale() == 1.0 for l in net.layers_)
    assert net.GetLayerByName("fc2").max_act_gaussian_dropout_ == 10 and net.GetLayerByName("fc3").max_act_gaussian_dropout_ == -1


def test_gaussian_dropout_without_dropprob_is_refused():
    _exits(models.gaussian_dropout_small().replace("  dropprob: 0.5\n", ""), "gaussian_dropout", "fc2", "dropprob")
    _exits(models.gaussian_dropout_small().replace("  dropprob: 0.5\n", "  dropprob: -0.5\n"), "gaussian_dropout", "fc2", "positive")


def test_gaussian_dropout_on_an_output_layer_is_refused():
    _exits(_with(models.gaussian_dropout_small(), "output", "  dropprob: 0.1\n" + GAUSS), "gaussian_dropout", "output", "output layer")


def test_max_act_without_gaussian_dropout_is_refused():
    _exits(_with(models.gaussian_dropout_small(), "pool1", "  max_act_gaussian_dropout: 5\n"), "max_act_gaussian_dropout", "pool1",
           "without gaussian_dropout")
    # (with binary dropout on the layer as well)
    _exits(_with(models.gaussian_dropout_small(), "pool1", "  dropprob: 0.5\n  max_act_gaussian_dropout: 5\n"), "max_act_gaussian_dropout", "pool1")


@pytest.mark.parametrize("value", ["inf", "nan"])
def test_a_dropprob_that_is_not_finite_is_refused(value):
    _exits(models.gaussian_dropout_small().replace("  dropprob: 0.5\n", f"  dropprob: {value}\n"), "gaussian_dropout", "fc2", "finite")


def test_a_softmax_hidden_layer_is_refused():
    text = models.gaussian_dropout_small().replace("activation: LOGISTIC", "activation: SOFTMAX")
    _exits(text, "gaussian_dropout", "fc3", "LOGISTIC")


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def test_layer_plan_fields_are_what_they_were():
    assert LayerPlan._fields == ("fuse_relu", "bn_relu", "activate", "output_entry", "logistic_dropout", "dropout_scale", "down_scale",
                                 "logistic_deriv")


def test_a_gaussian_layer_takes_none_of_the_dropout_fusions():
    net = ConvNet(models.gaussian_dropout_small(), fused=True)
    for name in ("conv1", "fc2", "fc3"):
        p = net.plan_[net.GetLayerByName(name)]
        assert p.down_scale is None and not p.logistic_dropout and not p.logistic_deriv and p.dropout_scale == 1.0, (name, p)
    assert net.plan_[net.GetLayerByName("conv1")].fuse_relu is True and net.plan_[net.GetLayerByName("fc2")].fuse_relu is True
    assert net.plan_[net.GetLayerByName("fc3")].activate          # the sigmoid rides in gaussian_dropout
    assert not net.gaussian_restore_                                # nothing reads these layers' states after their undo
    # the same net with binary dropout keeps its fusions
    binary = ConvNet(models.gaussian_dropout_small().replace(GAUSS, "").replace("  max_act_gaussian_dropout: 10\n", ""), fused=True)
    assert binary.plan_[binary.GetLayerByName("fc2")].down_scale == 2.0 and binary.plan_[binary.GetLayerByName("fc3")].logistic_dropout


# ---- the recorded calls -----------------------------------------------------------------------------------------------------------------
def _record(text, fused, steps=1):
    """(net, recorder, {section: lines}) of ``steps`` training steps and one validation pass, as host_trace.trace records them."""
    rec = host_trace.Recorder()
    saved = (matrix.lib, Matrix._device, Matrix.AllocateGPUMemory, Matrix._temp, Matrix._temp_size, Matrix._ones, Matrix._ones_size)
    allocate = Matrix.AllocateGPUMemory

    def allocate_and_register(self, rows, cols, name=""):
        allocate(self, rows, cols, name)
        rec.register(self)

    import torch
    matrix.lib = rec
    Matrix._device = torch.device("cpu")
    Matrix.AllocateGPUMemory = allocate_and_register
    Matrix._temp = Matrix._ones = None
    Matrix._temp_size = Matrix._ones_size = 0
    try:
        net = ConvNet(text, fused=fused)
        net.SetBatchsize(BATCH)
        net.SetupDataset(host_trace._NoData(BATCH))
        net.AllocateMemory(False)
        sections = {}
        for s in range(steps):
            start = len(rec.lines)
            net.TrainOneBatch()
            sections[f"train{s}"] = rec.lines[start:]
        start = len(rec.lines)
        for l in net.layers_:
            l.ResetAddOrOverwrite()
        net.Fprop(False)
        sections["valid"] = rec.lines[start:]
        names = {n: {k: rec._mat(getattr(net.GetLayerByName(n), k).mat_) for k in ("state_", "deriv_", "dropout_noise_")}
                 for n in (l.GetName() for l in net.layers_)}
    finally:
        (matrix.lib, Matrix._device, Matrix.AllocateGPUMemory, Matrix._temp, Matrix._temp_size, Matrix._ones, Matrix._ones_size) = saved
    return net, names, sections


def _f(v):
    return "f" + float(np.float64(v)).hex()


DROPOUT_ENTRIES = ("fill_with_randn", "fill_with_rand ", "sample_bernoulli", "dropout", "relu_dropout", "logistic_dropout", "gaussian_dropout")


def test_unfused_records_the_reference_sequences():
    text = _with(models.gaussian_dropout_small(), "input", "  dropprob: 0.1\n" + GAUSS)
    net, names, sec = _record(text, fused=False)
    for layer, p, max_act, deriv_entry in (("input", 0.1, None, None), ("conv1", 0.3, None, "apply_rectified_linear_deriv"),
                                           ("fc2", 0.5, 10, "apply_rectified_linear_deriv"), ("fc3", 0.2, None, "apply_logistic_deriv")):
        S, D, N = (names[layer][k] for k in ("state_", "deriv_", "dropout_noise_"))
        assert "unallocated" not in N, layer              # every Gaussian layer stores its noise, input layers and every class included
        forward = [f"fill_with_randn rnd {N}", f"mult_by_scalar {N} {_f(p)} {N} {_f(0)}", f"add_scalar {N} {_f(1)} {N}",
                   f"mult_elementwise {S} {N} {S} {_f(0)}"]
        backward = [] if deriv_entry is None else [f"mult_elementwise {D} {N} {D} {_f(0)}", f"divide_elementwise {S} {N} {S}"]
        lines = sec["train0"]
        assert [l for l in lines if N in l] == forward + backward, layer      # src/layer.cc:369-373 and 399-404, and nothing else
        after = lines[lines.index(forward[-1]) + 1]
        clip = f"upper_bound_mod_scalar {S} {_f(max_act)} {S}" if max_act else None
        assert (after == clip) if max_act else not after.startswith("upper_bound_mod_scalar"), (layer, after)      # :374-377
        if deriv_entry:
            assert lines[lines.index(backward[-1]) + 1] == f"{deriv_entry} {D} {S} {D}", layer      # the activation's derivative at the restored state
    assert net.gaussian_restore_ == {net.GetLayerByName(n) for n in ("conv1", "fc2", "fc3")}
    assert not [l for l in sec["valid"] if l.startswith(DROPOUT_ENTRIES)]


@pytest.mark.parametrize("variant, acts", [("relu_maxpool", (0, 0, 2, 1, 1, 2)), ("linear_avgpool", (0, 0, 2, 0, 0, 2)),
                                            ("relu_bn", (0, 0, 2, 1, 1, 2))])
def test_fused_records_one_entry_each_way_per_hidden_layer(variant, acts):
    text = {"relu_maxpool": models.gaussian_dropout_small(), "linear_avgpool": models.gaussian_dropout_small(relu=False, pool="AVERAGE_POOL"),
            "relu_bn": models.gaussian_dropout_small(batch_normalize=True, pool="AVERAGE_POOL")}[variant]
    text = _with(text, "input", "  dropprob: 0.1\n" + GAUSS)
    net, names, sec = _record(text, fused=True)
    lines = sec["train0"]
    gauss = [l for l in lines if l.startswith("gaussian_dropout")]
    layers = (("conv1", 0.3, -1.0), ("fc2", 0.5, 10.0), ("fc3", 0.2, -1.0))
    # forward: the input layer (no activation), then one entry per hidden layer; act is 0 where the conv / FC epilogue or bn_fprop_act
    # has applied the ReLU (or there is none), 2 for the logistic layer whose sigmoid rides along
    expect = [f"gaussian_dropout rnd {names['input']['state_']} {_f(0.1)} {_f(-1.0)} i0 i0"]
    expect += [f"gaussian_dropout rnd {names[n]['state_']} {_f(p)} {_f(m)} i{a} i0" for (n, p, m), a in zip(layers, acts[:3])]
    # backward: output to input, nothing on the input layer; restore_state only on the batch-normalised layer
    for (n, p, m), a in reversed(list(zip(layers, acts[3:]))):
        restore = int(variant == "relu_bn" and n == "conv1")
        expect.append(f"gaussian_dropout_undo rnd i0 {_f(p)} {names[n]['deriv_']} {names[n]['state_']} i{a} i{restore}")
    assert gauss == expect
    assert all("unallocated" in names[n]["dropout_noise_"] for n in ("input", "conv1", "fc2", "fc3"))      # no noise matrix
    # (pool1 itself has no dropout, so the max-pool edge out of conv1 may take its mask pair: it masks conv1's noised state and scales
    # nothing.  What must not appear is an epilogue that applies conv1's ReLU' or a dropout scale)
    banned = ("convDownMask", "convDown3DMask", "dotMask", "logistic_dropout", "logistic_deriv_scaled", "fill_with_randn", "divide_elementwise",
              "MaxPoolUndoRelu")
    assert not [l for l in lines if l.startswith("MaxPoolUndoMask") and not l.endswith(" i0")]      # relu = 0
    assert not [l for l in lines if l.startswith(banned)]
    # the derivative of the activation is not applied a second time
    for n, _, _ in layers:
        D, S = names[n]["deriv_"], names[n]["state_"]
        assert not [l for l in lines if l.startswith(("apply_rectified_linear_deriv", "apply_logistic_deriv")) and f"{D} {S}" in l], n
    assert not [l for l in sec["valid"] if l.startswith(DROPOUT_ENTRIES)]
    assert [l for l in sec["valid"] if l.startswith("apply_sigmoid")]      # ... and the logistic layer still gets its activation there


def test_a_gaussian_layer_behind_a_max_pool_applies_its_own_relu_and_restores_its_state():
    """The pool layer's ReLU has no epilogue to ride in (act 1), and the max-pool undo into the layer compares its input with the
    layer's state afterwards: the fused undo leaves the reference's state there (restore_state 1)."""
    text = _with(pool_dropout(0.5, relu=True), "p1", GAUSS)
    net, names, sec = _record(text, fused=True)
    S, D = names["p1"]["state_"], names["p1"]["deriv_"]
    assert [l for l in sec["train0"] if l.startswith("gaussian_dropout")] == [
        f"gaussian_dropout rnd {S} {_f(0.5)} {_f(-1.0)} i1 i0", f"gaussian_dropout_undo rnd i0 {_f(0.5)} {D} {S} i1 i1"]
    assert net.gaussian_restore_ == {net.GetLayerByName("p1")}
    # no mask pair on the edge INTO a layer with dropout, and no ReLU pass of its own (c1's ReLU' may still ride in that edge's undo)
    assert not [l for l in sec["train0"] if l.startswith(("MaxPoolMask", "MaxPoolUndoMask", "lower_bound_scalar"))]
    undo = [l for l in sec["train0"] if l.startswith("MaxPoolUndo")]
    assert len(undo) == 1 and f" {S} " in undo[0]                      # ... which reads p1's state: after the restoring undo
    assert sec["train0"].index(undo[0]) > sec["train0"].index(f"gaussian_dropout_undo rnd i0 {_f(0.5)} {D} {S} i1 i1")


def test_binary_dropout_records_what_it_recorded():
    """The same net with binary dropout: the fused entries of before, no Gaussian entry."""
    text = models.gaussian_dropout_small().replace(GAUSS, "").replace("  max_act_gaussian_dropout: 10\n", "")
    _, _, sec = _record(text, fused=True)
    names = [l.split()[0] for l in sec["train0"]]
    assert "gaussian_dropout" not in names and "gaussian_dropout_undo" not in names
    assert names.count("relu_dropout") + names.count("dropout") == 2 and names.count("logistic_dropout") == 1 and names.count("dotMask") >= 1


# ---- the reference module's own arithmetic ----------------------------------------------------------------------------------------------
def test_reference_noise_is_two_roundings():
    z = np.array([0.0, 1.0, -2.0, 3.0000002], np.float32)
    n = ref.noise(z, 0.3)
    assert n.dtype == np.float32
    assert np.array_equal(n, (z * np.float32(0.3)) + np.float32(1))
    assert n[2] == np.float32(np.float32(-2.0) * np.float32(0.3)) + np.float32(1) and n[2] > 0
    assert ref.noise(z, 0.3, np.float64).dtype == np.float64


def test_reference_forward_with_negative_noise_and_the_clip():
    x = np.array([2.0, -3.0, 4.0, 0.5, 30.0, 30.0], np.float32)
    n = np.array([1.5, 2.0, -0.5, 0.0, 0.5, -0.5], np.float32)
    assert np.array_equal(ref.forward(x, n, act=0), [3.0, -6.0, -2.0, 0.0, 15.0, -15.0])
    y = ref.forward(x, n, act=1)                   # ReLU first: a negative noise makes a NEGATIVE post-ReLU state
    assert np.array_equal(y, [3.0, 0.0, -2.0, 0.0, 15.0, -15.0]) and y[2] < 0
    assert np.array_equal(ref.forward(x, n, act=1, max_act=10.0), [3.0, 0.0, -2.0, 0.0, 10.0, -10.0])      # clipped at +-max_act
    assert np.array_equal(ref.forward(x, n, act=0, max_act=2.5), [2.5, -2.5, -2.0, 0.0, 2.5, -2.5])
    assert np.array_equal(ref.forward(x, n, act=0, max_act=0.0), ref.forward(x, n, act=0))                   # max_act <= 0: no clip
    s = ref.forward(np.zeros(2, np.float32), np.array([2.0, -2.0], np.float32), act=2)
    assert np.array_equal(s, [1.0, -1.0])          # sigmoid(0) = 0.5, times the noise


def test_reference_backward_divides_and_takes_the_derivative_at_the_restored_state():
    d = np.array([1.0, 1.0, 1.0, 1.0], np.float32)
    state = np.array([3.0, -2.0, 10.0, 0.0], np.float32)       # 2 * 1.5; 4 * -0.5; 30 * 0.5 clipped to 10; 0.5 * 0
    n = np.array([1.5, -0.5, 0.5, 0.0], np.float32)
    with np.errstate(all="ignore"):
        g, s = ref.backward(d, state, n, act=0)
    assert np.array_equal(g[:3], [1.5, -0.5, 0.5]) and np.array_equal(s[:3], [2.0, 4.0, 20.0])      # 20, not 30: the clip is not undone
    assert g[3] == 0 and np.isnan(s[3])                          # a noise of exactly 0: 0 / 0
    g, s = ref.backward(d, state, n, act=1)
    assert np.array_equal(g[:3], [1.5, -0.5, 0.5])              # negative noise: the restored state 4 > 0 passes a NEGATIVE derivative
    assert g[3] == 0                                            # NaN > 0 is false: the ReLU' gates the unit off
    g, s = ref.backward(np.array([2.0], np.float32), np.array([0.25], np.float32), np.array([0.5], np.float32), act=2)
    assert s[0] == 0.5 and g[0] == np.float32(np.float32(1.0 * 0.5) * np.float32(1 - 0.5))       # (d n) s (1 - s) at s = 0.5
    # float32 is rounded per operation, float64 is not the same computation in disguise
    g32, _ = ref.backward(np.float32(1) / 3, np.float32(0.7), np.float32(1.1), act=2)
    g64, _ = ref.backward(np.float32(1) / 3, np.float32(0.7), np.float32(1.1), act=2, dtype=np.float64)
    assert g32.dtype == np.float32 and g64.dtype == np.float64 and abs(float(g32) - float(g64)) < 1e-6
