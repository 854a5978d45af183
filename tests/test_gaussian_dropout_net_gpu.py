"""GPU: whole nets with Gaussian dropout — models.gaussian_dropout_small (ReLU, max pool), its linear / average-pool variant and a
batch-normalised one — unfused (the reference's call sequence on a stored noise matrix) against fused (gaussian_dropout /
gaussian_dropout_undo, no noise matrix) with equal seeds, each against tests/gaussian_dropout_ref.py with the device's noise replayed,
the test-time pass, and the train_convnet entry point from an HDF5 file.

The steps, the standard of fused against unfused (1e-5 on states, derivatives and gradients, 1e-6 on parameters) and the tolerance of
device against oracle (TOL) are those of tests/test_fused_host_configs_gpu.py, at that file's batch size.  A step records the states
twice: behind Fprop (post-dropout) and behind Bprop, where the unfused sequence has divided them by the noise again."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
import gaussian_dropout_ref as ref  # noqa: E402
from fused_host_nets import CONFIGS  # noqa: E402
from golden_cases import rel_err  # noqa: E402
from test_fused_host_configs_gpu import SEEDS, TOL, _check_fused_equals_unfused, _flat, _optimizers  # noqa: E402

N = CONFIGS["c_into_fc"][1]      # the batch the fused kernels' small nets run at
GAUSS_LAYERS = ("conv1", "fc2", "fc3")


def _texts():
    from convnet_amd import models
    return {"relu_maxpool": models.gaussian_dropout_small(), "linear_avgpool": models.gaussian_dropout_small(relu=False, pool="AVERAGE_POOL"),
            "relu_bn": models.gaussian_dropout_small(batch_normalize=True, pool="AVERAGE_POOL")}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _noise(net, l):
    """The multiplier of layer l's last training forward pass: the stored matrix (unfused), or drawn again from the call id (fused)."""
    from convnet_amd.matrix import Matrix
    if l.store_dropout_noise_:
        return _flat(l.dropout_noise_).copy()
    m = Matrix()
    m.AllocateGPUMemory(l.GetState().GetRows(), l.GetState().GetCols())
    m.GaussianDropoutNoise(l.gaussian_call_id_, l.dropprob_)
    return _flat(m).copy()


def _step(net, seed):
    from convnet_amd.matrix import Matrix
    Matrix.InitRandom(seed)
    for l in net.layers_:
        l.ResetAddOrOverwrite()
    for e in net.edges_:
        e.NotifyStart()
    net.GetBatch(net.train_dataset_)
    net.Fprop(True)
    r = dict(states={l.GetName(): _flat(l.GetState()).copy() for l in net.layers_},
             noise={l.GetName(): _noise(net, l) for l in net.layers_ if l.gaussian_dropout_})
    net.ComputeDeriv()
    for l in net.output_layers_:      # (the fused output entry keeps the logits until here)
        r["states"][l.GetName()] = _flat(l.GetState()).copy()
    net.Bprop()
    r.update(derivs={l.GetName(): _flat(l.GetDeriv()).copy() for l in net.layers_ if not l.IsInput()},
             final={l.GetName(): _flat(l.GetState()).copy() for l in net.layers_},
             grads=net.grad_parameters_.ToNumpy().reshape(-1).copy())
    return r


# ---- the Gaussian layers against the reference module, teacher-forced from the device's own tensors around them --------------------------
def _up(e, l, a):
    from convnet_amd.edge import ConvEdge
    from oracle_net import _geom
    O = oracle.port
    if isinstance(e, ConvEdge):
        g = _geom(e, e.GetSource(), N)
        y = O.conv_up(g, a.reshape(g.in_shape()), e.GetWeight().ToNumpy().reshape(g.filt_shape()))
        return O.add_row_vec(y.reshape(g.F, -1), e.GetBias().ToNumpy().reshape(-1)).reshape(-1)
    Fo = l.GetNumChannels()
    y = O.dot(np.ascontiguousarray(a.reshape(-1, N)), e.GetWeight().ToNumpy(), np.zeros((Fo, N), np.float32), 0.0, 1.0, False, True)
    return O.add_row_vec(y, e.GetBias().ToNumpy().reshape(-1)).reshape(-1)


def _down(e, l, a, dy, yact):
    from convnet_amd.edge import AvgPoolEdge, MaxPoolEdge
    from oracle_net import _geom
    O = oracle.port
    if isinstance(e, MaxPoolEdge):
        g = _geom(e, l, N, True)
        return O.max_pool_undo(g, a.reshape(g.in_shape()), dy.reshape(g.pooled_shape()), yact.reshape(g.pooled_shape())).reshape(-1)
    if isinstance(e, AvgPoolEdge):
        g = _geom(e, l, N, True)
        return O.avg_pool_undo(g, dy.reshape(g.pooled_shape())).reshape(-1)
    D, Fo = a.size // N, e.GetDest().GetNumChannels()
    return O.dot(np.ascontiguousarray(dy.reshape(Fo, N)), e.GetWeight().ToNumpy(), np.zeros((D, N), np.float32), 0.0, 1.0).reshape(-1)


def _check_vs_reference(net, r, mode):
    for name in GAUSS_LAYERS:
        l = net.GetLayerByName(name)
        (e,) = l.incoming_edge_
        n = r["noise"][name]
        assert not (n == 0).any(), "premise: no exact 0 in the noise"
        # forward: the device's state of the source layer through the edge, then activation, noise and clip
        pre = _up(e, l, r["states"][e.GetSource().GetName()])
        want = ref.forward(pre, n, l.gaussian_act, l.max_act_gaussian_dropout_)
        err = rel_err(r["states"][name], want)
        assert err < TOL, (mode, "state vs reference", name, err)
        # backward: the device's derivative of the layer above through the edge, then dropout' and the activation's derivative at the
        # restored state
        (o,) = l.outgoing_edge_
        dst = o.GetDest().GetName()
        dx = _down(o, l, r["states"][name], r["derivs"][dst], r["states"][dst])
        want_d, want_s = ref.backward(dx, r["states"][name], n, l.gaussian_act)
        err = rel_err(r["derivs"][name], want_d)
        assert err < TOL, (mode, "derivative vs reference", name, err)
        if mode == "unfused":
            err = rel_err(r["final"][name], want_s)
            assert err < TOL, (mode, "restored state vs reference", name, err)      # src/layer.cc:404
        else:
            assert np.array_equal(r["final"][name], r["states"][name]), (mode, "the fused undo rewrote the state", name)
    clipped = np.abs(r["states"]["fc2"]).max()
    assert clipped <= 10.0, clipped


def _zero_mean_history_err(e, opt, ha, hb, r):
    """The bias of an edge into a batch-normalised layer: batch normalisation removes the mean, so its gradient sum(dy) / N is 0 but
    for the rounding of the sum, and so is what one step adds to the history, epsilon times that.  A difference of two such roundings
    has no scale of its own: as tests/test_batchnorm_gpu.py does for this gradient, it is measured against sum|dy| / N per channel
    (times epsilon; the histories were equal before the step)."""
    dy = np.abs(r["derivs"][e.GetDest().GetName()].astype(np.float64)).reshape(ha.size, -1).sum(axis=1)
    return float(np.abs(ha.astype(np.float64) - hb).max() / (opt.epsilon_ * e.scale_gradients_ / N * dy.max()))


def _run(text, reference):
    from test_net_gpu import build, copy_params
    a, b = build(text, N, fused=False), build(text, N, fused=True)
    copy_params(a, b)
    gauss = [l.GetName() for l in a.layers_ if l.gaussian_dropout_]
    assert gauss == list(GAUSS_LAYERS)
    assert all(l.store_dropout_noise_ for l in a.layers_ if l.gaussian_dropout_)
    assert not any(l.store_dropout_noise_ or l.dropout_noise_._t is not None for l in b.layers_ if l.gaussian_dropout_)      # no noise matrix
    for i, seed in enumerate(SEEDS):
        ra, rb = _step(a, seed), _step(b, seed)
        for name in gauss:          # first: a misaligned RNG must not look like a numeric mismatch
            assert np.array_equal(ra["noise"][name], rb["noise"][name]), ("the two modes drew different noise", name, i)
            assert ra["noise"][name].std() > 0.1
        _check_fused_equals_unfused(a, b, ra, rb)      # post-dropout states, derivatives, gradients
        if reference:
            _check_vs_reference(a, ra, "unfused")
            _check_vs_reference(b, rb, "fused")
        a.UpdateWeights()
        b.UpdateWeights()
        assert rel_err(_flat(a.parameters_), _flat(b.parameters_)) < 1e-6, ("parameters fused vs unfused", i)
        for ea, eb in zip(a.edges_, b.edges_):      # as tests/test_fused_host_configs_gpu.py: the next step starts from equal parameters and momentum
            for oa, ob in _optimizers(ea, eb):
                ha, hb = _flat(oa.gradient_history_), _flat(ob.gradient_history_)
                if oa is ea.bias_optimizer_ and ea.GetDest().UseBatchNormalization():
                    err = _zero_mean_history_err(ea, oa, ha, hb, ra)
                else:
                    err = rel_err(ha, hb)
                assert err < 1e-5, ("optimizer history", ea.GetName(), i, err)
                ob.gradient_history_.Set(oa.gradient_history_)
        b.parameters_.Set(a.parameters_)
    return a, b


@pytest.mark.parametrize("which", ["relu_maxpool", "linear_avgpool"])
def test_fused_equals_unfused_and_both_equal_the_reference(gpu, which):
    _run(_texts()[which], reference=True)


def test_a_batch_normalised_gaussian_layer_runs_both_modes_alike(gpu):
    a, b = _run(_texts()["relu_bn"], reference=False)
    assert b.gaussian_restore_ == {b.GetLayerByName("conv1")}      # bn's derivative reads the state the undo restored


def test_a_gaussian_max_pool_layer_runs_both_modes_alike(gpu):
    """The max-pool undo INTO a Gaussian layer compares with the layer's state after its backward pass: the fused undo restores it."""
    from fused_host_nets import pool_dropout
    from test_net_gpu import build, copy_params
    text = pool_dropout(0.5, relu=True).replace('name: "p1"\n', 'name: "p1"\n  gaussian_dropout: true\n')
    a, b = build(text, N, fused=False), build(text, N, fused=True)
    copy_params(a, b)
    for seed in SEEDS[:2]:
        ra, rb = _step(a, seed), _step(b, seed)
        assert np.array_equal(ra["noise"]["p1"], rb["noise"]["p1"])
        _check_fused_equals_unfused(a, b, ra, rb)
        assert np.array_equal(ra["final"]["p1"], rb["final"]["p1"])      # the reference's bits, in both modes


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_test_time_pass_is_the_net_without_dropout(gpu, fused):
    from test_net_gpu import build, copy_params
    text = _texts()["relu_maxpool"]
    plain = text.replace("  gaussian_dropout: true\n", "").replace("  max_act_gaussian_dropout: 10\n", "")
    for p in (0.3, 0.5, 0.2):
        plain = plain.replace(f"  dropprob: {p}\n", "")
    assert "dropprob" not in plain
    a, b = build(text, N, fused=fused), build(plain, N, fused=fused)
    copy_params(a, b)
    for net in (a, b):
        for l in net.layers_:
            l.ResetAddOrOverwrite()
        net.GetBatch(net.train_dataset_)
        net.Fprop(False)
    for la, lb in zip(a.layers_, b.layers_):
        assert np.array_equal(_flat(la.GetState()), _flat(lb.GetState())), la.GetName()


def test_train_convnet_trains_the_model_from_an_hdf5_file(tmp_path):
    import subprocess
    import sys
    from convnet_amd import hdf5io, models, pbtxt
    cases, size, bs = 24, 12, 8
    rng = np.random.default_rng(9)
    h5 = str(tmp_path / "data.h5")
    with hdf5io.File(h5, "w") as h:
        h.WriteDataset("images", rng.integers(0, 256, (cases, 3 * size * size), dtype=np.uint8))
        h.WriteDataset("labels", (np.arange(cases) % 10).astype(np.float32))
    m = pbtxt.parse(models.gaussian_dropout_small(image_size=size))
    m.max_iter, m.print_after, m.validate_after, m.save_after, m.checkpoint_dir = 3, 1, 0, 3, str(tmp_path / "ckpt")
    model, train = str(tmp_path / "net.pbtxt"), str(tmp_path / "train_data.pbtxt")
    pbtxt.write(model, m)
    with open(train, "w") as f:
        f.write(f'data_config {{\n  file_pattern: "{h5}"\n  layer_name: "input"\n  dataset_name: "images"\n  image_size: {size}\n'
                f'  gpu_image_size_y: {size}\n  gpu_image_size_x: {size}\n  num_colors: 3\n}}\n'
                f'data_config {{\n  file_pattern: "{h5}"\n  layer_name: "output"\n  dataset_name: "labels"\n}}\nbatch_size: {bs}\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "convnet_amd.train_convnet", "--board", "0", "--model", model, "--train", train]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    steps = [l.split() for l in out.stderr.splitlines() if l.startswith("Step ") and "Train Acc" in l]
    assert [s[1] for s in steps] == ["1", "2", "3"], out.stderr[-3000:]
    assert all(np.isfinite(float(s[-1])) and 0.0 <= float(s[-1]) <= 1.0 for s in steps), steps
    ckpt = str(tmp_path / "ckpt")
    (log,) = [n for n in os.listdir(ckpt) if n.endswith("_train.log")]
    rows = [l.split() for l in open(os.path.join(ckpt, log)).read().splitlines()]
    assert [r[0] for r in rows] == ["1", "2", "3"] and all(np.isfinite(float(v)) for r in rows for v in r)
