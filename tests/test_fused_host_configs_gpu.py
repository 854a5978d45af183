"""GPU: the host's choice of entry point per layer configuration (ConvNet(fused=True): its per-layer ``LayerPlan``, the
max-pool mask path) on the small nets of tests/fused_host_nets.py — dropout on pool, conv, 1x1 and rnorm-fed layers, linear layers,
refused pool geometries, two outgoing / two incoming edges, and the reference's NIN model with its real dropout layers.

Each net is built unfused and fused with the same parameters and trained for three steps (Fprop(true), ComputeDeriv, Bprop,
UpdateWeights; one Fprop(false) between steps 1 and 2), the RNG re-seeded before each net's step and the fused net's parameters
and optimizer history re-synchronised to the unfused net's after each step's comparison.  After every step:
  1. the two runs' dropout masks are identical (checked first: a misaligned RNG must not look like a numeric mismatch);
  2. fused == unfused: every layer's state and derivative, the gradients and (after the update) the parameters; where the fused
     host used the max-pool mask pair, the pool undo equals the reference's call pair on the same tensors bit for bit;
  3. each mode == the whole-net CPU oracle (tests/oracle_net.py) with the device's dropout replayed: forward un-forced, backward
     teacher-forced op by op (as tests/test_full_geometry_gpu.py does).
Also: a refused mask geometry is tried once per (geometry, batch), and the persistent response-norm kernels keep their LDS limit
when one instantiation serves two channel counts in turn."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from golden_cases import rel_err  # noqa: E402
from fused_host_nets import CONFIGS  # noqa: E402

TOL = 1e-4
SEEDS = (101, 202, 303)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _flat(m):
    return m.ToNumpy().reshape(-1)


def _step(net, seed, train=True):
    """One step of TrainOneBatch's sequence, stopped before UpdateWeights; returns the device's states, derivatives, stored
    dropout noise and gradients."""
    from convnet_amd.matrix import Matrix
    Matrix.InitRandom(seed)
    for l in net.layers_:
        l.ResetAddOrOverwrite()
    if train:
        for e in net.edges_:
            e.NotifyStart()
    net.GetBatch(net.train_dataset_)
    net.Fprop(train)
    if not train:
        return {l.GetName(): _flat(l.GetState()) for l in net.layers_}
    net.ComputeDeriv()
    net.Bprop()
    return dict(states={l.GetName(): _flat(l.GetState()) for l in net.layers_},
                derivs={l.GetName(): _flat(l.GetDeriv()) for l in net.layers_ if not l.IsInput()},
                noise={l.GetName(): _flat(l.dropout_noise_) for l in net.layers_ if l.dropprob_ > 0 and l.store_dropout_noise_},
                grads=net.grad_parameters_.ToNumpy().reshape(-1).copy())


def _check_masks_equal(net, ra, rb):
    for l in net.layers_:
        if l.dropprob_ <= 0 or l.IsInput():
            continue
        n = l.GetName()
        if n in ra["noise"]:
            assert np.array_equal(ra["noise"][n], rb["noise"][n]), ("dropout mask (stored noise) differs between the runs", n)
        else:
            # a ReLU layer's mask is where its state is non-zero; a unit whose pre-activation is within rounding of 0 may differ
            a, b = ra["states"][n], rb["states"][n]
            diff = (a != 0) != (b != 0)
            assert np.abs(np.where(diff, a + b, 0)).max() <= 1e-5 * np.abs(a).max(), \
                ("dropout mask differs between the runs", n, int(diff.sum()))


def _check_fused_equals_unfused(a, b, ra, rb):
    for l in a.layers_:
        n = l.GetName()
        assert rel_err(ra["states"][n], rb["states"][n]) < 1e-5, ("state fused vs unfused", n, rel_err(ra["states"][n], rb["states"][n]))
        if n in ra["derivs"] and not l.IsInput():
            assert rel_err(ra["derivs"][n], rb["derivs"][n]) < 1e-5, ("deriv fused vs unfused", n, rel_err(ra["derivs"][n], rb["derivs"][n]))
    assert rel_err(ra["grads"], rb["grads"]) < 1e-5, ("gradients fused vs unfused", rel_err(ra["grads"], rb["grads"]))


def _check_mask_pool_pairs_bit_identical(net):
    """Where the fused host took the mask pair, the reference's call pair on the same tensors gives the same derivative, bit for bit
    (the source layer's derivative is final after the undo: it has one outgoing edge and either its ReLU' rode in the undo or it is
    a linear layer without dropout)."""
    from convnet_amd.edge import MaxPoolEdge
    from convnet_amd.matrix import Matrix
    checked = 0
    for e in net.edges_:
        if not isinstance(e, MaxPoolEdge) or e.mask_for_ is None:
            continue
        src, dst = e.GetSource(), e.GetDest()
        scale = net._fused_down_scale(src)
        if src.IsInput() or len(src.outgoing_edge_) != 1 or (scale is None and (src.is_relu or src.dropprob_ > 0)):
            continue
        d = src.GetDeriv()
        t = Matrix()
        t.AllocateGPUMemory(d.GetRows(), d.GetCols())
        t.SetShape4D_like(d)
        undo = Matrix.ConvMaxPoolUndoRelu if scale == 1.0 else Matrix.ConvMaxPoolUndo
        undo(src.GetState(), dst.GetDeriv(), dst.GetState(), t, e.conv_desc_, 0)
        assert np.array_equal(_flat(t), _flat(d)), ("mask pool undo != reference call pair", e.GetName())
        checked += 1
    return checked


def _check_vs_oracle(net, r):
    from convnet_amd.edge import FCEdge
    from oracle_net import forward_backward
    from test_full_geometry_gpu import _within
    x = r["states"][net.input_layers_[0].GetName()]
    labels = net.output_layers_[0].GetData().ToNumpy().reshape(-1)
    acts, od, og = forward_backward(net, x, labels, force=(r["states"], r["derivs"]), dropout_states=r["states"], dropout_noise=r["noise"])
    for l in net.layers_:
        e = rel_err(r["states"][l.GetName()], acts[l.GetName()])
        assert e < TOL, ("state vs oracle", l.GetName(), e)
    for name, d in od.items():
        if name in r["derivs"] and not net.GetLayerByName(name).IsInput():
            e = rel_err(r["derivs"][name], d)
            assert e < TOL, ("deriv vs oracle (forced)", name, e)
    assert og, "no parameter gradients"
    for e in net.edges_:
        if e.GetName() in og:
            dw, db = og[e.GetName()]
            gw, gb = _flat(e.GetGradWeight()), _flat(e.GetGradBias())
            # FC weight gradients at N = 8 are sums of 8 terms: as in test_full_geometry_gpu, elements that miss the max-over-mean
            # metric must agree to a few ulps of themselves
            ok = _within(gw, dw, TOL) if type(e) is FCEdge else rel_err(gw, dw) < TOL
            assert ok, ("dW vs oracle (forced)", e.GetName(), rel_err(gw, dw))
            assert rel_err(gb, db) < TOL, ("db vs oracle (forced)", e.GetName(), rel_err(gb, db))


def _optimizers(ea, eb):
    from convnet_amd.edge import EdgeWithWeight
    if not isinstance(ea, EdgeWithWeight) or ea.IsTied():
        return []
    pairs = [(ea.weight_optimizer_, eb.weight_optimizer_)]
    if ea.bias_optimizer_ is not None:
        pairs.append((ea.bias_optimizer_, eb.bias_optimizer_))
    return pairs


def _run(which, path):
    from convnet_amd import _lib
    from test_net_gpu import build, copy_params
    text, N = CONFIGS[which]
    _lib.lib.convnet_hip_set_matrix_path(1 if path == "split" else 0)
    try:
        a, b = build(text, N, fused=False), build(text, N, fused=True)
        copy_params(a, b)
        mask_pairs = 0
        for i, seed in enumerate(SEEDS):
            ra, rb = _step(a, seed), _step(b, seed)
            _check_masks_equal(a, ra, rb)
            _check_fused_equals_unfused(a, b, ra, rb)
            mask_pairs += _check_mask_pool_pairs_bit_identical(b)
            _check_vs_oracle(a, ra)
            _check_vs_oracle(b, rb)
            a.UpdateWeights()
            b.UpdateWeights()
            assert rel_err(_flat(a.parameters_), _flat(b.parameters_)) < 1e-6, ("parameters fused vs unfused", i)
            # the next step compares the two entry-point sequences on the same parameters and momentum: without this, rounding-level
            # drift compounds over the steps (the NIN model's conv1 derivative reached 3.4e-5 at step 2 with step 1 bit-identical)
            for ea, eb in zip(a.edges_, b.edges_):
                for oa, ob in _optimizers(ea, eb):
                    ha, hb = _flat(oa.gradient_history_), _flat(ob.gradient_history_)
                    assert rel_err(ha, hb) < 1e-5, ("optimizer history fused vs unfused", ea.GetName(), i, rel_err(ha, hb))
                    ob.gradient_history_.Set(oa.gradient_history_)
            b.parameters_.Set(a.parameters_)
            if i == 0:
                ea, eb = _step(a, 0, train=False), _step(b, 0, train=False)
                for n in ea:
                    assert rel_err(ea[n], eb[n]) < 1e-5, ("Fprop(false) state fused vs unfused", n)
        return b, mask_pairs
    finally:
        _lib.lib.convnet_hip_set_matrix_path(1)


@pytest.mark.parametrize("which", list(CONFIGS))
def test_fused_host_config_vs_unfused_and_oracle(gpu, which):
    from convnet_amd.edge import MaxPoolEdge
    net, mask_pairs = _run(which, "split")
    pools = [e for e in net.edges_ if isinstance(e, MaxPoolEdge)]
    if which in ("a_linear_pool_control", "f_max3s2_N8", "g_pool_then_conv", "g_conv_then_pool"):
        assert all(e.mask_ is not None for e in pools)    # these reach the mask pair (and the pair was checked where its output is final)
    if which in ("a_linear_pool_control", "f_max3s2_N8"):
        assert mask_pairs == len(SEEDS)
    if which in ("a_linear_pool_dropout", "b_relu_pool_dropout", "f_max3s2_N6", "f_max3s2_N10", "f_max2s2", "f_max3s1"):
        assert all(e.mask_ is None for e in pools)


@pytest.mark.parametrize("which", ["a_linear_pool_dropout", "c_into_nin", "g_conv_then_pool", "h_alexnet_nin67"])
def test_fused_host_config_on_the_fp32_matrix_path(gpu, which):
    _run(which, "fp32")


def test_refused_pool_geometry_is_tried_once(gpu, monkeypatch):
    """3 x 3 s2 max-pool at N = 6: the mask kernel refuses it (N % 4 != 0).  The edge remembers the refusal: over three fused
    steps MaxPoolMask is called at most once and the edge holds no mask buffer."""
    from convnet_amd.edge import MaxPoolEdge
    from convnet_amd.matrix import Matrix
    from test_net_gpu import build
    calls = []
    real = Matrix.ConvMaxPoolMask

    def counting(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(Matrix, "ConvMaxPoolMask", staticmethod(counting))
    text, N = CONFIGS["f_max3s2_N6"]
    net = build(text, N, fused=True)
    for seed in SEEDS:
        _step(net, seed)
        net.UpdateWeights()
    pool = next(e for e in net.edges_ if isinstance(e, MaxPoolEdge))
    assert len(calls) <= 1 and pool.mask_ is None, (len(calls), pool.mask_)


def test_rnorm_fast_kernels_across_channel_counts_in_one_process(gpu):
    """rnorm_undo_fast_kernel<64, 12, 24> serves C = 96 (73,216 B of LDS) and C = 84 (66,560 B): its dynamic-LDS limit must not drop
    below what a later C = 96 call needs.  Shape (C, 5, 5, 16), window 24: 400 locations, the fast path.  rnorm (64,256 B at C = 96)
    stays under 64 KB and runs alongside."""
    from hip_adapter import HipImpl
    hip = HipImpl()
    rng = np.random.default_rng(11)
    for C in (96, 84, 96):
        x = rng.standard_normal((C, 5, 5, 16)).astype(np.float32)
        dy = rng.standard_normal((C, 5, 5, 16)).astype(np.float32)
        e = rel_err(hip.rnorm(x, 24, 0.005, 0.75), oracle.port.rnorm(x, 24, 0.005, 0.75))
        assert e < TOL, ("rnorm", C, e)
        e = rel_err(hip.rnorm_undo(dy, x, 24, 0.005, 0.75), oracle.port.rnorm_undo(dy, x, 24, 0.005, 0.75))
        assert e < TOL, ("rnorm_undo", C, e)
