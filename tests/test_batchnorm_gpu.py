"""GPU: batch-normalised layers — csrc/batch_norm.hip against tests/bn_ref.py (float64) and eigenmat, bit-reproducibility, and whole
nets trained on both matrix paths, fused and unfused.

The reference's compiled bn_bprop_inplace (eigenmat.cc:2515-2537) has no return statement; built as the oracle builds it, the
function has no return instruction and runs on into the next function.  Neither that symbol of oracle/_ref/libconvnet_ref.so nor the
whole-host oracle oracle/_ref/libref_host_cpu.so (whose Layer::ApplyDerivativeofBatchNormalization calls it) can run a
batch-normalised net, so bn_bprop_inplace is checked against its float64 restatement here, and whole nets against fused vs unfused
runs of this library and against bn_ref.py on the library's own tensors."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bn_ref  # noqa: E402
from golden_cases import rel_err  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libconvnet_ref.so")
SHAPES = [(64, 20000), (4, 200000), (2, 300001), (1, 1001), (4096, 128), (37, 250), (130, 36), (3, 1)]   # (C, H)
IDS = [f"C{c}xH{h}" for c, h in SHAPES]


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _mat(a):
    """(C, H) array -> device Matrix (H, C): column c is row c of `a`."""
    from hip_adapter import _mat as device_mat
    a = np.asarray(a, np.float32)
    return device_mat(a, a.shape[1], a.shape[0])


def _vec(v):
    return _mat(np.asarray(v, np.float32).reshape(-1, 1))


def _host(m, C):
    return m.ToNumpy().reshape(C, -1)


def _v(m):
    return m.ToNumpy().reshape(-1)


def _err(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def _inputs(C, H, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((C, H)) * rng.uniform(0.5, 3, (C, 1)) + rng.uniform(-4, 4, (C, 1))).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 2, C).astype(np.float32), rng.uniform(-1, 1, C).astype(np.float32)
    mu, sigma = rng.uniform(-1, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    return rng, x, gamma, beta, mu, sigma


@pytest.mark.parametrize("C, H", SHAPES, ids=IDS)
@pytest.mark.parametrize("train, relu", [(1, 0), (1, 1), (0, 0), (0, 1)])
def test_fused_forward_matches_bn_ref(M, C, H, train, relu):
    _, x, gamma, beta, mu, sigma = _inputs(C, H, C + H)
    st, g, b, m, s, bm, bs = _mat(x), _vec(gamma), _vec(beta), _vec(mu), _vec(sigma), _vec(np.zeros(C)), _vec(np.zeros(C))
    M.BNFpropAct(st, g, b, m, s, bm, bs, 0.9, 1e-5, train, relu)
    y, mu_r, sigma_r, mb, sb = bn_ref.fprop(x, gamma, beta, mu, sigma, 0.9, 1e-5, train, relu=bool(relu))
    assert _err(_host(st, C), y) < 2e-5
    assert _err(_v(m), mu_r) < 1e-5 and _err(_v(s), sigma_r) < 1e-5
    if train:
        assert _err(_v(bm), mb) < 1e-5 and np.abs(_v(bs) / sb - 1).max() < 1e-5


@pytest.mark.parametrize("C, H", SHAPES, ids=IDS)
@pytest.mark.parametrize("relu", [0, 1])
def test_fused_backward_matches_bn_ref(M, C, H, relu):
    rng, x, gamma, beta, _, _ = _inputs(C, H, 7 * C + H)
    y, _, _, _, sb = bn_ref.fprop(x, gamma, beta, np.zeros(C), np.ones(C), 0.9, 1e-5, True, relu=bool(relu))
    state = y.astype(np.float32)
    d = rng.standard_normal((C, H)).astype(np.float32)
    if relu:
        d = np.where(state > 0, d, 0).astype(np.float32)   # ReLU' (applied before BN', by the edge's epilogue or the layer)
    sb = sb.astype(np.float32)
    dv, sv, dg, db = _mat(d), _mat(state), _vec(np.zeros(C)), _vec(np.zeros(C))
    M.BNBpropFused(dv, sv, _vec(gamma), _vec(beta), _vec(sb), dg, db)
    ref, dgamma, dbeta = bn_ref.bprop(d, state, gamma, beta, sb)
    assert _err(_host(dv, C), ref) < 2e-5
    assert _err(_v(dg), dgamma) < 1e-5 and _err(_v(db), dbeta) < 1e-5
    assert np.array_equal(_host(sv, C), state)   # the state is only read


def _eigenmat():
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/libconvnet_ref.so not built (reference tree absent at build time)")

    class eigenmat(ctypes.Structure):
        _fields_ = [("data", ctypes.POINTER(ctypes.c_float)), ("size", ctypes.c_int * 2), ("is_trans", ctypes.c_int),
                    ("owns_data", ctypes.c_int)]

    lib = ctypes.CDLL(REF_SO)

    def em(a):   # (C, H) array -> eigenmat (H, C), kept alive by the returned pair
        a = np.ascontiguousarray(a, np.float32)
        e = eigenmat()
        e.data = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        e.size[0], e.size[1] = a.shape[1], a.shape[0]
        return a, e
    return lib, em


@pytest.mark.parametrize("C, H", [(5, 1000), (1, 33), (40, 64), (2, 50001)])
def test_cudamat_entries_match_eigenmat(M, C, H):
    lib, em = _eigenmat()
    rng, x, gamma, _, mu, sigma = _inputs(C, H, 3 * C + H)
    d, tgt = rng.standard_normal((C, H)).astype(np.float32), rng.standard_normal((C, H)).astype(np.float32)
    # bn_bprop, scale_targets 0 and 0.5
    for st in (0.0, 0.5):
        t_host = [em(a) for a in (d, x, gamma.reshape(-1, 1), mu.reshape(-1, 1), sigma.reshape(-1, 1), tgt.copy())]
        fn = lib._Z8bn_bpropP8eigenmatS0_S0_S0_S0_S0_f
        assert fn(*[ctypes.byref(e) for _, e in t_host], ctypes.c_float(st)) == 0
        want = t_host[5][0]
        t = _mat(tgt)
        M.BNBprop(_mat(d), _mat(x), _vec(gamma), _vec(mu), _vec(sigma), t, st)
        assert _err(_host(t, C), want) < 1e-4
        assert _err(want, bn_ref.bn_bprop(d, x, gamma, mu, sigma, tgt, st)) < 1e-4
    # bn_grad
    dg, db = np.zeros((C, 1), np.float32), np.zeros((C, 1), np.float32)
    args = [em(a) for a in (d, x, mu.reshape(-1, 1), sigma.reshape(-1, 1))] + [em(dg), em(db)]
    dg, db = args[4][0], args[5][0]
    fn = lib._Z7bn_gradP8eigenmatS0_S0_S0_S0_S0_
    assert fn(*[ctypes.byref(e) for _, e in args]) == 0
    gg, gb = _vec(np.zeros(C)), _vec(np.zeros(C))
    M.BNGrad(_mat(d), _mat(x), _vec(mu), _vec(sigma), gg, gb)
    scale_g = np.abs((x - mu[:, None]) / sigma[:, None] * d).sum(axis=1)
    assert (np.abs(_v(gg) - dg.reshape(-1)) / scale_g).max() < 1e-5
    assert (np.abs(_v(gb) - db.reshape(-1)) / np.abs(d).sum(axis=1)).max() < 1e-5
    # bn_bprop_inplace: eigenmat's has no return path (module docstring); against its restatement
    dv, dgm = _mat(d), _vec(np.zeros(C))
    M.BNBpropInplace(dv, _mat(x), dgm)
    want, wdg = bn_ref.bn_bprop_inplace(d, x)
    assert _err(_host(dv, C), want) < 2e-5 and _err(_v(dgm), wdg) < 1e-5


def test_cudamat_entries_check_dimensions(M):
    from convnet_amd.matrix import MatrixError
    a, b = _mat(np.zeros((3, 10))), _mat(np.zeros((4, 10)))
    with pytest.raises(MatrixError, match="dimensions"):
        M.BNBpropInplace(a, b, _vec(np.zeros(3)))
    with pytest.raises(MatrixError, match="dimensions"):
        M.BNGrad(a, a, _vec(np.zeros(3)), _vec(np.zeros(2)), _vec(np.zeros(3)), _vec(np.zeros(3)))


def test_bn_calls_are_bit_reproducible(M):
    C, H = 64, 100000
    rng, x, gamma, beta, mu, sigma = _inputs(C, H, 11)
    d = rng.standard_normal((C, H)).astype(np.float32)
    outs = []
    for _ in range(2):
        st, m, s, bm, bs = _mat(x), _vec(mu), _vec(sigma), _vec(np.zeros(C)), _vec(np.zeros(C))
        M.BNFpropAct(st, _vec(gamma), _vec(beta), m, s, bm, bs, 0.9, 1e-5, 1, 1)
        dv, dg, db = _mat(d), _vec(np.zeros(C)), _vec(np.zeros(C))
        M.BNBpropFused(dv, st, _vec(gamma), _vec(beta), bs, dg, db)
        outs.append([t.ToNumpy() for t in (st, m, s, bm, bs, dv, dg, db)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- whole nets ----------------------------------------------------------------------------------------------------------------------
def _net(text, batch, fused, **kw):
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import SyntheticDataHandler
    net = ConvNet(text, fused=fused, **kw)
    net.SetBatchsize(batch)
    net.SetupDataset(SyntheticDataHandler(net, batch, seed=5, num_batches=1))
    net.AllocateMemory(False)
    return net


def _bn_state(net):
    return {l.GetName(): [m.ToNumpy().reshape(-1) for m in (l.gamma_, l.beta_, l.mu_, l.sigma_)]
            for l in net.layers_ if l.UseBatchNormalization()}


def _train(net, steps, seed=17):
    from convnet_amd.matrix import Matrix
    losses = []
    for i in range(steps):
        Matrix.InitRandom(seed + i)
        net.TrainOneBatch()
        out = net.output_layers_[0]
        p = out.GetState().ToNumpy().reshape(out.GetNumChannels(), -1)    # softmax probabilities, (classes, batch)
        y = out.GetData().ToNumpy().reshape(-1).astype(int)
        losses.append(float(-np.log(np.maximum(p[y, np.arange(y.size)], 1e-30)).mean()))
    return np.array(losses)


def _pair(text, batch, **kw):
    a, b = _net(text, batch, False, **kw), _net(text, batch, True, **kw)
    b.parameters_.FromNumpy(a.parameters_.ToNumpy())
    return a, b


def test_bn_parameters_start_as_the_reference_sets_them(M):
    from convnet_amd import models
    net = _net(models.small_bn(), 8, True)
    for name, (g, b, m, s) in _bn_state(net).items():
        assert (g == 1).all() and (b == 0).all() and (m == 0).all() and (s == 1).all(), name


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("relu", [True, False])
def test_small_bn_net_trains_fused_like_unfused(M, path, relu):
    from convnet_amd import _lib, models
    old = _lib.lib.convnet_hip_get_matrix_path()
    _lib.lib.convnet_hip_set_matrix_path(path)
    try:
        a, b = _pair(models.small_bn(relu=relu), 32)
        la, lb = _train(a, 5), _train(b, 5)
    finally:
        _lib.lib.convnet_hip_set_matrix_path(old)
    assert np.all(np.isfinite(la)) and np.all(np.isfinite(lb))
    np.testing.assert_allclose(lb, la, rtol=2e-4)
    pa, pb = a.parameters_.ToNumpy().reshape(-1), b.parameters_.ToNumpy().reshape(-1)
    assert rel_err(pb, pa) < 1e-3 and not np.array_equal(pa, _net(models.small_bn(relu=relu), 32, False).parameters_.ToNumpy().reshape(-1))
    sa, sb = _bn_state(a), _bn_state(b)
    for name in sa:
        for u, v in zip(sa[name], sb[name]):
            assert rel_err(v, u) < 1e-3, name
        assert not np.all(sa[name][0] == 1), ("gamma never moved", name)


def test_test_mode_forward_uses_the_running_statistics(M):
    from convnet_amd import models
    from convnet_amd.layer import LinearLayer
    net = _net(models.small_bn(), 32, True)
    _train(net, 3)
    for name in ("conv1", "fc3"):
        l = net.GetLayerByName(name)
        cls = l.__class__
        l.__class__, l.batch_normalize_ = LinearLayer, False    # the same pass without BN and ReLU: the pre-BN activations
        net.PlanLayers()
        for k in net.layers_:
            k.ResetAddOrOverwrite()
        net.Fprop(False)
        C = l.GetNumChannels()
        x = l.GetState().ToNumpy().reshape(C, -1)
        l.__class__, l.batch_normalize_ = cls, True
        net.PlanLayers()
        for k in net.layers_:
            k.ResetAddOrOverwrite()
        net.Fprop(False)
        g, b, m, s = (v.ToNumpy().reshape(-1) for v in (l.gamma_, l.beta_, l.mu_, l.sigma_))
        want = bn_ref.fprop(x, g, b, m, s, l.bn_f_, l.bn_epsilon_, False, relu=True)[0]
        assert _err(l.GetState().ToNumpy().reshape(C, -1), want) < 2e-5, name


def test_unfused_overlap_run_equals_one_stream_run(M):
    from convnet_amd import models
    a = _net(models.small_bn(), 32, False)
    b = _net(models.small_bn(), 32, False, overlap_wgrad=True)
    b.parameters_.FromNumpy(a.parameters_.ToNumpy())
    la, lb = _train(a, 3), _train(b, 3)
    assert np.array_equal(la, lb)
    assert np.array_equal(a.parameters_.ToNumpy(), b.parameters_.ToNumpy())
    for name, vs in _bn_state(a).items():
        for u, v in zip(vs, _bn_state(b)[name]):
            assert np.array_equal(u, v), name


def test_vgg16_bn_step_fused_matches_unfused(M):
    # The fused entry applies the ReLU to (x - m)·(gamma/s) + beta, the reference sequence to ((x - m)/s)·gamma + beta from statistics
    # summed in another order: a pre-activation within rounding of 0 can land on either side, and with ~10^8 normalised units per
    # step some do — those units pass their derivative in one run and not in the other.  So: the loss tightly, the update in norm.
    from convnet_amd import models
    a, b = _pair(models.vgg_bn(), 32)
    p0 = a.parameters_.ToNumpy().reshape(-1).copy()
    la, lb = _train(a, 1), _train(b, 1)
    assert np.all(np.isfinite(la)) and np.all(np.isfinite(lb))
    np.testing.assert_allclose(lb, la, rtol=1e-4)
    pa, pb = a.parameters_.ToNumpy().reshape(-1), b.parameters_.ToNumpy().reshape(-1)
    assert np.all(np.isfinite(pb))
    ua, ub = pa.astype(np.float64) - p0, pb.astype(np.float64) - p0
    assert np.linalg.norm(ub - ua) / np.linalg.norm(ua) < 1e-2
    sb = _bn_state(b)
    for name, vs in _bn_state(a).items():
        u, v = np.concatenate(vs).astype(np.float64), np.concatenate(sb[name])   # mu is ~1e-7 here: measured against the whole set
        assert np.linalg.norm(v - u) / np.linalg.norm(u) < 1e-4, name


def test_fused_train_step_runs_gamma_beta_in_the_multi_step_batch(M, monkeypatch):
    from convnet_amd import models
    net = _net(models.small_bn(), 32, True)
    seen = {}
    update, multi = net.UpdateWeights, M.SGDMomentumStepMulti

    def spy_update():
        seen["planned"] = list(net._bn_steps)
        return update()

    def spy_multi(items):
        seen.setdefault("batches", []).append([it[1] for it in items])
        return multi(items)
    monkeypatch.setattr(net, "UpdateWeights", spy_update)
    monkeypatch.setattr(M, "SGDMomentumStepMulti", staticmethod(spy_multi))
    net.TrainOneBatch()
    bn = [l for l in net.layers_ if l.UseBatchNormalization()]
    want = {id(m) for l in bn for m in (l.gamma_, l.beta_)}
    assert {id(it[1]) for it in seen["planned"]} == want and len(seen["planned"]) == 2 * len(bn)
    assert len(seen["batches"]) == 1 and want <= {id(p) for p in seen["batches"][0]}   # one launch with the edges' steps
    assert not net._bn_steps


def _torch_pass(net, x, labels, gb):
    """float64 torch restatement of one training pass (Fprop(true), CE derivative, Bprop) of a built LINEAR, dropout-free small_bn():
    conv (shared bias), average pool, FC, batch norm with batch statistics (biased variance, eps in the sqrt), softmax CE summed over
    the batch.  For such a net the reference's BN' is the true gradient (tests/test_batchnorm_cpu.py).  Layouts are the library's:
    states (C, H, W, N), conv banks (C, Ky, Kx, F), FC weights (D, F).  `gb` = {layer: (gamma, beta)} before the pass (Bprop steps
    them).  Returns ({edge: (dW, db, sum|dy| per channel)} scaled like ComputeOuter by 1/N, {layer: (batch mu, batch sigma)})."""
    import torch
    import torch.nn.functional as Fn
    from convnet_amd.edge import AvgPoolEdge, ConvEdge, FCEdge
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)   # noqa: E731
    N = labels.size
    inp = net.input_layers_[0]
    acts = {inp.GetName(): t(x.reshape(inp.GetNumChannels(), inp.GetSizeY(), inp.GetSizeX(), N))}
    leaves, stats = {}, {}
    for l in net.layers_:
        if l.IsInput():
            continue
        (e,) = l.incoming_edge_
        a = acts[e.GetSource().GetName()]
        if isinstance(e, ConvEdge):
            d = e.conv_desc_
            w = t(e.GetWeight().ToNumpy().reshape(a.shape[0], d.kernel_size_y, d.kernel_size_x, l.GetNumChannels()), True)
            b = t(e.GetBias().ToNumpy().reshape(-1), True)
            y = Fn.conv2d(a.permute(3, 0, 1, 2), w.permute(3, 0, 1, 2), stride=(d.stride_y, d.stride_x),
                          padding=(-d.padding_y, -d.padding_x)) + b[None, :, None, None]
            y = y.permute(1, 2, 3, 0)
            leaves[e.GetName()] = (w, b, y)
        elif isinstance(e, AvgPoolEdge):
            d = e.conv_desc_
            y = Fn.avg_pool2d(a.permute(3, 0, 1, 2), (d.kernel_size_y, d.kernel_size_x), (d.stride_y, d.stride_x),
                              (-d.padding_y, -d.padding_x)).permute(1, 2, 3, 0)
        else:
            assert isinstance(e, FCEdge)
            w, b = t(e.GetWeight().ToNumpy(), True), t(e.GetBias().ToNumpy().reshape(-1), True)
            y = (w.T @ a.reshape(-1, N) + b[:, None]).reshape(l.GetNumChannels(), 1, 1, N)
            leaves[e.GetName()] = (w, b, y)
        assert tuple(y.shape) == (l.GetNumChannels(), l.GetSizeY(), l.GetSizeX(), N), (l.GetName(), tuple(y.shape))
        y.retain_grad()
        if l.UseBatchNormalization():
            C = l.GetNumChannels()
            col = y.reshape(C, -1)
            mb = col.mean(dim=1)
            sb = torch.sqrt(((col - mb[:, None]) ** 2).mean(dim=1) + l.bn_epsilon_)
            g, be = (t(v) for v in gb[l.GetName()])
            y = ((col - mb[:, None]) / sb[:, None] * g[:, None] + be[:, None]).reshape(y.shape)
            stats[l.GetName()] = (mb.detach().numpy(), sb.detach().numpy())
        acts[l.GetName()] = y
    out = net.output_layers_[0]
    logits = acts[out.GetName()].reshape(out.GetNumChannels(), N)
    loss = -torch.log_softmax(logits, dim=0)[torch.tensor(labels), torch.arange(N)].sum()
    loss.backward()
    # the bias gradient of an edge into a BN layer is ~0 (BN removes the mean): its error is measured against sum|dy| / N per channel
    grads = {k: tuple(v * net.GetEdgeByName(k).scale_gradients_ / N for v in (
        w.grad.numpy().reshape(-1), b.grad.numpy().reshape(-1), y.grad.abs().reshape(b.numel(), -1).sum(dim=1).numpy()))
        for k, (w, b, y) in leaves.items()}
    return grads, stats


@pytest.mark.parametrize("fused", [False, True])
def test_linear_small_bn_pass_matches_a_float64_restatement_of_the_net(M, fused):
    # independent of this library's host: the whole net written out in torch float64 (no relu, no dropout: the reference's BN' is then
    # the true gradient), against one Fprop(true) / ComputeDeriv / Bprop of the library
    from convnet_amd import models
    net = _net(models.small_bn(relu=False, dropprob=0.0), 32, fused)
    for l in net.layers_:
        l.ResetAddOrOverwrite()
    for e in net.edges_:
        e.NotifyStart()
    net.GetBatch(net.train_dataset_)
    x = net.input_layers_[0].GetState().ToNumpy().reshape(-1)
    labels = net.output_layers_[0].GetData().ToNumpy().reshape(-1).astype(np.int64)
    bn = [l for l in net.layers_ if l.UseBatchNormalization()]
    gb = {l.GetName(): (_v(l.gamma_), _v(l.beta_)) for l in bn}
    net.Fprop(True)
    net.ComputeDeriv()
    net.Bprop()
    grads, stats = _torch_pass(net, x, labels, gb)
    assert len(grads) == 4
    for name, (dw, db, dy_abs) in grads.items():
        e = net.GetEdgeByName(name)
        lb = _v(e.GetGradBias())
        ew = rel_err(_v(e.GetGradWeight()), dw)
        eb = float(np.abs(lb - db).max() / max(np.abs(lb + db).mean(), dy_abs.max()))
        print(name, f"dW {ew:.2e} db {eb:.2e}")
        assert ew < 1e-4 and eb < 1e-4, (name, ew, eb)
    for l in bn:
        mb, sb = stats[l.GetName()]
        assert _err(_v(l.batch_mu_), mb) < 1e-5 and np.abs(_v(l.batch_sigma_) / sb - 1).max() < 1e-5, l.GetName()
