"""GPU: the Adagrad / RMSProp library entries (csrc/elementwise.hip) and the hosts built on them, on matrix path 1 as the trainer runs.

The float32 numpy restatements below are written from the formulas in include/convnet_hip.h, every statement one rounded operation;
tests/test_optimizers_cpu.py shows the same statements reproduce the reference's compiled CPU optimizer bit for bit."""
import numpy as np
import pytest

from golden_cases import rel_err

pytestmark = pytest.mark.gpu
f32 = np.float32
BIG = 2 * (1 << 20) + 5          # more than one grid pass of 2048 blocks x 256 threads x 4 floats: stride loop and tail together
SIZES = [1, 3, 4, 5, 1027, "off4", BIG]      # "off4": 1027 floats starting 4 bytes off 16-byte alignment (the scalar path)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _n(size):
    return 1027 if size == "off4" else size


def _mat(a, size=None):
    """A (1, n) device matrix holding `a`; size "off4": a view one float into a flat buffer."""
    from hip_adapter import _mat as device_mat
    a = np.asarray(a, np.float32).reshape(-1)
    if size != "off4":
        return device_mat(a, 1, a.size)
    m, _ = device_mat(a, 1, a.size, guard=(1, 0))   # the view keeps the buffer alive: Matrix.GetSlice stores a torch slice of its storage
    assert m.mat_.data_device % 16 == 4
    return m


def _data(size, seed=0):
    rng = np.random.default_rng(1000 + seed + _n(size) % 997)
    n = _n(size)
    g = rng.standard_normal(n).astype(np.float32)
    g[::7] = 0                                       # exact zeros: Adagrad's history then stays where it is
    w = rng.standard_normal(n).astype(np.float32)
    h = (0.1 * rng.standard_normal(n)).astype(np.float32)
    a = (0.5 + rng.random(n)).astype(np.float32)     # a second-moment history after some steps: positive, above delta
    return g, w, h, a


# ---- numpy restatements ------------------------------------------------------------------------------------------------------------
def np_adagrad(a, g, delta):
    c = a - f32(delta)
    return f32(delta) + np.sqrt(c * c + g * g)


def np_rms_prop(a, g, factor):
    return np.sqrt(f32(factor) * a * a + (f32(1) - f32(factor)) * g * g)


def np_sgd(g, w, h, l2, clip, eps, mom):
    if l2 > 0:
        g = g + w * f32(l2)
    if clip > 0:
        g = np.clip(g, -f32(clip), f32(clip))
    g = g * f32(eps)
    h = h * f32(mom) + g
    return g, w - h, h


def np_adagrad_step(g, w, h, a, delta, scale, l2, clip, eps, mom):
    a = np_adagrad(a, g, delta)
    g = g / a
    g = g * f32(scale)
    g, w, h = np_sgd(g, w, h, l2, clip, eps, mom)
    return g, w, h, a


def np_rmsprop_step(g, w, h, a, factor, l2, clip, eps, mom):
    h = h * f32(mom)
    if l2 > 0:
        g = g + w * f32(l2)
    if clip > 0:
        g = np.clip(g, -f32(clip), f32(clip))
    a = np_rms_prop(a, g, factor)
    g = g / a
    h = h + f32(eps) * g
    return g, w - h, h, a


# ---- 1. the reference's three entries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_reference_entries_equal_the_numpy_restatement(M, size):
    g, w, _, a = _data(size)
    A, G = _mat(a, size), _mat(g, size)
    M.AdagradUpdate(A, G, 0.1)
    assert np.array_equal(A.ToNumpy().reshape(-1), np_adagrad(a, g, 0.1))
    A = _mat(a, size)
    M.RMSPropUpdate(A, G, 0.9)
    assert np.array_equal(A.ToNumpy().reshape(-1), np_rms_prop(a, g, 0.9))
    W = _mat(w, size)
    W.Divide(A)
    assert np.array_equal(W.ToNumpy().reshape(-1), w / np_rms_prop(a, g, 0.9))
    assert np.array_equal(G.ToNumpy().reshape(-1), g)


def test_reference_entries_return_cudamat_error_codes(M):
    from convnet_amd._lib import lib
    a, b, short = _mat(np.ones(12)), _mat(np.ones(12)), _mat(np.ones(11))
    t = _mat(np.ones(12))
    t.mat_.is_trans = 1
    for fn, args in ((lib.adagrad, (0.5,)), (lib.rms_prop, (0.5,))):
        assert fn(a.GetMat(), short.GetMat(), *args) == -1          # ERROR_INCOMPATIBLE_DIMENSIONS
        assert fn(a.GetMat(), t.GetMat(), *args) == -7              # ERROR_TRANSPOSEDNESS
        short.mat_.is_trans = 1
        assert fn(a.GetMat(), short.GetMat(), *args) == -7          # transposedness is checked first
        short.mat_.is_trans = 0
    assert lib.divide_elementwise(a.GetMat(), short.GetMat(), a.GetMat()) == -1
    assert lib.divide_elementwise(a.GetMat(), b.GetMat(), short.GetMat()) == -1
    assert lib.divide_elementwise(a.GetMat(), t.GetMat(), a.GetMat()) == -7
    assert lib.adagrad_momentum_step(a.GetMat(), b.GetMat(), short.GetMat(), a.GetMat(), 1, 1, 0, 0, 0.1, 0.9) == -1
    assert lib.rmsprop_momentum_step(a.GetMat(), b.GetMat(), b.GetMat(), short.GetMat(), 0.9, 0, 0, 0.1, 0.9) == -1
    assert np.array_equal(a.ToNumpy().reshape(-1), np.ones(12, np.float32))   # a refused call changes nothing
    t.mat_.is_trans = 0


# ---- 2. the fused single entries ------------------------------------------------------------------------------------------------------
# (l2_decay, gradient_clip, momentum)
CORNERS = {"plain": (0.0, 0.0, 0.9), "l2": (0.01, 0.0, 0.9), "clip": (0.0, 0.3, 0.9), "l2_clip_no_momentum": (0.002, 0.5, 0.0)}


def _unfused(M, kind, mats, hyper, l2, clip, eps, mom):
    """The reference's call sequence through the library's own entries (src/optimizer.cc:226-231 + :174-200, :257-279)."""
    G, W, H, A = mats
    if kind == "adagrad":
        delta, scale = hyper
        M.AdagradUpdate(A, G, delta)
        G.Divide(A)
        G.Mult(scale)
        if l2 > 0:
            G.Add(W, l2)
        if clip > 0:
            G.UpperBoundMod(clip)
        G.Mult(eps)
        H.Mult(mom)
        H.Add(G)
    else:
        H.Mult(mom)
        if l2 > 0:
            G.Add(W, l2)
        if clip > 0:
            G.UpperBoundMod(clip)
        M.RMSPropUpdate(A, G, hyper[0])
        G.Divide(A)
        H.Add(G, eps)
    W.Add(H, -1)


def _fused(M, kind, mats, hyper, l2, clip, eps, mom):
    (M.AdagradMomentumStep if kind == "adagrad" else M.RMSPropMomentumStep)(*mats, *hyper, l2, clip, eps, mom)


def _restated(kind, arrays, hyper, l2, clip, eps, mom):
    return (np_adagrad_step if kind == "adagrad" else np_rmsprop_step)(*arrays, *hyper, l2, clip, eps, mom)


HYPER = {"adagrad": (0.1, float(f32(np.sqrt(7.0)))), "rmsprop": (0.9,)}


@pytest.mark.parametrize("corner", sorted(CORNERS))
@pytest.mark.parametrize("kind", ["adagrad", "rmsprop"])
def test_fused_step_equals_the_numpy_restatement(M, kind, corner):
    l2, clip, mom = CORNERS[corner]
    for size in SIZES:
        arrays = _data(size, 1)
        mats = [_mat(x, size) for x in arrays]
        _fused(M, kind, mats, HYPER[kind], l2, clip, 0.05, mom)
        want = _restated(kind, arrays, HYPER[kind], l2, clip, 0.05, mom)
        for what, m, v in zip(("gradient", "parameter", "history", "second history"), mats, want):
            got = m.ToNumpy().reshape(-1)
            assert np.array_equal(got, v), (kind, corner, size, what, int((got != v).sum()), rel_err(got, v))


@pytest.mark.parametrize("corner", sorted(CORNERS))
@pytest.mark.parametrize("kind", ["adagrad", "rmsprop"])
def test_fused_step_equals_the_unfused_sequence_of_library_entries(M, kind, corner):
    """Every entry of the unfused sequence is one rounded fp32 operation per reference statement, add_mult (`x += alpha*y`, behind
    Matrix.Add(m, alpha)) included: product rounded, then the sum.  With an fma there, Adagrad with l2_decay > 0 (g += l2*w) and every
    RMSProp case (h += epsilon*g) differ from the fused step by one rounding in some elements (20.8 % of RMSProp's momentum history at
    2*2^20 + 5 elements), so this test also pins that entry's arithmetic."""
    l2, clip, mom = CORNERS[corner]
    unequal = []
    for size in SIZES:
        arrays = _data(size, 2)
        a, b = [_mat(x, size) for x in arrays], [_mat(x, size) for x in arrays]
        _fused(M, kind, a, HYPER[kind], l2, clip, 0.05, mom)
        _unfused(M, kind, b, HYPER[kind], l2, clip, 0.05, mom)
        for what, x, y in zip(("gradient", "parameter", "history", "second history"), a, b):
            got, want = x.ToNumpy().reshape(-1), y.ToNumpy().reshape(-1)
            print(kind, corner, size, what, "differing", int((got != want).sum()), "of", got.size, "rel_err", rel_err(got, want))
            if not np.array_equal(got, want):
                unequal.append((size, what, int((got != want).sum()), rel_err(got, want)))
    assert not unequal, (kind, corner, unequal)


# ---- 3. the multi entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adagrad", "rmsprop"])
def test_multi_step_equals_single_steps_and_repeats_itself(M, kind):
    sizes = [1, 3, 4, 5, 1027, "off4", 1027, 5, 4, "off4", 3, 1, 1027, 4, 5, BIG, 3]      # 17 tensors: two launches
    assert len(sizes) == 17
    rng = np.random.default_rng(5)
    hypers = []
    for i in range(len(sizes)):
        l2, clip, mom = list(CORNERS.values())[i % 4]
        first = (0.05 + 0.1 * i, float(f32(np.sqrt(i + 1.0)))) if kind == "adagrad" else (0.5 + 0.02 * i,)
        hypers.append((*first, l2 * (1 + i), clip * (1 + 0.1 * i), 0.01 * (1 + i), mom * rng.random()))
    runs = []
    for mode in ("single", "multi", "multi"):
        items = [tuple(_mat(x, s) for x in _data(s, 3 + i)) + hypers[i] for i, s in enumerate(sizes)]
        if mode == "single":
            for it in items:
                _fused(M, kind, it[:4], it[4:-4], *it[-4:])
        else:
            (M.AdagradMomentumStepMulti if kind == "adagrad" else M.RMSPropMomentumStepMulti)(items)
        runs.append([m.ToNumpy().reshape(-1) for it in items for m in it[:4]])
    for k, (s, m1, m2) in enumerate(zip(*runs)):
        assert np.array_equal(s, m1), (kind, "tensor", k // 4, "array", k % 4)
        assert np.array_equal(m1, m2), (kind, "second run", k // 4, k % 4)
    assert not np.array_equal(runs[0][4 * 4 + 1], _data(sizes[4], 3 + 4)[1])      # the steps did step


# ---- 4. fused against unfused training --------------------------------------------------------------------------------------------------
def _with_optimizer(text, kind):
    if kind == "SGD":
        return text
    extra = {"ADAGRAD_SGD": "", "RMSPROP_SGD": "    rms_prop_factor: 0.9\n"}[kind]
    out = text.replace("optimizer {\n", "optimizer {\n    optimizer_type: " + kind + "\n" + extra)
    assert out.count(kind) == text.count("optimizer {\n") > 0
    return out


def _net(text, batch, fused):
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import SyntheticDataHandler
    net = ConvNet(text, fused=fused)
    net.SetBatchsize(batch)
    net.SetupDataset(SyntheticDataHandler(net, batch, seed=5, num_batches=1))
    net.AllocateMemory(False)
    return net


def _train(net, steps, seed=17):
    from convnet_amd.matrix import Matrix
    for i in range(steps):
        Matrix.InitRandom(seed + i)      # the same dropout masks in every run
        net.TrainOneBatch()


def _optimizers(net):
    from convnet_amd.edge import EdgeWithWeight
    out = [(e.GetName() + k, o) for e in net.edges_ if isinstance(e, EdgeWithWeight)
           for k, o in ((":weight", e.weight_optimizer_), (":bias", e.bias_optimizer_))]
    return out + [(l.GetName() + k, o) for l in net.layers_ if l.UseBatchNormalization()
                  for k, o in ((":gamma", l.gamma_optimizer_), (":beta", l.beta_optimizer_))]


def _state(net):
    """{name: array}: all parameters, all momentum histories and all second-moment histories, each as one vector over every optimizer in
    net order (the flat buffers without their alignment padding, which nothing initialises), and the batch-norm parameters per layer.
    Whole vectors, as the existing whole-net tests compare the flat parameter buffer: a conv bias in front of a batch-normalised layer
    has a gradient of pure rounding noise, which no relative measure of its own can compare."""
    from convnet_amd.edge import EdgeWithWeight
    cat = lambda ms: np.concatenate([m.ToNumpy().reshape(-1) for m in ms])      # noqa: E731
    opts = [o for _, o in _optimizers(net)]
    out = {"parameters": cat([m for e in net.edges_ if isinstance(e, EdgeWithWeight) for m in (e.GetWeight(), e.GetBias())]),
           "history": cat([o.gradient_history_ for o in opts])}
    if any(o.NeedsSecondHistory() for o in opts):
        out["second history"] = cat([o.second_history_ for o in opts if o.NeedsSecondHistory()])
    for l in net.layers_:
        if l.UseBatchNormalization():
            out[l.GetName() + " gamma"], out[l.GetName() + " beta"] = l.gamma_.ToNumpy().reshape(-1), l.beta_.ToNumpy().reshape(-1)
    return out


# the small net: the reference's GPU-vs-CPU tolerance, which tests/test_reference_host.py puts on whole-net runs of several steps (TOL);
# the batch-normalised net: the bound of test_small_bn_net_trains_fused_like_unfused (tests/test_batchnorm_gpu.py), whose fused
# batch-norm entries are a few ulp from the unfused sequence by design
@pytest.mark.parametrize("which,tol", [("tiny_alex", 1e-4), ("small_bn", 1e-3)])
def test_fused_training_equals_unfused_training(M, which, tol):
    from convnet_amd import models
    from convnet_amd.optimizer import AdagradSGDOptimizer, RMSPropSGDOptimizer, SGDOptimizer
    from test_net_gpu import small_alexnet
    base = small_alexnet() if which == "tiny_alex" else models.small_bn()
    for kind, cls in (("ADAGRAD_SGD", AdagradSGDOptimizer), ("RMSPROP_SGD", RMSPropSGDOptimizer), ("SGD", SGDOptimizer)):   # SGD: the control
        text = _with_optimizer(base, kind)
        a, b = _net(text, 32, False), _net(text, 32, True)
        b.parameters_.FromNumpy(a.parameters_.ToNumpy())
        p0 = a.parameters_.ToNumpy().reshape(-1).copy()
        assert all(type(o) is cls for _, o in _optimizers(a) + _optimizers(b))
        assert (a.second_history_.GetNumEls() > 0) == (kind != "SGD") == (b.second_history_.GetNumEls() > 0)
        _train(a, 4)
        _train(b, 4)
        sa, sb = _state(a), _state(b)
        assert set(sa) == set(sb) and not np.array_equal(sa["parameters"], p0)
        for name in sa:
            assert np.all(np.isfinite(sb[name])), (which, kind, name)
            err = rel_err(sb[name], sa[name])
            assert err < tol, (which, kind, name, err)
        assert all(o.step_ == 4 for _, o in _optimizers(a) + _optimizers(b))


# ---- 5. checkpoint ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ADAGRAD_SGD", "RMSPROP_SGD"])
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_checkpoint_resumes_bit_for_bit(M, tmp_path, kind, fused):
    from test_net_gpu import small_alexnet
    text = _with_optimizer(small_alexnet(), kind)
    straight = _net(text, 16, fused)
    p0 = straight.parameters_.ToNumpy()
    _train(straight, 4)
    first = _net(text, 16, fused)
    first.parameters_.FromNumpy(p0)
    _train(first, 2)
    path = str(tmp_path / "ckpt.h5")
    first.Save(path)
    resumed = _net(text, 16, fused)
    resumed.Load(path)
    mid = _state(resumed)
    assert any("second history" in k for k in mid)
    for name, v in _state(first).items():
        assert np.array_equal(mid[name], v), ("loaded", name)
    assert not np.array_equal(mid["second history"], mid["history"])    # the second moments, not the momentum a second time
    _train(resumed, 2, seed=19)
    want = _state(straight)
    for name, v in _state(resumed).items():
        assert np.array_equal(v, want[name]), (kind, name, rel_err(v, want[name]))
