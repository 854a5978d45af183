"""Locally connected layers on the GPU (convnet_amd/csrc/local_conv.hip): localUp / localDown / localOutp and their *Gemm names
against the float64 oracle (tests/local_ref.py) on both matrix paths, the layout cross-check against the conv path, the face-net-scale
layer on sampled elements, the fused bias + ReLU entry, and whole nets with LOCAL edges."""
import ctypes

import numpy as np
import pytest

import local_ref as L  # noqa: E402
from golden_cases import rel_err  # noqa: E402
from local_ref import LocalGeom  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(42)
    return True


@pytest.fixture(params=["split", "fp32"])
def matrix_path(request, gpu):
    from convnet_amd import _lib
    _lib.lib.convnet_hip_set_matrix_path(1 if request.param == "split" else 0)
    yield request.param
    _lib.lib.convnet_hip_set_matrix_path(1)


def run_up(g, x, w, t=None, st=0.0, name="localUpGemm"):
    from convnet_amd._lib import lib
    from hip_adapter import _desc, _w_local, _x, _y
    X, W, T = _x(g, x), _w_local(g, w), _y(g, t if t is not None else np.zeros(g.out_shape()))
    getattr(lib, name)(X.GetMat(), W.GetMat(), T.GetMat(), ctypes.byref(X.shape_), ctypes.byref(W.shape_), ctypes.byref(T.shape_),
                       _desc(g), float(st))
    return T.ToNumpy().reshape(g.out_shape())


def run_down(g, dy, w, t=None, st=0.0, name="localDownGemm"):
    from convnet_amd._lib import lib
    from hip_adapter import _desc, _w_local, _x, _y
    D, W, T = _y(g, dy), _w_local(g, w), _x(g, t if t is not None else np.zeros(g.in_shape()))
    getattr(lib, name)(D.GetMat(), W.GetMat(), T.GetMat(), ctypes.byref(D.shape_), ctypes.byref(W.shape_), ctypes.byref(T.shape_),
                       _desc(g), float(st))
    return T.ToNumpy().reshape(g.in_shape())


def run_outp(g, x, dy, t=None, st=0.0, so=1.0, name="localOutpGemm", guard=0):
    """guard: that many columns of guard floats follow the bank gradient in its allocation (the matrix handed to the kernel is a view)"""
    from convnet_amd._lib import lib
    from hip_adapter import _desc, _w_local, _x, _y
    X, D = _x(g, x), _y(g, dy)
    bank = _w_local(g, t if t is not None else np.zeros(g.bank_shape()), (0, guard))
    T, full = bank if guard else (bank, bank)
    getattr(lib, name)(X.GetMat(), D.GetMat(), T.GetMat(), ctypes.byref(X.shape_), ctypes.byref(D.shape_), ctypes.byref(T.shape_),
                       _desc(g), float(st), float(so))
    a = full.ToNumpy().reshape(-1)
    return a[:g.F * g.K * g.M].reshape(g.bank_shape()), a[g.F * g.K * g.M:]


def rnd(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


GEOMS = [
    LocalGeom(N=1, C=3, H=7, W=7, F=7, Ky=3, Kx=3),
    LocalGeom(N=6, C=3, H=9, W=8, F=16, Ky=3, Kx=2, sy=2, sx=1, pady=1, padx=0),
    LocalGeom(N=100, C=16, H=6, W=10, F=7, Ky=2, Kx=4, sy=1, sx=3, pady=0, padx=2),
    LocalGeom(N=128, C=16, H=11, W=11, F=16, Ky=2, Kx=2, sy=3, sx=3),                    # stride > kernel
    LocalGeom(N=256, C=64, H=5, W=5, F=64, Ky=3, Kx=3, pady=1, padx=1),
    LocalGeom(N=6, C=64, H=7, W=6, F=16, Ky=3, Kx=5, sy=2, sx=2, pady=2, padx=1),
    LocalGeom(N=128, C=64, H=5, W=5, F=64, Ky=3, Kx=3, pady=1, padx=1),                  # cifar_local's local3
    LocalGeom(N=128, C=64, H=5, W=5, F=32, Ky=3, Kx=3, pady=1, padx=1),                  # cifar_local's local4
]


@pytest.mark.parametrize("g", GEOMS, ids=str)
@pytest.mark.parametrize("st", [0.0, 1.0])
def test_local_kernels_match_the_float64_oracle(matrix_path, g, st):
    rng = np.random.default_rng(g.N + g.C)
    x, w, dy = rnd(rng, g.in_shape()), rnd(rng, g.bank_shape()), rnd(rng, g.out_shape())
    to, tx, tw = rnd(rng, g.out_shape()), rnd(rng, g.in_shape()), rnd(rng, g.bank_shape())
    so = 0.37
    names = [("localUpGemm", "localDownGemm", "localOutpGemm"), ("localUp", "localDown", "localOutp")]
    for up_n, down_n, outp_n in names:
        assert rel_err(run_up(g, x, w, to, st, up_n), L.up(g, x, w, to, st)) < 1e-4
        assert rel_err(run_down(g, dy, w, tx, st, down_n), L.down(g, dy, w, tx, st)) < 1e-4
        got, guard = run_outp(g, x, dy, tw, st, so, outp_n, guard=3)
        assert rel_err(got, L.outp(g, x, dy, tw, st, so)) < 1e-4
        assert np.all(guard == 7.0)


@pytest.mark.parametrize("g", [GEOMS[1], GEOMS[3], GEOMS[5]], ids=str)
def test_local_layout_equals_conv_when_every_module_has_the_same_bank(matrix_path, g):
    from hip_adapter import HipImpl
    from oracle import Geom
    hip = HipImpl()
    cg = Geom(N=g.N, C=g.C, H=g.H, W=g.W, F=g.F, Ky=g.Ky, Kx=g.Kx, sy=g.sy, sx=g.sx, pady=g.pady, padx=g.padx)
    rng = np.random.default_rng(11)
    x, dy = rnd(rng, g.in_shape()), rnd(rng, g.out_shape())
    wc = rnd(rng, cg.filt_shape())                       # (C, Ky, Kx, F)
    wl = np.broadcast_to(wc, (g.M,) + wc.shape).copy()   # every module block = the conv bank
    assert rel_err(run_up(g, x, wl), hip.conv_up(cg, x, wc)) < 1e-4
    assert rel_err(run_down(g, dy, wl), hip.conv_down(cg, dy, wc)) < 1e-4
    dwl, _ = run_outp(g, x, dy)
    assert rel_err(dwl.astype(np.float64).sum(0), hip.conv_outp(cg, x, dy)) < 1e-4


def test_face_net_scale_layer_on_sampled_elements(matrix_path):
    """C = 16, 63 x 63, 9 x 9, F = 16 -> 55 x 55 modules, N = 256 (bank 251 MB, 32.1 GFLOP): sampled elements in float64, the last
    module's block checked explicitly, and nothing written past the bank gradient (the reference's off-by-one)."""
    g = LocalGeom(N=256, C=16, H=63, W=63, F=16, Ky=9, Kx=9)
    rng = np.random.default_rng(2)
    x, w, dy = rnd(rng, g.in_shape()), rnd(rng, g.bank_shape()), rnd(rng, g.out_shape())
    up, down = run_up(g, x, w), run_down(g, dy, w)
    dw, guard = run_outp(g, x, dy, so=1.0 / g.N, guard=4)
    assert np.all(guard == 7.0)

    def check(got, ref):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        assert np.abs(got - ref).max() / (np.abs(got + ref).mean() + 1e-30) < 1e-4, (got, ref)

    idx = [(int(rng.integers(g.F)), int(rng.integers(g.My)), int(rng.integers(g.Mx)), int(rng.integers(g.N))) for _ in range(48)]
    idx += [(f, g.My - 1, g.Mx - 1, n) for f in (0, g.F - 1) for n in (0, g.N - 1)]
    check([up[i] for i in idx], [L.up_at(g, x, w, *i) for i in idx])
    idx = [(int(rng.integers(g.C)), int(rng.integers(g.H)), int(rng.integers(g.W)), int(rng.integers(g.N))) for _ in range(48)]
    idx += [(g.C - 1, g.H - 1, g.W - 1, g.N - 1), (0, 0, 0, 0)]
    check([down[i] for i in idx], [L.down_at(g, dy, w, *i) for i in idx])
    idx = [(int(rng.integers(g.M)), int(rng.integers(g.C)), int(rng.integers(g.Ky)), int(rng.integers(g.Kx)), int(rng.integers(g.F)))
           for _ in range(48)]
    idx += [(g.M - 1, c, ky, kx, f) for c in (0, g.C - 1) for ky in (0, g.Ky - 1) for kx in (0, g.Kx - 1) for f in (0, g.F - 1)]
    check([dw[i] for i in idx], [L.outp_at(g, x, dy, *i) / g.N for i in idx])


@pytest.mark.parametrize("g", [GEOMS[1], GEOMS[4]], ids=str)
def test_fused_bias_relu_is_bit_identical_to_the_unfused_sequence(matrix_path, g):
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _mat, _w_local, _x, _y
    rng = np.random.default_rng(4)
    x, w, b, t = rnd(rng, g.in_shape()), rnd(rng, g.bank_shape()), rnd(rng, (1, g.F * g.M)), rnd(rng, g.out_shape())
    for st, relu in ((0.0, True), (1.0, True), (0.0, False)):
        X, W, B = _x(g, x), _w_local(g, w), _mat(b, 1, g.F * g.M)
        T1, T2 = _y(g, t), _y(g, t)
        Matrix.LocalUp(X, W, T1, _desc(g), st)
        T1.AddRowVec(B)
        if relu:
            T1.LowerBound(0.0)
        Matrix.LocalUpBiasAct(X, W, B, T2, _desc(g), st, relu)
        a1, a2 = T1.ToNumpy(), T2.ToNumpy()
        assert np.array_equal(a1, a2)
        T3 = _y(g, t)
        Matrix.LocalUpBiasAct(X, W, B, T3, _desc(g), st, relu)
        assert np.array_equal(T3.ToNumpy(), a2)                      # repeated calls: bit-identical
    # the bias mapping of local_edge.cc: element j of the (1, F*M) row goes to output column j
    ref = L.up(g, x, w) + b.reshape(g.F, g.My, g.Mx)[..., None]
    X, W, B, T = _x(g, x), _w_local(g, w), _mat(b, 1, g.F * g.M), _y(g, np.zeros(g.out_shape()))
    Matrix.LocalUpBiasAct(X, W, B, T, _desc(g), 0.0, False)
    assert rel_err(T.ToNumpy().reshape(g.out_shape()), ref) < 1e-4


def test_repeated_calls_are_bit_identical(matrix_path):
    g = GEOMS[4]
    rng = np.random.default_rng(8)
    x, w, dy = rnd(rng, g.in_shape()), rnd(rng, g.bank_shape()), rnd(rng, g.out_shape())
    assert np.array_equal(run_up(g, x, w), run_up(g, x, w))
    assert np.array_equal(run_down(g, dy, w), run_down(g, dy, w))
    assert np.array_equal(run_outp(g, x, dy)[0], run_outp(g, x, dy)[0])


# ---- whole nets -------------------------------------------------------------------------------------------------------------------
def _small_local_net(grad_check=False):
    # (no padding on the first edge: the checked parameters are the first ten of module 0, which a padding tap would leave at an
    # all-zero gradient — 0/0, a failed check in the reference's criterion)
    from convnet_amd import models
    gc = models._gc(grad_check)
    s = models._header("small_local") + models._layer("input", 3, size=8)
    s += models._layer("l1", 6, "RECTIFIED_LINEAR") + models._layer("l2", 5, "RECTIFIED_LINEAR") + models._layer("output", 4, "SOFTMAX")
    s += models._local("input", "l1", 3, 1, 0, init_bias=0.1, grad_check=gc) + models._local("l1", "l2", 3, 2, 0, init_bias=0.1, grad_check=gc)
    return s + models._fc("l2", "output", grad_check=gc)


def test_cifar_local_trains_the_same_fused_and_unfused(gpu):
    from convnet_amd import _lib, models
    from test_net_gpu import build
    _lib.lib.convnet_hip_set_matrix_path(1)
    a = build(models.cifar_local(), 128, fused=True)
    b = build(models.cifar_local(), 128, fused=False)
    b.parameters_.Set(a.parameters_)
    for _ in range(3):
        a.TrainOneBatch()
        b.TrainOneBatch()
    pa, pb = a.parameters_.ToNumpy(), b.parameters_.ToNumpy()
    assert np.all(np.isfinite(pa)) and rel_err(pa, pb) < 1e-4


def test_grad_checker_passes_on_a_net_with_two_local_edges(gpu):
    from convnet_amd import _lib
    from convnet_amd.grad_check import GradChecker
    from convnet_amd.datahandler import SyntheticDataHandler
    _lib.lib.convnet_hip_set_matrix_path(0)
    try:
        net = GradChecker(_small_local_net(grad_check=True), fused=False)
        net.SetBatchsize(6)
        net.SetupDataset(SyntheticDataHandler(net, 6, seed=3, num_batches=1))
        net.AllocateMemory(False)
        res = net.Run(fixed_batch=True)
    finally:
        _lib.lib.convnet_hip_set_matrix_path(1)
    assert {"input:l1", "l1:l2"} <= set(res)
    for name in ("input:l1", "l1:l2"):
        for kind in ("weights", "bias"):
            assert res[name][kind][0], (name, kind, res[name][kind])


def test_one_sgd_step_matches_float64_numpy(gpu):
    """input -> local (no activation) -> fc -> softmax: the local edge's weight and bias gradients of one training pass against a
    float64 numpy evaluation of the same net at the same parameters and batch."""
    from convnet_amd import models
    from test_net_gpu import build
    s = models._header("one_step") + models._layer("input", 3, size=6) + models._layer("h", 4) + models._layer("output", 5, "SOFTMAX")
    s += models._local("input", "h", 3, 2, 1, l2=0.0) + models._fc("h", "output", l2=0.0)
    net = build(s, 7, fused=False)
    for l in net.layers_:
        l.ResetAddOrOverwrite()
    net.GetBatch(net.train_dataset_)
    x = net.input_layers_[0].GetState().ToNumpy().reshape(-1)
    labels = net.output_layers_[0].GetData().ToNumpy().reshape(-1).astype(int)
    net.Fprop(True)
    net.ComputeDeriv()
    net.Bprop()
    le, fe = net.GetEdgeByName("input:h"), net.GetEdgeByName("h:output")
    g = LocalGeom(N=7, C=3, H=6, W=6, F=4, Ky=3, Kx=3, sy=2, sx=2, pady=1, padx=1)
    W = le.GetWeight().ToNumpy().reshape(-1).astype(np.float64).reshape(g.bank_shape())
    b = le.GetBias().ToNumpy().reshape(-1).astype(np.float64)
    xa = x.astype(np.float64).reshape(g.in_shape())
    h = L.up(g, xa, W).reshape(g.F * g.M, g.N).T + b[None, :]          # (N, F*M): column j = f*M + m gets bias element j
    Wfc = fe.GetWeight().ToNumpy().reshape(-1).astype(np.float64).reshape(g.F * g.M, 5).T   # (5, F*M), column-major storage
    fb = fe.GetBias().ToNumpy().reshape(-1).astype(np.float64)
    logits = h @ Wfc.T + fb[None, :]
    p = np.exp(logits - logits.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    d = p.copy()
    d[np.arange(g.N), labels] -= 1.0
    dh = d @ Wfc                                                        # (N, F*M)
    dyl = dh.T.reshape(g.out_shape())
    gw = L.outp(g, xa, dyl, scale_output=1.0 / g.N)
    gb = dh.sum(0) / g.N
    assert rel_err(le.GetGradWeight().ToNumpy().reshape(-1), gw.reshape(-1)) < 1e-4
    assert rel_err(le.GetGradBias().ToNumpy().reshape(-1), gb) < 1e-4


def test_local_edge_slices_and_checkpoint_round_trip(gpu, tmp_path):
    from test_net_gpu import build
    net = build(_small_local_net(), 4, fused=True)
    e = net.GetEdgeByName("input:l1")
    g = LocalGeom(N=4, C=3, H=8, W=8, F=6, Ky=3, Kx=3)
    n, wshape, bshape, s4 = L.local_edge_sizes(g)
    assert (e.GetWeight().GetRows(), e.GetWeight().GetCols()) == wshape
    assert (e.GetBias().GetRows(), e.GetBias().GetCols()) == bshape
    assert tuple(e.GetWeight().shape_.shape) == s4
    assert tuple(e.GetGradWeight().shape_.shape) == s4
    net.TrainOneBatch()
    before = {x.GetName(): (x.GetWeight().ToNumpy().copy(), x.GetBias().ToNumpy().copy()) for x in net.edges_ if x.GetParameterMemoryRequirement()}
    f = str(tmp_path / "ck.h5")
    net.Save(f)
    net2 = build(_small_local_net(), 4, fused=True)
    net2.Load(f)
    for name, (w, b) in before.items():
        e2 = net2.GetEdgeByName(name)
        assert np.array_equal(e2.GetWeight().ToNumpy(), w) and np.array_equal(e2.GetBias().ToNumpy(), b), name
