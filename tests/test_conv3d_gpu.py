"""Spatio-temporal (3-D) convolution, response norm and pooling on the GPU (convnet_amd/csrc/conv3d.hip) against the float64 statement
of tests/conv3d_ref.py and against the loop of this library's 2-D entries over get_slice views, on both matrix paths; fused entries
against their unfused sequences; pooling over time; whole video nets through the host."""
import ctypes

import numpy as np
import pytest

import conv3d_ref as R  # noqa: E402
from conv3d_ref import Geom3D  # noqa: E402
from golden_cases import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4   # tests/test_hip_parity.py: the reference's own kernel-test tolerance


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


GUARD = 3   # guard columns before and after a guarded tensor
GUARDED = (GUARD, GUARD)


def _guards_intact(full, rows):
    a = full.ToNumpy().reshape(-1)
    return bool(np.all(a[:GUARD * rows] == 7.0) and np.all(a[-GUARD * rows:] == 7.0))


def _bytes(*ms):
    from convnet_amd._lib import cudamat
    return b"".join(ctypes.string_at(ctypes.addressof(m.mat_), ctypes.sizeof(cudamat)) + bytes(m.shape_) for m in ms)


def _frames(m, first, count, frame_cols, shape4):
    from convnet_amd.matrix import Matrix
    v = Matrix()
    m.GetSlice(v, first * frame_cols, (first + count) * frame_cols)
    v.SetShape4D(*shape4)
    return v


def _loop_2d(g, X, W, DY, what, T, st=0.0, so=1.0):
    """The reference's form on THIS library: its 2-D entries over get_slice views, frame by frame (cudamat_conv3d_gemm.cu)."""
    from convnet_amd.matrix import Matrix, make_conv_desc
    d2 = make_conv_desc(g.C * g.Kt, g.F, g.Ky, g.Kx, g.sy, g.sx, g.pady, g.padx)
    fin, fout = g.H * g.W * g.C, g.My * g.Mx * g.F
    W2 = _frames(W, 0, 1, W.GetCols(), (g.F, g.Kx, g.Ky, g.C * g.Kt))
    if what == "down":
        T.Mult(st)     # Scale(targets, scaleTargets), then every frame accumulates
    for m in range(g.Mt):
        xs = _frames(X if what != "down" else T, m * g.st, g.Kt, fin, (g.N, g.W, g.H, g.C * g.Kt))
        ys = _frames(DY if what != "up" else T, m, 1, fout, (g.N, g.Mx, g.My, g.F))
        if what == "up":
            Matrix.ConvUp(xs, W2, ys, d2, st)
        elif what == "down":
            Matrix.ConvDown(ys, W2, xs, d2, 1.0)
        else:
            Matrix.ConvOutp(xs, ys, T, d2, 0, 0, st if m == 0 else 1.0, so)


SHAPES = {
    "c3_first_layer": dict(C=3, H=12, W=12, T=6, F=32, Ky=3, Kx=3, Kt=3, pady=1, padx=1),
    "c16_3x3_rows10": dict(C=16, H=10, W=10, T=5, F=32, Ky=3, Kx=3, Kt=3, pady=1, padx=1),
    "c16_5x5_s2_st2": dict(C=16, H=13, W=13, T=7, F=48, Ky=5, Kx=5, Kt=3, sy=2, sx=2, st=2),
    "f12_st_gt_kt": dict(C=16, H=7, W=7, T=8, F=12, Ky=3, Kx=3, Kt=2, st=3, pady=1, padx=1),     # frames 2, 5 uncovered (dgrad: gather)
    "c8_st_gt_kt": dict(C=8, H=7, W=7, T=8, F=24, Ky=3, Kx=3, Kt=2, st=3, pady=1, padx=1),        # the same with dgrad as the loop
}
CASES = [(s, n) for s in SHAPES for n in (4, 32, 64, 128)]


def _data(g, seed=0):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in (g.in_shape(), g.filt_shape(), g.out_shape()))


@pytest.mark.parametrize("shape,N", CASES, ids=[f"{s}-N{n}" for s, n in CASES])
def test_conv3d_entries_against_ref_and_2d_loop(matrix_path, shape, N):
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _w, _x, _y
    g = Geom3D(N=N, **SHAPES[shape])
    x, w, dy = _data(g, seed=N)
    rng = np.random.default_rng(1)
    t_up, t_dn, t_w = (rng.standard_normal(s).astype(np.float32) for s in (g.out_shape(), g.in_shape(), g.filt_shape()))
    ref_up, ref_dn, ref_w = R.conv_up(g, x, w), R.conv_down(g, dy, w), R.conv_outp(g, x, dy, None, 0.0, 0.5)
    d = _desc(g)
    X, W, DY = _x(g, x), _w(g, w), _y(g, dy)
    before = _bytes(X, W, DY)
    for st in (0.0, 1.0):
        # forward: against the float64 statement, and bit for bit the 2-D loop
        T1, F1 = _y(g, t_up, guard=GUARDED)
        Matrix.Conv3DUp(X, W, T1, d, st)
        up = T1.ToNumpy().reshape(g.out_shape())
        e = rel_err(up, st * t_up + ref_up)
        print(f"{shape} N={N} {matrix_path} st={st}: up {e:.2e}", end=" ")
        assert e < TOL and _guards_intact(F1, N)
        T2 = _y(g, t_up)
        _loop_2d(g, X, W, DY, "up", T2, st)
        assert np.array_equal(up, T2.ToNumpy().reshape(g.out_shape())), "forward differs from the loop of 2-D entries"
        T3 = _y(g, t_up)
        Matrix.Conv3DUp(X, W, T3, d, st)
        assert np.array_equal(up, T3.ToNumpy().reshape(g.out_shape())), "forward is not bit-identical from run to run"
        # dgrad: every input frame written (uncovered ones included), nothing outside the tensor
        T1, F1 = _x(g, t_dn, guard=GUARDED)
        Matrix.Conv3DDown(DY, W, T1, d, st)
        dn = T1.ToNumpy().reshape(g.in_shape())
        e = rel_err(dn, st * t_dn + ref_dn)
        print(f"down {e:.2e}", end=" ")
        assert e < TOL and _guards_intact(F1, N)
        covered = {m * g.st + k for m in range(g.Mt) for k in range(g.Kt)}
        for ti in set(range(g.T)) - covered:
            assert np.array_equal(dn[ti], np.float32(st) * t_dn[ti]), f"uncovered frame {ti}"
        T2 = _x(g, t_dn)
        _loop_2d(g, X, W, DY, "down", T2, st)
        assert rel_err(dn, T2.ToNumpy().reshape(g.in_shape())) < TOL
        T3 = _x(g, t_dn)
        Matrix.Conv3DDown(DY, W, T3, d, st)
        assert np.array_equal(dn, T3.ToNumpy().reshape(g.in_shape())), "dgrad is not bit-identical from run to run"
        # wgrad
        T1, F1 = _w(g, t_w, guard=GUARDED)
        Matrix.Conv3DOutp(X, DY, T1, d, st, 0.5)
        dw = T1.ToNumpy().reshape(g.filt_shape())
        e = rel_err(dw, st * t_w + ref_w)
        print(f"outp {e:.2e}")
        assert e < TOL and _guards_intact(F1, g.F)
        T2 = _w(g, t_w)
        _loop_2d(g, X, W, DY, "outp", T2, st, 0.5)
        assert rel_err(dw, T2.ToNumpy().reshape(g.filt_shape())) < TOL
        T3 = _w(g, t_w)
        Matrix.Conv3DOutp(X, DY, T3, d, st, 0.5)
        assert np.array_equal(dw, T3.ToNumpy().reshape(g.filt_shape())), "wgrad is not bit-identical from run to run"
    assert _bytes(X, W, DY) == before, "a 3-D entry wrote to its caller's cudamat structs"


@pytest.mark.parametrize("shape,N", [("c3_first_layer", 32), ("c16_3x3_rows10", 64), ("c16_5x5_s2_st2", 4), ("f12_st_gt_kt", 128)])
def test_fused_conv3d_entries_equal_their_unfused_sequences(matrix_path, shape, N):
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _mat, _w, _x, _y
    g = Geom3D(N=N, **SHAPES[shape])
    x, w, dy = _data(g, seed=7)
    rng = np.random.default_rng(2)
    bias = rng.standard_normal(g.F).astype(np.float32)
    state = rng.standard_normal(g.in_shape()).astype(np.float32)
    t_dn = rng.standard_normal(g.in_shape()).astype(np.float32)
    d = _desc(g)
    X, W, DY, B, S = _x(g, x), _w(g, w), _y(g, dy), _mat(bias, 1, g.F), _x(g, state)
    # convUp3DBiasAct == convUp3DGemm + the shared bias per output frame + ReLU (conv_edge.cc:155-164, layer.cc:549)
    for relu in (0, 1):
        A = _y(g, np.zeros(g.out_shape()))
        Matrix.Conv3DUpBiasAct(X, W, B, A, d, 0.0, relu)
        U = _y(g, np.zeros(g.out_shape()))
        Matrix.Conv3DUp(X, W, U, d, 0.0)
        U.Reshape(-1, g.F * g.Mt)
        for m in range(g.Mt):
            s = Matrix()
            U.GetSlice(s, m * g.F, (m + 1) * g.F)
            s.AddRowVec(B)
        U.Reshape(N, -1)
        if relu:
            U.LowerBound(0.0)
        assert np.array_equal(A.ToNumpy(), U.ToNumpy()), f"convUp3DBiasAct relu={relu}"
        A2 = _y(g, np.zeros(g.out_shape()))
        Matrix.Conv3DUpBiasAct(X, W, B, A2, d, 0.0, relu)
        assert np.array_equal(A.ToNumpy(), A2.ToNumpy()), "convUp3DBiasAct is not bit-identical from run to run"
        assert rel_err(A.ToNumpy().reshape(g.out_shape()),
                       (np.maximum if relu else lambda a, b: a)(R.conv_up(g, x, w) + bias.reshape(1, -1, 1, 1, 1), 0.0)) < TOL
    # convDown3DMask == convDown3DGemm + ReLU' of the source layer (layer.cc:556-558), accumulated target included
    for st in (0.0, 1.0):
        A, FA = _x(g, t_dn, guard=GUARDED)
        Matrix.Conv3DDownMask(DY, W, S, A, d, st, 1.0)
        U = _x(g, t_dn)
        Matrix.Conv3DDown(DY, W, U, d, st)
        U.ApplyDerivativeOfReLU(S)
        assert np.array_equal(A.ToNumpy(), U.ToNumpy()), f"convDown3DMask st={st}"
        A2 = _x(g, t_dn)
        Matrix.Conv3DDownMask(DY, W, S, A2, d, st, 1.0)
        assert np.array_equal(A.ToNumpy(), A2.ToNumpy()), "convDown3DMask is not bit-identical from run to run"
        assert _guards_intact(FA, N)
    A = _x(g, t_dn)
    Matrix.Conv3DDownMask(DY, W, S, A, d, 0.0, 0.5)
    assert rel_err(A.ToNumpy().reshape(g.in_shape()), 0.5 * R.conv_down(g, dy, w) * (state > 0)) < TOL
    # convOutp3DBias: dW as convOutp3DGemm, and the shared-bias gradient summed over images, pixels and frames
    for st in (0.0, 1.0):
        t_w, t_b = rng.standard_normal(g.filt_shape()).astype(np.float32), rng.standard_normal(g.F).astype(np.float32)
        A, (DB, FDB) = _w(g, t_w), _mat(t_b, 1, g.F, guard=GUARDED)
        Matrix.Conv3DOutpBias(X, DY, A, DB, d, st, 0.25)
        U = _w(g, t_w)
        Matrix.Conv3DOutp(X, DY, U, d, st, 0.25)
        assert np.array_equal(A.ToNumpy(), U.ToNumpy()), f"convOutp3DBias dW st={st}"
        A2, DB2 = _w(g, t_w), _mat(t_b, 1, g.F)
        Matrix.Conv3DOutpBias(X, DY, A2, DB2, d, st, 0.25)
        assert np.array_equal(A.ToNumpy(), A2.ToNumpy()) and np.array_equal(DB.ToNumpy(), DB2.ToNumpy()), "convOutp3DBias is not bit-identical from run to run"
        assert rel_err(DB.ToNumpy().reshape(-1), st * t_b + 0.25 * dy.astype(np.float64).sum(axis=(0, 2, 3, 4))) < TOL and _guards_intact(FDB, 1)


@pytest.mark.parametrize("C,F", [(32, 64), (64, 256)], ids=["K256_F64", "K512_F256"])
def test_fused_bias_gradient_beside_the_batched_dw_slabs(matrix_path, C, F):
    """convOutp3DBias where the weight-gradient tile has NO spare row for the bias (K = C*Kt*Ky*Kx a multiple of the k tile: 128 / 256)
    and the column sum of derivs is tall enough (N*My*Mx >= 32768 rows) to take split scratch of its own: the per-frame column sums
    run between the frame launches and the call's one dW reduction, and must not touch the frames' slabs.  dW bit for bit
    convOutp3DGemm's, db against float64."""
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _mat, _w, _x, _y
    g = Geom3D(N=64, C=C, H=24, W=24, T=4, F=F, Ky=2, Kx=2, Kt=2)
    assert (g.C * g.Kt * g.Ky * g.Kx) % 256 == 0 and g.N * g.My * g.Mx >= 32768 and g.Mt == 3
    x, w, dy = _data(g, seed=C)
    rng = np.random.default_rng(4)
    d = _desc(g)
    X, DY = _x(g, x), _y(g, dy)
    for st in (0.0, 1.0):
        t_w, t_b = rng.standard_normal(g.filt_shape()).astype(np.float32), rng.standard_normal(g.F).astype(np.float32)
        (A, FA), (DB, FDB) = _w(g, t_w, guard=GUARDED), _mat(t_b, 1, g.F, guard=GUARDED)
        Matrix.Conv3DOutpBias(X, DY, A, DB, d, st, 0.25)
        U = _w(g, t_w)
        Matrix.Conv3DOutp(X, DY, U, d, st, 0.25)
        assert np.array_equal(A.ToNumpy(), U.ToNumpy()), f"convOutp3DBias dW differs from convOutp3DGemm's, st={st}"
        e = rel_err(DB.ToNumpy().reshape(-1), st * t_b + 0.25 * dy.astype(np.float64).sum(axis=(0, 2, 3, 4)))
        print(f"C={C} F={F} {matrix_path} st={st}: db {e:.2e}")
        assert e < TOL and _guards_intact(FA, g.F) and _guards_intact(FDB, 1)
        # and dW itself against the loop of 2-D entries (the unbatched form), so that both sides cannot be wrong together
        L = _w(g, t_w)
        W0 = _w(g, w)
        _loop_2d(g, X, W0, DY, "outp", L, st, 0.25)
        assert rel_err(A.ToNumpy(), L.ToNumpy()) < TOL


@pytest.mark.parametrize("C,size_f,N,T,blocked", [(16, 5, 32, 4, False), (64, 16, 4, 3, False), (96, 24, 64, 2, False), (20, 5, 128, 3, True)])
def test_rnorm3d_is_the_2d_operation_on_every_frame(gpu, C, size_f, N, T, blocked):
    from convnet_amd.matrix import Matrix
    from hip_adapter import _mat
    rng = np.random.default_rng(C)
    x, dy = (rng.standard_normal((T, C, 5, 6, N)).astype(np.float32) for _ in range(2))
    X, DY, (Y, FY), YR, (DX, FDX) = (_mat(a, N, a.size // N, None, gd) for a, gd in
                                         ((x, (0, 0)), (dy, (0, 0)), (np.zeros_like(x), GUARDED), (np.zeros_like(x), (0, 0)), (np.zeros_like(x), GUARDED)))
    before = _bytes(X, DY)
    Matrix.ConvResponseNormCrossMap3D(X, Y, C, size_f, 0.01, 0.75, blocked, T)
    Matrix.ConvResponseNormCrossMap3D(X, YR, C, size_f, 0.01, 0.75, blocked, T, relu=True)
    Matrix.ConvResponseNormCrossMapUndo3D(DY, X, Y, DX, C, size_f, 0.01, 0.75, blocked, T)
    y, dx = Y.ToNumpy().reshape(x.shape), DX.ToNumpy().reshape(x.shape)
    Y2, YR2, DX2 = (_mat(np.zeros_like(x), N, x.size // N) for _ in range(3))   # run-to-run bit-identity
    Matrix.ConvResponseNormCrossMap3D(X, Y2, C, size_f, 0.01, 0.75, blocked, T)
    Matrix.ConvResponseNormCrossMap3D(X, YR2, C, size_f, 0.01, 0.75, blocked, T, relu=True)
    Matrix.ConvResponseNormCrossMapUndo3D(DY, X, Y2, DX2, C, size_f, 0.01, 0.75, blocked, T)
    assert np.array_equal(Y2.ToNumpy().reshape(x.shape), y) and np.array_equal(DX2.ToNumpy().reshape(x.shape), dx)
    assert np.array_equal(YR2.ToNumpy(), YR.ToNumpy())
    assert rel_err(y, R.rnorm(x, size_f, 0.01, 0.75, blocked)) < TOL and rel_err(dx, R.rnorm_undo(dy, x, size_f, 0.01, 0.75, blocked)) < TOL
    assert np.array_equal(YR.ToNumpy().reshape(x.shape), np.maximum(y, 0.0)), "ResponseNormCrossMap3DRelu != rnorm + ReLU"
    assert _guards_intact(FY, N) and _guards_intact(FDX, N) and _bytes(X, DY) == before
    frame = x[0].size // N
    for t in range(T):   # bit for bit the 2-D entries on the frame's slice
        xs, ds = _frames(X, t, 1, frame, (N, 6, 5, C)), _frames(DY, t, 1, frame, (N, 6, 5, C))
        y2, d2 = _mat(np.zeros_like(x[0]), N, frame), _mat(np.zeros_like(x[0]), N, frame)
        Matrix.ConvResponseNormCrossMap(xs, y2, C, size_f, 0.01, 0.75, blocked)
        Matrix.ConvResponseNormCrossMapUndo(ds, xs, y2, d2, C, size_f, 0.01, 0.75, blocked)
        assert np.array_equal(y2.ToNumpy().reshape(x[0].shape), y[t]) and np.array_equal(d2.ToNumpy().reshape(x[0].shape), dx[t])


POOLS = [
    Geom3D(N=32, C=16, H=9, W=9, T=6, F=16, Ky=3, Kx=3, Kt=2, sy=2, sx=2, st=2),
    Geom3D(N=4, C=8, H=7, W=6, T=7, F=8, Ky=3, Kx=2, Kt=3, sy=2, sx=1, st=2, pady=1, padx=0, padt=1),     # clipped in time and y
    Geom3D(N=64, C=4, H=6, W=6, T=9, F=4, Ky=2, Kx=2, Kt=2, sy=2, sx=2, st=3),                             # frames nobody pools
    Geom3D(N=128, C=3, H=5, W=5, T=4, F=3, Ky=5, Kx=5, Kt=4, sy=5, sx=5, st=1),                            # one box over everything
    Geom3D(N=6, C=5, H=8, W=8, T=5, F=5, Ky=3, Kx=3, Kt=1, sy=2, sx=2, st=2),                              # N % 4 != 0; Kt = 1 with a stride
]


@pytest.mark.parametrize("g", POOLS, ids=str)
def test_pooling_over_time(gpu, g):
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _mat, _x, _y, last_kernel
    rng = np.random.default_rng(g.N)
    d = _desc(g, pool=True)
    # small integers: many ties, and every sum of routed derivatives is exact in fp32 -> max pooling compares exactly
    x = rng.integers(-4, 5, g.in_shape()).astype(np.float32)
    dy = rng.integers(-4, 5, g.pooled_shape()).astype(np.float32)
    t_in = rng.integers(-4, 5, g.in_shape()).astype(np.float32)
    X, DY, (Y, FY) = _x(g, x), _y(g, dy, pool=True), _y(g, np.zeros(g.pooled_shape()), guard=GUARDED, pool=True)
    before = _bytes(X, DY)
    Matrix.ConvMaxPool(X, Y, d)
    assert last_kernel()[0].startswith("pool3d_fwd_kernel<max>/")
    y = Y.ToNumpy().reshape(g.pooled_shape())
    assert np.array_equal(y, R.max_pool(g, x)) and _guards_intact(FY, g.N)
    for st in (0.0, 1.0):
        DX, FDX = _x(g, t_in, guard=GUARDED)
        Matrix.ConvMaxPoolUndo(X, DY, Y, DX, d, st)
        assert np.array_equal(DX.ToNumpy().reshape(g.in_shape()), R.max_pool_undo(g, x, dy, y, t_in, st)) and _guards_intact(FDX, g.N)
    DX = _x(g, t_in)
    Matrix.ConvMaxPoolUndoRelu(X, DY, Y, DX, d, 0.0)
    assert np.array_equal(DX.ToNumpy().reshape(g.in_shape()), R.max_pool_undo(g, x, dy, y) * (x > 0))
    # averages on real-valued data, against float64
    xr, dyr = rng.standard_normal(g.in_shape()).astype(np.float32), rng.standard_normal(g.pooled_shape()).astype(np.float32)
    XR, DYR, (YA, FYA) = _x(g, xr), _y(g, dyr, pool=True), _y(g, np.zeros(g.pooled_shape()), guard=GUARDED, pool=True)
    Matrix.ConvAvgPool(XR, YA, d)
    e1 = rel_err(YA.ToNumpy().reshape(g.pooled_shape()), R.avg_pool(g, xr))
    assert e1 < TOL and _guards_intact(FYA, g.N)
    for st in (0.0, 1.0):
        DX, FDX = _x(g, t_in, guard=GUARDED)
        Matrix.ConvAvgPoolUndo(DYR, DX, d, st)
        e2 = rel_err(DX.ToNumpy().reshape(g.in_shape()), R.avg_pool_undo(g, dyr, t_in, st))
        print(f"{g}: avg fwd {e1:.2e} undo(st={st}) {e2:.2e}")
        assert e2 < TOL and _guards_intact(FDX, g.N)
    assert _bytes(X, DY) == before
    # run-to-run bit-identity of the four kernels, on the real-valued data
    runs = []
    for _ in range(2):
        YM, YV, DM, DV = (_y(g, np.zeros(g.pooled_shape()), pool=True), _y(g, np.zeros(g.pooled_shape()), pool=True),
                                              _x(g, t_in), _x(g, t_in))
        Matrix.ConvMaxPool(XR, YM, d)
        Matrix.ConvAvgPool(XR, YV, d)
        Matrix.ConvMaxPoolUndo(XR, DYR, YM, DM, d, 1.0)
        Matrix.ConvAvgPoolUndo(DYR, DV, d, 1.0)
        runs.append([m.ToNumpy() for m in (YM, YV, DM, DV)])
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "pooling over time is not bit-identical from run to run"
    # the mask pair is 2-D only: refuses, touches nothing
    M, Y2 = _mat(np.full(g.N * ((y.size // g.N + 1) // 2), 5.0), g.N, (y.size // g.N + 1) // 2), _y(g, np.full(g.pooled_shape(), 5.0), pool=True)
    assert Matrix.ConvMaxPoolMask(X, Y2, M, d) is False
    assert np.all(Y2.ToNumpy() == 5.0) and np.all(M.ToNumpy() == 5.0)


@pytest.mark.parametrize("N,K,S,pad", [(32, 3, 2, 0), (4, 3, 2, 1), (64, 2, 2, 0), (128, 4, 3, 1)])
def test_frames_behind_a_2d_window_are_channels_bit_for_bit(gpu, N, K, S, pad):
    """T > 1 with kernel_size_t = 1, stride_t = 1, padding_t = 0: today's 2-D call on C*T channels, to the bit (mask pair included)."""
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _mat, _x, _y
    C, T = 8, 3
    g = Geom3D(N=N, C=C, H=11, W=11, T=T, F=C, Ky=K, Kx=K, Kt=1, sy=S, sx=S, st=1, pady=pad, padx=pad)
    g2 = Geom3D(N=N, C=C * T, H=11, W=11, T=1, F=C * T, Ky=K, Kx=K, Kt=1, sy=S, sx=S, st=1, pady=pad, padx=pad)
    rng = np.random.default_rng(N)
    x, dy = rng.standard_normal(g.in_shape()).astype(np.float32), rng.standard_normal(g.pooled_shape()).astype(np.float32)
    out = {}
    for key, gg in (("frames", g), ("channels", g2)):
        d = _desc(gg, pool=True)
        X, DY = _x(g, x), _y(g, dy, pool=True)
        res = []
        for fwd, undo in ((Matrix.ConvMaxPool, "max"), (Matrix.ConvAvgPool, "avg")):
            Y = _y(g, np.zeros(g.pooled_shape()), pool=True)
            fwd(X, Y, d)
            DX = _x(g, np.zeros(g.in_shape()))
            if undo == "max":
                Matrix.ConvMaxPoolUndo(X, DY, Y, DX, d, 0.0)
            else:
                Matrix.ConvAvgPoolUndo(DY, DX, d, 0.0)
            res += [Y.ToNumpy(), DX.ToNumpy()]
        Y = _y(g, np.zeros(g.pooled_shape()), pool=True)
        M = _mat(np.zeros(N * ((Y.GetCols() + 1) // 2)), N, (Y.GetCols() + 1) // 2)
        ok = Matrix.ConvMaxPoolMask(X, Y, M, d)
        res += [np.asarray(ok), Y.ToNumpy() if ok else None, M.ToNumpy() if ok else None]
        out[key] = res
    for a, b in zip(out["frames"], out["channels"]):
        assert (a is None and b is None) or np.array_equal(a, b)
    assert rel_err(out["frames"][0].reshape(g.pooled_shape()), R.max_pool(g, x)) < TOL


# ---- whole nets -------------------------------------------------------------------------------------------------------------------------
def _build(text, batch, fused, seed_data=5):
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import SyntheticDataHandler
    net = ConvNet(text, fused=fused)
    net.SetBatchsize(batch)
    net.SetupDataset(SyntheticDataHandler(net, batch, seed=seed_data, num_batches=1))
    net.AllocateMemory(False)
    return net


def _pass(net):
    for l in net.layers_:
        l.ResetAddOrOverwrite()
    net.GetBatch(net.train_dataset_)
    net.Fprop(True)
    net.ComputeDeriv()
    net.Bprop()


def test_video_small_gradients_match_float64_whole_net(matrix_path):
    """One Fprop / ComputeDeriv / Bprop of the unfused host on video_small at N = 32: every layer state against the float64 forward
    pass, and every layer derivative and weight / bias gradient against the float64 backward ops.  The backward ops are fed the
    device's own states and incoming derivatives (as tests/test_net_gpu.py does for its deep net): ~1.2 M ReLU units and 0.8 M pooling
    boxes per image always hold a few that gate differently within fp32 rounding, and each would colour everything upstream."""
    from convnet_amd import models
    N = 32
    net = _build(models.video_small(), N, fused=False)
    _pass(net)
    x = net.input_layers_[0].GetState().ToNumpy()
    labels = net.output_layers_[0].GetData().ToNumpy().reshape(-1)
    force = ({l.GetName(): l.GetState().ToNumpy().reshape(-1) for l in net.layers_},
             {l.GetName(): l.GetDeriv().ToNumpy().reshape(-1) for l in net.layers_ if not l.IsInput()})
    acts, derivs, grads = R.forward_backward(net, x, labels, force=force)
    for l in net.layers_:
        e = rel_err(l.GetState().ToNumpy().reshape(-1), acts[l.GetName()])
        print(f"state {l.GetName()}: {e:.2e}")
        assert e < TOL, ("state", l.GetName(), e)
        if l.GetName() in derivs and not l.IsInput():
            e = rel_err(l.GetDeriv().ToNumpy().reshape(-1), derivs[l.GetName()])
            print(f"deriv {l.GetName()}: {e:.2e}")
            assert e < TOL, ("deriv", l.GetName(), e)
    for ed in net.edges_:
        if ed.GetName() in grads:
            dw, db = grads[ed.GetName()]
            ew, eb = rel_err(ed.GetGradWeight().ToNumpy().reshape(-1), dw), rel_err(ed.GetGradBias().ToNumpy().reshape(-1), db)
            print(f"grad {ed.GetName()}: dW {ew:.2e} db {eb:.2e}")
            assert ew < TOL and eb < TOL, (ed.GetName(), ew, eb)


def test_video_small_fused_host_equals_unfused_host_over_two_steps(gpu):
    from convnet_amd import models
    a, b = _build(models.video_small(), 32, fused=False), _build(models.video_small(), 32, fused=True)
    b.parameters_.Set(a.parameters_)
    for _ in range(2):
        for net in (a, b):
            net.train_dataset_.pos_ = 0
            net.TrainOneBatch()
    for ea, eb in zip(a.edges_, b.edges_):
        if ea.GetParameterMemoryRequirement():
            ew, ebias = rel_err(ea.GetWeight().ToNumpy(), eb.GetWeight().ToNumpy()), rel_err(ea.GetBias().ToNumpy(), eb.GetBias().ToNumpy())
            print(f"{ea.GetName()}: weight {ew:.2e} bias {ebias:.2e}")
            assert ew < TOL and ebias < TOL, (ea.GetName(), ew, ebias)
    assert not np.array_equal(a.parameters_.ToNumpy(), np.zeros_like(a.parameters_.ToNumpy()))


def test_video_small_checkpoint_resume_is_bit_exact(gpu, tmp_path):
    from convnet_amd import models
    a = _build(models.video_small(), 32, fused=True, seed_data=9)
    for _ in range(2):
        a.TrainOneBatch()
    path = str(tmp_path / "video.h5")
    a.Save(path)
    b = _build(models.video_small(), 32, fused=True, seed_data=9)
    b.parameters_.Mult(0.5)
    b.Load(path)
    for net in (a, b):
        net.train_dataset_.pos_ = 0
        net.TrainOneBatch()
    for ea, eb in zip(a.edges_, b.edges_):
        if ea.GetParameterMemoryRequirement():
            assert np.array_equal(ea.GetWeight().ToNumpy(), eb.GetWeight().ToNumpy()), ea.GetName()
            assert np.array_equal(ea.GetBias().ToNumpy(), eb.GetBias().ToNumpy()), ea.GetName()
            assert np.array_equal(ea.weight_optimizer_.gradient_history_.ToNumpy(), eb.weight_optimizer_.gradient_history_.ToNumpy())
