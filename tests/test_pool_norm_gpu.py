"""GPU: 2-D pooling (MaxPoolGemm, AvgPoolGemm, MaxPoolUndoGemm, MaxPoolUndoRelu, AvgPoolUndoGemm) and cross-map response norm
(ResponseNormCrossMapGemm / Relu / UndoGemm) on every launch path of convnet_amd/csrc/pool_norm.hip, against the float64 reference of
tests/pool_norm_ref.py (held against the oracle's compiled C by tests/test_pool_norm_ref_cpu.py).

Every tensor sits between guard floats of 7.0 in one allocation: "aligned" four floats in, "misaligned" one float in
(data_device % 16 == 4); guards and input operands are checked after every call.  Test ids carry the kernel that
pool_norm_ref.expected_path expects, a restatement of the dispatch; after every call the library's own report of the kernel and grid it
launched (convnet_hip_last_kernel_info) is held against that restatement (_ran).

Pooling.  Max pooling and its undo run on integer data (negative maxima, ties, an all -5 tensor whose padded taps must not count as 0)
with the scales 0, 1, -2, 0.5: every result is exact in any float32 order (CPU file), so the comparison is np.array_equal.  The averages
run on N(0, 1) and on 2^[-6, 6]-scaled data under per-element bounds counted from the operations (pool_norm_ref.avg_fwd / avg_undo).

Response norm.  Per element, in units of 2^-24 * s_j (pool_norm_ref.rnorm_fwd / rnorm_undo).  The bound cannot be derived — the kernels
slide their window sums, subtracting what leaves as the reference does, and replace powf by exp2(-b * log2(u)) — so it is measured
against the REFERENCE, not the kernels: E_case = the fp32 oracle's own largest error on the same arrays, allowed = 4 * E_case + 34
(4: the kernels walk differently, but each lane or segment restarts its sum, so no walk is longer than the oracle's; 34: twice the 17
units of the "relative error ~1e-6" the kernel file states for its exp2 / log2 pair)."""
import ctypes

import numpy as np
import pytest

import oracle
import pool_norm_ref as P

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    from convnet_amd._lib import lib
    return lib


class Dev:
    """`a` ((C, H, W, N) numpy: the column-major bytes of the (N, W*H*C) matrix) on the device between guard floats of 7.0"""

    def __init__(self, a, mis=False):
        from hip_adapter import _mat
        a = np.asarray(a, np.float32)
        C, H, W, N = a.shape
        self.g = 1 if mis else 4
        self.m, self.full = _mat(a.reshape(-1), 1, a.size, guard=(self.g, self.g))
        self.m.Reshape(N, W * H * C)
        self.m.SetShape4D(N, W, H, C)
        assert self.m.mat_.data_device % 16 == (4 if mis else 0)
        self.shape = a.shape

    @property
    def mat(self):
        return self.m.GetMat()

    @property
    def s4(self):
        return ctypes.byref(self.m.shape_)

    def get(self):
        """the tensor's bytes, after checking the guards"""
        x = self.full.ToNumpy().reshape(-1)
        assert np.all(x[:self.g] == 7.0) and np.all(x[-self.g:] == 7.0), "guard floats overwritten"
        return x[self.g:-self.g].reshape(self.shape)


def same(got, want, *what):
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError((*what, "differing", bad.size, "of", got.size, "first", bad[:4].tolist(), got.reshape(-1)[bad[:4]].tolist(),
                              want.reshape(-1)[bad[:4]].tolist()))


def within(got, exact, bound, *what):
    err = np.abs(got.astype(np.float64) - exact)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(*what, f"worst error / bound {worst:.3f}")
    assert np.all(err <= bound), (*what, worst, int((err > bound).sum()))


def _desc(g):
    from hip_adapter import _desc
    return _desc(g, pool=True)


def _pool_id(case):
    name, mis = case
    p = P.pool_paths(name, mis)
    return f"{name}-{'misaligned' if mis else 'aligned'}-{p['max_fwd']}|{p['max_undo']}".replace(" ", "")


def _ran(path):
    """the library reports the kernel and the grid that pool_norm_ref.expected_path names for the call just made"""
    from hip_adapter import last_kernel
    P.launched(path, *last_kernel())


def _fwd(lib, kind, g, X, T, st, so):
    (lib.MaxPoolGemm if kind == "max" else lib.AvgPoolGemm)(X.mat, T.mat, X.s4, T.s4, _desc(g), st, so)
    _ran(P.expected_path(f"{kind}_fwd", g, X.g == 4))


def _max_undo(lib, g, X, DY, Y, T, st, relu):
    (lib.MaxPoolUndoRelu if relu else lib.MaxPoolUndoGemm)(X.mat, DY.mat, Y.mat, T.mat, X.s4, DY.s4, _desc(g), st)
    _ran(P.expected_path("max_undo", g, X.g == 4))


def _avg_undo(lib, g, DY, T, st):
    lib.AvgPoolUndoGemm(DY.mat, T.mat, DY.s4, T.s4, _desc(g), st)
    _ran(P.expected_path("avg_undo", g, DY.g == 4))


# ======== pooling ===========================================================================================================================
@pytest.mark.parametrize("case", P.POOL_CASES, ids=_pool_id)
def test_max_pool_forward_is_exact_on_negative_data(lib, case):
    """scales (0, 1): integer data with negative maxima, and the all -5 tensor — a maximum that starts from 0, or a padded tap that takes
    part as 0, gives 0 where -5 is due"""
    name, mis = case
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    for key in ("xi", "x5"):
        X, T = Dev(d[key], mis), Dev(np.full(P.shape_out(g), 3.25), mis)
        _fwd(lib, "max", g, X, T, 0.0, 1.0)
        same(T.get(), P.max_fwd(g, d[key]), name, key)
        same(X.get(), d[key], "input")
        if key == "x5":
            assert np.all(T.get() == -5.0)


@pytest.mark.parametrize("case", P.POOL_CASES, ids=_pool_id)
def test_max_pool_forward_scales_are_exact(lib, case):
    """targets = scaleTargets * targets + scaleOutput * max with an integer target: every arm of the kernels' epilogues"""
    name, mis = case
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    X = Dev(d["xi"], mis)
    for st, so in P.SCALES[1:]:
        T = Dev(d["ti_out"], mis)
        _fwd(lib, "max", g, X, T, st, so)
        same(T.get(), P.max_fwd(g, d["xi"], d["ti_out"], st, so), name, st, so)
    same(X.get(), d["xi"], "input")


@pytest.mark.parametrize("case", P.POOL_CASES, ids=_pool_id)
def test_max_pool_undo_routes_every_tie_exactly(lib, case):
    name, mis = case
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    X, DY, Y = Dev(d["xi"], mis), Dev(d["dyi"], mis), Dev(d["yi"], mis)
    for st in P.UNDO_SCALES:
        T = Dev(d["ti_in"], mis)
        _max_undo(lib, g, X, DY, Y, T, st, False)
        same(T.get(), P.max_undo(g, d["xi"], d["dyi"], d["yi"], d["ti_in"], st), name, "undo", st)
    same(X.get(), d["xi"], "images"), same(DY.get(), d["dyi"], "maxGrads"), same(Y.get(), d["yi"], "maxActs")


@pytest.mark.parametrize("case", P.POOL_CASES, ids=_pool_id)
def test_max_pool_undo_relu_masks_the_accumulated_target(lib, case):
    """MaxPoolUndoRelu = (x > 0) ? scaleTargets * targets + undo : 0 — strictly greater: the integer data hold many x == 0"""
    name, mis = case
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    X, DY, Y = Dev(d["xi"], mis), Dev(d["dyi"], mis), Dev(d["yi"], mis)
    assert (d["xi"] == 0).any()
    for st in P.UNDO_SCALES:
        T = Dev(d["ti_in"], mis)
        _max_undo(lib, g, X, DY, Y, T, st, True)
        got = T.get()
        same(got, P.max_undo(g, d["xi"], d["dyi"], d["yi"], d["ti_in"], st, True), name, "undo relu", st)
        assert np.all(got[d["xi"] <= 0] == 0)
    same(X.get(), d["xi"], "images"), same(DY.get(), d["dyi"], "maxGrads"), same(Y.get(), d["yi"], "maxActs")


@pytest.mark.parametrize("case", P.POOL_CASES, ids=_pool_id)
def test_avg_pool_forward_within_the_counted_bound(lib, case):
    name, mis = case
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    for key in ("xn", "xw"):
        X = Dev(d[key], mis)
        for st, so in P.SCALES:
            T = Dev(d["tn_out"], mis)
            _fwd(lib, "avg", g, X, T, st, so)
            within(T.get(), *P.avg_fwd(g, d[key], d["tn_out"], st, so), name, key, st, so)
        same(X.get(), d[key], "input")


@pytest.mark.parametrize("case", P.POOL_CASES, ids=_pool_id)
def test_avg_pool_undo_within_the_counted_bound(lib, case):
    name, mis = case
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    for key in ("dyn", "dyw"):
        DY = Dev(d[key], mis)
        for st in P.UNDO_SCALES:
            T = Dev(d["tn_in"], mis)
            _avg_undo(lib, g, DY, T, st)
            exact, bound, covered = P.avg_undo(g, d[key], d["tn_in"], st)
            got = T.get()
            within(got, exact, bound, name, key, st)
            same(got[~covered], (f32(st) * d["tn_in"])[~covered], "a pixel no window covers is exactly st * t0")
        same(DY.get(), d[key], "avgGrads")


@pytest.mark.parametrize("name", P.FIXED_CASES, ids=lambda n: f"{n}-{P.pool_paths(n, False)['avg_undo']}".replace(" ", ""))
def test_fixed_window_kernels_are_bit_identical_to_the_generic_ones(lib, name):
    """the kernel file's claim ("same visiting order as the generic kernels, so the fp32 sums are bit-identical to them"): the same data
    aligned (fixed-window or 2 x 2-block kernel) and misaligned (generic kernel, scalar arm)"""
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    assert "fixed" in P.pool_paths(name, False)["avg_fwd"] and P.pool_paths(name, True)["avg_fwd"] == "pool_fwd_kernel<avg>/scalar"
    out = {}
    for mis in (False, True):
        X, DY, Y = Dev(d["xn"], mis), Dev(d["dyn"], mis), Dev(d["yn"], mis)
        T1, T2, T3, T4 = Dev(d["tn_out"], mis), Dev(d["tn_in"], mis), Dev(d["tn_in"], mis), Dev(d["tn_in"], mis)
        _fwd(lib, "avg", g, X, T1, 0.5, -2.0)
        _avg_undo(lib, g, DY, T2, 1.0)
        _max_undo(lib, g, X, DY, Y, T3, 1.0, False)
        _max_undo(lib, g, X, DY, Y, T4, 0.0, True)
        out[mis] = [t.get() for t in (T1, T2, T3, T4)]
        same(X.get(), d["xn"], "images"), same(DY.get(), d["dyn"], "grads"), same(Y.get(), d["yn"], "maxActs")
    for what, a, b in zip(("avg forward", "avg undo", "max undo", "max undo relu"), out[False], out[True]):
        same(a, b, name, what)
    # ... and the max undo on N(0, 1) data is right, not merely the same twice (sums of at most four routed terms plus the target)
    exact = P.max_undo(g, d["xn"], d["dyn"], d["yn"], d["tn_in"], 1.0)
    mag = P.max_undo(g, d["xn"], np.abs(d["dyn"]), d["yn"], np.abs(d["tn_in"]), 1.0)
    within(out[False][2], exact, (P.box_sizes(g)[1].max() + 1) * P.U * mag, name, "max undo N(0,1)")


@pytest.mark.parametrize("case", [c for c in P.POOL_CASES if c[0] in ("k3s1_6x7_p1p2_N4", "k3s1_6x7_p1p2_N6", "f32_11x11_p1_C13", "f22_7x7_p1",
                                                                      "blk_43x41_C7")], ids=_pool_id)
def test_pooling_is_bit_identical_from_run_to_run(lib, case):
    name, mis = case
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    runs = []
    for _ in range(2):
        X, DY, Y = Dev(d["xn"], mis), Dev(d["dyn"], mis), Dev(d["yn"], mis)
        TM, TA, UM, UA = Dev(d["tn_out"], mis), Dev(d["tn_out"], mis), Dev(d["tn_in"], mis), Dev(d["tn_in"], mis)
        _fwd(lib, "max", g, X, TM, 1.0, 1.0)
        _fwd(lib, "avg", g, X, TA, 1.0, 1.0)
        _max_undo(lib, g, X, DY, Y, UM, 1.0, False)
        _avg_undo(lib, g, DY, UA, 1.0)
        runs.append([t.get() for t in (TM, TA, UM, UA)])
        same(X.get(), d["xn"], "images"), same(DY.get(), d["dyn"], "grads"), same(Y.get(), d["yn"], "maxActs")
    for a, b in zip(*runs):
        same(a, b, name)


# ======== response norm =====================================================================================================================
def _rn_id(name):
    p = P.rnorm_paths(name)
    return f"{name}-{p['rnorm_fwd']}|{p['rnorm_undo']}".replace(" ", "")


def _rn(lib, X, T, C, size_f, a, b, blocked, relu=False):
    (lib.ResponseNormCrossMapRelu if relu else lib.ResponseNormCrossMapGemm)(X.mat, T.mat, C, size_f, a, b, blocked)
    _ran(P.expected_path("rnorm_fwd", C=C, size_f=size_f, blocked=blocked, locs=int(np.prod(X.shape[1:])), aligned=X.g == 4))


def _rn_undo(lib, DY, X, T, C, size_f, a, b, blocked):
    lib.ResponseNormCrossMapUndoGemm(DY.mat, X.mat, T.mat, C, size_f, a, b, blocked)
    _ran(P.expected_path("rnorm_undo", C=C, size_f=size_f, blocked=blocked, locs=int(np.prod(X.shape[1:])), aligned=X.g == 4))


@pytest.mark.parametrize("ab", P.PARAMS, ids=lambda ab: f"a{ab[0]}b{ab[1]}")
@pytest.mark.parametrize("name", list(P.RNORM_CASES), ids=_rn_id)
def test_response_norm_forward(lib, name, ab):
    size_f, blocked, shape, mis = P.RNORM_CASES[name]
    (a, b), d, C = ab, P.rnorm_data(name), shape[0]
    for key in ("xn", "xw"):
        x = d[key]
        X = Dev(x, mis)
        T, T2, TR = (Dev(np.full(shape, 3.25), mis) for _ in range(3))
        _rn(lib, X, T, C, size_f, a, b, blocked)
        _rn(lib, X, T2, C, size_f, a, b, blocked)
        _rn(lib, X, TR, C, size_f, a, b, blocked, relu=True)
        got = T.get()
        same(X.get(), x, "images")
        same(T2.get(), got, name, "run to run")
        same(TR.get(), np.maximum(got, 0), name, "ResponseNormCrossMapRelu == max(plain, 0)")
        assert np.all(got[x == 0] == 0), "x_j == 0 must give exactly 0"
        exact, s = P.rnorm_fwd(x, size_f, a, b, blocked)
        e_case = P.units(oracle.port.rnorm(x, size_f, a, b, blocked), exact, s)
        e_gpu = P.units(got, exact, s)
        print(f"UNITS forward {name} ({a}, {b}) {key}: E_case {e_case:.1f} allowed {P.rnorm_allowed(e_case):.1f} gpu {e_gpu:.1f}")
        assert e_gpu <= P.rnorm_allowed(e_case), (name, key, e_gpu, e_case)


@pytest.mark.parametrize("ab", P.PARAMS, ids=lambda ab: f"a{ab[0]}b{ab[1]}")
@pytest.mark.parametrize("name", list(P.RNORM_CASES), ids=_rn_id)
def test_response_norm_undo(lib, name, ab):
    size_f, blocked, shape, mis = P.RNORM_CASES[name]
    (a, b), d, C = ab, P.rnorm_data(name), shape[0]
    for k in ("n", "w"):
        x, dy = d["x" + k], d["dy" + k]
        X, DY = Dev(x, mis), Dev(dy, mis)
        T, T2 = (Dev(np.full(shape, 3.25), mis) for _ in range(2))
        _rn_undo(lib, DY, X, T, C, size_f, a, b, blocked)
        _rn_undo(lib, DY, X, T2, C, size_f, a, b, blocked)
        got = T.get()
        same(X.get(), x, "inputs"), same(DY.get(), dy, "outGrads")
        same(T2.get(), got, name, "run to run")
        exact, s = P.rnorm_undo(dy, x, size_f, a, b, blocked)
        e_case = P.units(oracle.port.rnorm_undo(dy, x, size_f, a, b, blocked), exact, s)
        e_gpu = P.units(got, exact, s)
        print(f"UNITS undo {name} ({a}, {b}) {k}: E_case {e_case:.1f} allowed {P.rnorm_allowed(e_case):.1f} gpu {e_gpu:.1f}")
        assert e_gpu <= P.rnorm_allowed(e_case), (name, k, e_gpu, e_case)


@pytest.mark.parametrize("name", list(P.RNORM_CASES), ids=_rn_id)
def test_response_norm_in_place_equals_out_of_place(lib, name):
    """targets == images (forward) and targets == outGrads (undo).  The LDS-tiled and the fast kernels stage a tile's every channel before
    they write it, and the two-pass undo has read outGrads completely (pass 1) before pass 2 writes: bit-identical to out of place.
    rnorm_fwd_kernel (C > 768) subtracts channels it has already overwritten and reads other segments' channels while they are
    written: include/convnet_hip.h forbids targets == images there, and it is not called."""
    size_f, blocked, shape, mis = P.RNORM_CASES[name]
    (a, b), d, C = P.PARAMS[0], P.rnorm_data(name), shape[0]
    x, dy = d["xn"], d["dyn"]
    if not P.rnorm_paths(name)["rnorm_fwd"].startswith("rnorm_fwd_kernel"):
        X, T, XI = Dev(x, mis), Dev(np.full(shape, 3.25), mis), Dev(x, mis)
        _rn(lib, X, T, C, size_f, a, b, blocked)
        _rn(lib, XI, XI, C, size_f, a, b, blocked)
        same(XI.get(), T.get(), name, "forward in place")
        same(X.get(), x, "images")
    X, DY, T, DI = Dev(x, mis), Dev(dy, mis), Dev(np.full(shape, 3.25), mis), Dev(dy, mis)
    _rn_undo(lib, DY, X, T, C, size_f, a, b, blocked)
    _rn_undo(lib, DI, X, DI, C, size_f, a, b, blocked)
    same(DI.get(), T.get(), name, "undo in place")
    same(X.get(), x, "inputs"), same(DY.get(), dy, "outGrads")
