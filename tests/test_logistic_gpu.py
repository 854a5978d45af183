"""GPU: the logistic and softmax-distribution entries of include/convnet_hip.h — apply_sigmoid, apply_logistic_deriv, apply_logistic_grad,
get_logistic_correct_normalized, compute_cross_entropy and the fused logistic_dropout, logistic_deriv_scaled, logistic_ce_grad_correct,
softmax_dist_ce_grad — against the numpy restatements of tests/logistic_ref.py (pinned by tests/test_logistic_ref_cpu.py).

No GEMM is involved, so the matrix path plays no part.  Shapes: one element, odd sizes, one column, more than one 32-row block, the
(256, 1000) output layer, and a length above one grid pass (2048 blocks x 256 threads x 4 floats) whose tail is no multiple of 4.  Every
tensor sits between guard columns of 7.0; the view case is a get_slice of a 67-row matrix from column 1, which starts 4-byte aligned only.
Tolerances: probabilities and cross entropies within P_TOL of float64 (the softmax family's tolerance, tests/test_elementwise_gpu.py);
derivatives, gradients and correct shares bit-identical to the fp32 restatement; every fused entry bit-identical to its unfused call
sequence in the same process; the accumulators within the whole-matrix reductions' bound of a float64 sum."""
import ctypes

import numpy as np
import pytest

import logistic_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
P_TOL = dict(rtol=1e-5, atol=1e-12)
SUM_BOUND = 1e-5                       # |got - exact| / sum of |terms|: the bound of test_whole_matrix_reductions
BIG = 2 * (1 << 20) + 7                # one grid pass is 2048 * 256 * 4 = 2^21 floats (blocks_for / kMaxBlocks, csrc/elementwise.hip)
SHAPES = [(1, 1), (3, 5), (64, 1), (67, 33), (256, 1000), (1, BIG)]
SHAPE_IDS = [f"{r}x{c}" for r, c in SHAPES]
ROW_SHAPES = SHAPES[:-1] + [(BIG // 64 + 1, 3)]     # the per-row entries: many 32-row blocks instead of one endless row
ROW_IDS = [f"{r}x{c}" for r, c in ROW_SHAPES]
ERR_DIMS, ERR_TRANSPOSEDNESS = -1, -7
MARK = 3.25
TINY = 1e-10


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


@pytest.fixture(scope="module")
def lib(M):
    from convnet_amd._lib import lib
    return lib


class Dev:
    """`a` (numpy (cols, rows)) as a (rows, cols) device matrix: a get_slice view between one guard column of 7.0 on either side."""

    def __init__(self, a, rows, cols):
        from hip_adapter import _mat
        a = np.asarray(a, np.float32).reshape(cols, rows)
        self.m, self.full = _mat(a.reshape(-1), rows, cols, guard=(1, 1))
        self.rows, self.shape = rows, a.shape

    @property
    def mat(self):
        return self.m.GetMat()

    def get(self):
        x = self.full.ToNumpy().reshape(-1)
        assert np.all(x[:self.rows] == 7.0) and np.all(x[-self.rows:] == 7.0), "guard floats overwritten"
        return x[self.rows:-self.rows].reshape(self.shape).copy()


def same_bits(got, want, *what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    g, w = got.reshape(-1), want.reshape(-1)
    bad = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w)))      # (a NaN equals a NaN)
    if bad.size:
        raise AssertionError((*what, "differing", bad.size, "of", got.size, "first", bad[:4].tolist(), got.reshape(-1)[bad[:4]].tolist(),
                              want.reshape(-1)[bad[:4]].tolist()))


def close(got, want, *what):
    ok = np.isclose(got.astype(np.float64), want, equal_nan=True, **P_TOL)
    assert np.all(ok), (*what, int((~ok).sum()), got[~ok][:4].tolist(), np.asarray(want)[~ok][:4].tolist())


def x_normal(rows, cols, seed=0):
    return np.random.default_rng([11, rows, cols, seed]).standard_normal((cols, rows)).astype(np.float32)


def x_grid(rows, cols, nan=True):
    """[-100, 100] in equal steps with +-88, +-89, +-0 placed first and (nan) one NaN, filling the matrix in a scrambled order"""
    n = rows * cols
    special = np.array([88.0, -88.0, 89.0, -89.0, 0.0, -0.0, 100.0, -100.0] + ([np.nan] if nan else []), np.float32)
    x = np.linspace(-100.0, 100.0, n, dtype=np.float64).astype(np.float32)
    k = min(n, special.size)
    x[np.random.default_rng([13, n]).permutation(n)[:k]] = special[:k] if n >= special.size else special[-k:]
    return x.reshape(cols, rows)


def targets(rows, cols, seed=0):
    return np.random.default_rng([17, rows, cols, seed]).choice(np.array([-1.0, 0.0, 0.5, 1.0], np.float32), size=(cols, rows))


def probs01(rows, cols, seed=0):
    """fp32 values in [0, 1] with exact 0, 0.5 and 1 among them"""
    p = np.random.default_rng([19, rows, cols, seed]).random((cols, rows), dtype=np.float32)
    flat = p.reshape(-1)
    flat[::7] = 0.5
    flat[3::11] = 1.0
    flat[5::13] = 0.0
    return p


def accum(value=0.0):
    from hip_adapter import _mat
    return _mat(np.array([value], np.float32), 1, 1)


INPUTS = {"normal": x_normal, "grid": x_grid}


# ======== the five cudamat entries =====================================================================================================
@pytest.mark.parametrize("kind", list(INPUTS))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_apply_sigmoid(lib, shape, kind):
    rows, cols = shape
    x = INPUTS[kind](rows, cols)
    want = R.sigmoid_f64(x)
    for in_place in (False, True):
        X = Dev(x, rows, cols)
        T = X if in_place else Dev(np.full(x.shape, MARK), rows, cols)
        assert lib.apply_sigmoid(X.mat, T.mat) == 0
        got = T.get()
        close(got, want, "apply_sigmoid", shape, kind, in_place)
        assert np.array_equal(np.isnan(got), np.isnan(x)), "NaN in gives NaN out, and overflow gives none"
        assert np.all(got[x >= 89] == 1.0) and np.all(got[x <= -89] == 0.0)
        assert np.all((got[x == 0] == 0.5))
        ok = ~np.isnan(x)
        assert np.all((got[ok] >= 0) & (got[ok] <= 1))
        if not in_place:
            same_bits(X.get(), x, "operand untouched")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_logistic_deriv_and_grad_equal_the_float32_restatement(lib, shape):
    rows, cols = shape
    d, y, t = x_normal(rows, cols, 1), probs01(rows, cols), targets(rows, cols)
    for in_place in (False, True):
        D, Y = Dev(d, rows, cols), Dev(y, rows, cols)
        T = D if in_place else Dev(np.full(d.shape, MARK), rows, cols)
        assert lib.apply_logistic_deriv(D.mat, Y.mat, T.mat) == 0
        same_bits(T.get(), R.logistic_deriv(d, y), "apply_logistic_deriv", shape, in_place)
        same_bits(Y.get(), y, "state untouched")
        Y, G = Dev(y, rows, cols), Dev(t, rows, cols)
        T = Y if in_place else Dev(np.full(d.shape, MARK), rows, cols)
        assert lib.apply_logistic_grad(Y.mat, G.mat, T.mat) == 0
        same_bits(T.get(), R.logistic_grad(y, t), "apply_logistic_grad", shape, in_place)
        same_bits(G.get(), t, "targets untouched")
        # the fused in-place derivative: the restatement, and the two calls it replaces
        for scale in (1.0, 1.0 / (1 - 0.3)):
            D, Y = Dev(d, rows, cols), Dev(y, rows, cols)
            assert lib.logistic_deriv_scaled(D.mat, Y.mat, scale) == 0
            same_bits(D.get(), R.logistic_deriv(d, y, scale), "logistic_deriv_scaled", shape, scale)
            U = Dev(d, rows, cols)
            assert lib.mult_by_scalar(U.mat, scale, U.mat, 0.0) == 0 and lib.apply_logistic_deriv(U.mat, Y.mat, U.mat) == 0
            same_bits(D.get(), U.get(), "logistic_deriv_scaled vs mult_by_scalar + apply_logistic_deriv", shape, scale)


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ROW_IDS)
def test_logistic_correct_normalized_equals_the_restatement(lib, shape):
    rows, cols = shape
    p, t = probs01(rows, cols, 2), targets(rows, cols, 2)
    if rows > 2:
        t[:, 1] = -1.0               # a row with no counted entry
        t[:, 2] = 0.5                # a row of t = 0.5 against p on both sides of 0.5
    P, T, O = Dev(p, rows, cols), Dev(t, rows, cols), Dev(np.full(rows, MARK), rows, 1)
    assert lib.get_logistic_correct_normalized(P.mat, T.mat, O.mat) == 0
    want = R.logistic_correct_normalized(p, t)
    same_bits(O.get().reshape(-1), want, "get_logistic_correct_normalized", shape)
    if rows > 2:
        assert want[1] == 0
    same_bits(P.get(), p), same_bits(T.get(), t)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_compute_cross_entropy(lib, shape):
    rows, cols = shape
    t = np.abs(x_normal(rows, cols, 3))
    t.reshape(-1)[::3] = 0
    p = probs01(rows, cols, 3)
    want = R.cross_entropy_f64(t, p, TINY)
    for in_place in (False, True):
        Tm, P = Dev(t, rows, cols), Dev(p, rows, cols)
        O = Tm if in_place else Dev(np.full(t.shape, MARK), rows, cols)
        assert lib.compute_cross_entropy(Tm.mat, P.mat, O.mat, TINY) == 0
        got = O.get()
        close(got, want, "compute_cross_entropy", shape, in_place)
        assert np.all(np.isfinite(got)) and np.all(got[t == 0] == 0)
        same_bits(P.get(), p, "probabilities untouched")


def test_operands_that_disagree_in_alignment(lib):
    """(67, 33) operands at byte offsets 12 (the view), 4 and 0 within 16: no common head, so the entries run scalar."""
    from hip_adapter import _mat
    rows, cols = 67, 33
    d, y = x_normal(rows, cols, 8), probs01(rows, cols, 8)
    D = Dev(d, rows, cols)
    ym, yfull = _mat(y.reshape(-1), 1, rows * cols, guard=(1, 1))
    ym.Reshape(rows, cols)
    T = _mat(np.full(rows * cols, MARK, np.float32), rows, cols)
    offsets = [m.mat_.data_device % 16 for m in (D.m, ym, T)]
    assert offsets == [12, 4, 0], offsets
    assert lib.apply_logistic_deriv(D.mat, ym.GetMat(), T.GetMat()) == 0
    same_bits(T.ToNumpy(), R.logistic_deriv(d, y), "apply_logistic_deriv, mixed alignment")
    assert lib.apply_sigmoid(D.mat, T.GetMat()) == 0
    close(T.ToNumpy(), R.sigmoid_f64(d), "apply_sigmoid, mixed alignment")
    same_bits(D.get(), d), same_bits(yfull.ToNumpy().reshape(-1)[1:-1], y.reshape(-1))


def test_entries_refuse_mismatched_and_transposed_operands(M, lib):
    a, b, o = Dev(np.zeros((5, 3)), 3, 5), Dev(np.zeros((3, 5)), 5, 3), Dev(np.full(3, MARK), 3, 1)
    acc = accum()
    same_sized = Dev(np.zeros((5, 3)), 3, 5)
    calls = {
        "apply_sigmoid": lambda X, Y: lib.apply_sigmoid(X, Y),
        "apply_logistic_deriv": lambda X, Y: lib.apply_logistic_deriv(X, Y, X),
        "apply_logistic_grad": lambda X, Y: lib.apply_logistic_grad(X, Y, X),
        "get_logistic_correct_normalized": lambda X, Y: lib.get_logistic_correct_normalized(X, Y, o.mat),
        "compute_cross_entropy": lambda X, Y: lib.compute_cross_entropy(X, Y, X, TINY),
        "logistic_deriv_scaled": lambda X, Y: lib.logistic_deriv_scaled(X, Y, 2.0),
        "logistic_ce_grad_correct": lambda X, Y: lib.logistic_ce_grad_correct(X, Y, X, same_sized.mat, acc.GetMat(), 1.0),
        "softmax_dist_ce_grad": lambda X, Y: lib.softmax_dist_ce_grad(X, Y, X, same_sized.mat, acc.GetMat(), 1.0, TINY),
    }
    for name, call in calls.items():
        assert call(a.mat, b.mat) == ERR_DIMS, name                       # (3, 5) against (5, 3): same element count, other shape
        assert call(a.mat, same_sized.m.GetMatTranspose()) == ERR_TRANSPOSEDNESS, name
    assert lib.get_logistic_correct_normalized(a.mat, same_sized.mat, Dev(np.zeros(5), 5, 1).mat) == ERR_DIMS
    assert lib.logistic_ce_grad_correct(a.mat, same_sized.mat, a.mat, same_sized.mat, o.mat, 1.0) == ERR_DIMS   # the accumulator is 1x1
    assert np.all(a.get() == 0) and np.all(b.get() == 0) and np.all(o.get() == MARK) and acc.ToNumpy()[0, 0] == 0


# ======== the fused entries ============================================================================================================
@pytest.fixture()
def rnd(lib):
    """a generator state of the test's own: the stream Matrix._rnd hands later tests stays where it is"""
    from convnet_amd import _lib

    def make(seed):
        st = _lib.rnd_struct()
        assert lib.init_random(ctypes.byref(st), seed) == 0
        return st
    return make


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_logistic_dropout_equals_sigmoid_then_dropout(lib, rnd, shape):
    rows, cols = shape
    x = x_normal(rows, cols, 4)
    p, scale = 0.4, 1.0 / (1 - 0.4)
    fused_st, plain_st = rnd(77), rnd(77)
    for call in range(2):                          # the second call draws the next mask in both streams
        F, U = Dev(x, rows, cols), Dev(x, rows, cols)
        assert lib.logistic_dropout(ctypes.byref(fused_st), F.mat, p, scale) == 0
        assert lib.apply_sigmoid(U.mat, U.mat) == 0
        s = U.get()
        assert lib.dropout(ctypes.byref(plain_st), U.mat, p, 0.0, scale) == 0
        f, u = F.get(), U.get()
        assert np.array_equal(R.dropout_mask(f, s), R.dropout_mask(u, s)), ("masks differ", shape, call)
        same_bits(f, u, "logistic_dropout vs apply_sigmoid + dropout", shape, call)
        if call == 0:
            first = R.dropout_mask(f, s)
        kept = ~R.dropout_mask(f, s)
        same_bits(f[kept], (s * f32(scale))[kept], "kept units are sigmoid * scale")
    if rows * cols >= 1000:
        n = rows * cols
        assert abs(first.mean() - p) < 6 * np.sqrt(p * (1 - p) / n)
        assert not np.array_equal(first, R.dropout_mask(f, s)), "the second call repeated the first mask"


@pytest.mark.parametrize("kind", list(INPUTS))
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ROW_IDS)
def test_logistic_ce_grad_correct(lib, shape, kind):
    rows, cols = shape
    x, t = INPUTS[kind](rows, cols), targets(rows, cols, 5)
    if rows > 2:
        t[:, 1] = -1.0
    deriv_scale = 0.5
    # the sequence it replaces
    S, T, G, O = Dev(x, rows, cols), Dev(t, rows, cols), Dev(np.full(x.shape, MARK), rows, cols), Dev(np.full(rows, MARK), rows, 1)
    assert lib.apply_sigmoid(S.mat, S.mat) == 0 and lib.apply_logistic_grad(S.mat, T.mat, G.mat) == 0
    assert lib.mult_by_scalar(G.mat, deriv_scale, G.mat, 0.0) == 0 and lib.get_logistic_correct_normalized(S.mat, T.mat, O.mat) == 0
    probs, deriv, share = S.get(), G.get(), O.get().reshape(-1)
    same_bits(share, R.logistic_correct_normalized(probs, t), "the unfused share on the device's probabilities")
    exact, terms = float(share.astype(np.float64).sum()), float(np.abs(share.astype(np.float64)).sum())
    for alias in (False, True):
        X, T, D, acc = Dev(x, rows, cols), Dev(t, rows, cols), Dev(np.full(x.shape, MARK), rows, cols), accum()
        P = X if alias else Dev(np.full(x.shape, MARK), rows, cols)
        assert lib.logistic_ce_grad_correct(X.mat, T.mat, P.mat, D.mat, acc.GetMat(), deriv_scale) == 0
        got_p = P.get()
        close(got_p, R.sigmoid_f64(x), "probs", shape, kind, alias)
        same_bits(got_p, probs, "probs vs apply_sigmoid", shape, kind, alias)
        same_bits(D.get(), deriv, "deriv vs apply_logistic_grad + mult_by_scalar", shape, kind, alias)
        same_bits(T.get(), t, "targets untouched")
        if not alias:
            same_bits(X.get(), x, "logits untouched")
        one = float(acc.ToNumpy()[0, 0])
        print(shape, kind, "correct share sum", one, "float64", exact)
        assert abs(one - exact) <= SUM_BOUND * max(terms, 1e-30), (one, exact)
        # a second call adds, and gives the same bits as the first (no atomics)
        X2 = Dev(x, rows, cols)
        assert lib.logistic_ce_grad_correct(X2.mat, T.mat, X2.mat, D.mat, acc.GetMat(), deriv_scale) == 0
        two = float(acc.ToNumpy()[0, 0])
        assert abs(two - 2 * exact) <= SUM_BOUND * max(2 * terms, 1e-30), (two, 2 * exact)
        assert f32(two) == f32(one) + f32(one)


@pytest.mark.parametrize("kind", list(INPUTS))
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ROW_IDS)
def test_softmax_dist_ce_grad(lib, shape, kind):
    rows, cols = shape
    x = x_normal(rows, cols, 6) * f32(3) if kind == "normal" else x_grid(rows, cols, nan=False)
    t = np.abs(x_normal(rows, cols, 7))
    t.reshape(-1)[::3] = 0
    t = (t / np.maximum(t.sum(axis=0, keepdims=True), f32(1e-30))).astype(np.float32)      # one distribution per row
    deriv_scale = 0.5
    # the sequence it replaces
    S, T, G, C = (Dev(x, rows, cols), Dev(t, rows, cols), Dev(np.full(x.shape, MARK), rows, cols), Dev(np.full(x.shape, MARK), rows, cols))
    assert lib.softmax_row_major(S.mat, S.mat) == 0 and lib.subtract_elementwise(S.mat, T.mat, G.mat) == 0
    assert lib.mult_by_scalar(G.mat, deriv_scale, G.mat, 0.0) == 0 and lib.compute_cross_entropy(T.mat, S.mat, C.mat, TINY) == 0
    probs, deriv = S.get(), G.get()
    close(C.get(), R.cross_entropy_f64(t, probs, TINY), "the unfused cross entropy on the device's probabilities")
    ce64 = R.cross_entropy_f64(t, probs, TINY)
    exact, terms = float(ce64.sum()), float(np.abs(ce64).sum())
    for alias in (False, True):
        X, T, D, acc = Dev(x, rows, cols), Dev(t, rows, cols), Dev(np.full(x.shape, MARK), rows, cols), accum()
        P = X if alias else Dev(np.full(x.shape, MARK), rows, cols)
        assert lib.softmax_dist_ce_grad(X.mat, T.mat, P.mat, D.mat, acc.GetMat(), deriv_scale, TINY) == 0
        got_p = P.get()
        close(got_p, R.softmax_rows_f64(x), "probs", shape, kind, alias)
        same_bits(got_p, probs, "probs vs softmax_row_major", shape, kind, alias)
        same_bits(D.get(), deriv, "deriv vs subtract_elementwise + mult_by_scalar", shape, kind, alias)
        same_bits(T.get(), t, "targets untouched")
        one = float(acc.ToNumpy()[0, 0])
        print(shape, kind, "cross entropy sum", one, "float64", exact)
        assert abs(one - exact) <= SUM_BOUND * max(terms, 1e-30), (one, exact)
        X2 = Dev(x, rows, cols)
        assert lib.softmax_dist_ce_grad(X2.mat, T.mat, X2.mat, D.mat, acc.GetMat(), deriv_scale, TINY) == 0
        two = float(acc.ToNumpy()[0, 0])
        assert abs(two - 2 * exact) <= SUM_BOUND * max(2 * terms, 1e-30), (two, 2 * exact)
        assert f32(two) == f32(one) + f32(one)
