"""GPU: the element-wise, row/column-vector, reduction, norm-limit, softmax, RNG and copy/view entries of include/convnet_hip.h on every
launch path of csrc/elementwise.hip, csrc/input_staging.hip and the copy/view part of csrc/state.hip.

References are the numpy restatements of tests/elementwise_ref.py (held against the oracle's compiled C by
tests/test_elementwise_ref_cpu.py).  Where the library promises separately rounded fp32 operations the comparison is np.array_equal.
Reductions run on integer-valued (or grid-valued) data, for which that CPU file proves every order of fp32 summation gives the int64
sum — a dropped, repeated or mis-indexed element cannot hide behind a tolerance — and on N(0, 1) data against float64 under the bound
of the existing reductions test.  Every tensor sits between guard floats of 7.0 in one allocation: "aligned" four floats in, "misaligned"
one float in (data_device % 16 == 4), which is how the trainer's slices of its flat buffers arrive."""
import ctypes

import numpy as np
import pytest

import elementwise_ref as R
from golden_cases import rel_err

pytestmark = pytest.mark.gpu
f32 = np.float32
BIG = 2 * (1 << 20) + 5          # more than one grid pass of 2048 blocks x 256 threads x 4 floats
SIZES = [1, 3, 4, 5, 1027, BIG]
PLACES = [False, True]
PLACE_IDS = ["aligned", "misaligned"]
ERR_DIMS, ERR_GENERIC, ERR_UNSUPPORTED = -1, -6, -9


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
    """`a` (numpy (cols, rows): the column-major bytes) as a (rows, cols) device matrix between guard floats of 7.0."""

    def __init__(self, a, rows, cols, mis=False):
        from hip_adapter import _mat
        a = np.asarray(a, np.float32)
        self.g = 1 if mis else 4
        self.m, self.full = _mat(a.reshape(-1), 1, a.size, guard=(self.g, self.g))
        self.m.Reshape(rows, cols)
        assert self.m.mat_.data_device % 16 == (4 if mis else 0)
        self.shape = a.shape

    @property
    def mat(self):
        return self.m.GetMat()

    def get(self):
        """the tensor's bytes, after checking the guards"""
        x = self.full.ToNumpy().reshape(-1)
        assert np.all(x[:self.g] == 7.0) and np.all(x[-self.g:] == 7.0), "guard floats overwritten"
        return x[self.g:-self.g].reshape(self.shape)


def flat(a, mis=False):
    a = np.asarray(a, np.float32)
    return Dev(a.reshape(-1), 1, a.size, mis)


def same(got, want, *what):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != np.asarray(want).reshape(-1))
        raise AssertionError((*what, "differing", bad.size, "of", got.size, "first", bad[:4].tolist(), got.reshape(-1)[bad[:4]].tolist(),
                              np.asarray(want).reshape(-1)[bad[:4]].tolist()))


def within(got, exact, bound, *what):
    err = np.abs(got.astype(np.float64) - exact)
    assert np.all(err <= bound), (*what, float((err - bound).max()), int((err > bound).sum()))


# ======== a. the map2 entries ==============================================================================================================
MARK = 3.25
# name -> (call(lib, X, Y, T), restatement(x, y), in place only)
MAP2 = {
    "add_elementwise": (lambda L, X, Y, T: L.add_elementwise(X, Y, T), R.add_elementwise, False),
    "subtract_elementwise": (lambda L, X, Y, T: L.subtract_elementwise(X, Y, T), R.subtract_elementwise, False),
    "mult_elementwise": (lambda L, X, Y, T: L.mult_elementwise(X, Y, T, 0.0), R.mult_elementwise, False),
    "mult_by_scalar": (lambda L, X, Y, T: L.mult_by_scalar(X, 0.3, T, 0.0), lambda x, y: R.mult_by_scalar(x, 0.3), False),
    "divide_by_scalar": (lambda L, X, Y, T: L.divide_by_scalar(X, 0.3, T), lambda x, y: R.divide_by_scalar(x, 0.3), False),
    "add_scalar": (lambda L, X, Y, T: L.add_scalar(X, 0.3, T), lambda x, y: R.add_scalar(x, 0.3), False),
    "apply_sqrt": (lambda L, X, Y, T: L.apply_sqrt(X, T), lambda x, y: R.apply_sqrt(x), False),
    "lower_bound_scalar": (lambda L, X, Y, T: L.lower_bound_scalar(X, 0.25, T), lambda x, y: R.lower_bound_scalar(x, 0.25), False),
    "upper_bound_mod_scalar": (lambda L, X, Y, T: L.upper_bound_mod_scalar(X, 0.4, T), lambda x, y: R.upper_bound_mod_scalar(x, 0.4), False),
    "apply_rectified_linear_deriv": (lambda L, X, Y, T: L.apply_rectified_linear_deriv(X, Y, T), R.relu_deriv, False),
    "assign_scalar": (lambda L, X, Y, T: L.assign_scalar(X, 0.3), lambda x, y: R.assign_scalar(x, 0.3), True),
    "add_mult": (lambda L, X, Y, T: L.add_mult(X, Y, 0.3), lambda x, y: R.add_mult(x, y, 0.3), True),
}


def _map2_data(n, name):
    rng = np.random.default_rng([5, n])
    x, y = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    y[::5] = 0
    if name == "apply_sqrt":
        x = np.abs(x)
        x[::7] = 0
    return x, y


@pytest.mark.parametrize("mis", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_map2_entries_equal_the_float32_restatement(lib, n, mis):
    for name, (call, ref, in_place_only) in MAP2.items():
        x, y = _map2_data(n, name)
        want = ref(x, y)
        for in_place in (True,) if in_place_only else (True, False):
            X, Y = flat(x, mis), flat(y, mis)
            T = X if in_place else flat(np.full(n, MARK), mis)
            assert call(lib, X.mat, Y.mat, T.mat) == 0, name
            same(T.get(), want, name, n, "in place" if in_place else "out of place")
            same(Y.get(), y, name, "second operand")
            if not in_place:
                same(X.get(), x, name, "first operand")


@pytest.mark.parametrize("mis", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_mult_by_scalar_accumulating_into_the_target(lib, n, mis):
    """target = scale_targets*target + x*alpha may contract to one fma: within two roundings of the exact value; with scale_targets = 0.5
    and alpha = 2 both products are exact and so is every way of forming the sum but one rounding: bit-exact."""
    x, t = _map2_data(n, "mult_by_scalar")
    t = t + f32(1)
    X, T = flat(x, mis), flat(t, mis)
    assert lib.mult_by_scalar(X.mat, 0.3, T.mat, 0.7) == 0
    exact, bound = R.mult_by_scalar_f64(x, 0.3, t, 0.7)
    within(T.get(), exact, bound, "scale 0.7, alpha 0.3")
    same(X.get(), x)
    T = flat(t, mis)
    assert lib.mult_by_scalar(X.mat, 2.0, T.mat, 0.5) == 0
    same(T.get(), f32(0.5) * t + x * f32(2), "scale 0.5, alpha 2")
    X2 = flat(x, mis)                                                   # in place: x = 0.5*x + 2*x
    assert lib.mult_by_scalar(X2.mat, 2.0, X2.mat, 0.5) == 0
    same(X2.get(), f32(0.5) * x + x * f32(2), "in place")


def test_map2_entries_refuse_what_they_cannot_do(lib):
    x = np.arange(12, dtype=np.float32)
    X, Y, S, T = flat(x), flat(x + 1), flat(x[:11]), flat(np.full(12, MARK))
    assert lib.mult_elementwise(X.mat, Y.mat, T.mat, 1.0) == ERR_UNSUPPORTED
    for fn in (lib.add_elementwise, lib.subtract_elementwise):
        assert fn(X.mat, S.mat, T.mat) == ERR_DIMS and fn(X.mat, Y.mat, S.mat) == ERR_DIMS
    assert lib.mult_elementwise(X.mat, S.mat, T.mat, 0.0) == ERR_DIMS
    assert lib.add_mult(X.mat, S.mat, 0.5) == ERR_DIMS
    for fn, args in ((lib.add_scalar, (1.0,)), (lib.divide_by_scalar, (2.0,)), (lib.lower_bound_scalar, (0.0,)), (lib.upper_bound_mod_scalar, (1.0,))):
        assert fn(X.mat, *args, S.mat) == ERR_DIMS
    assert lib.mult_by_scalar(X.mat, 2.0, S.mat, 0.0) == ERR_DIMS and lib.mult_by_scalar(X.mat, 2.0, S.mat, 1.0) == ERR_DIMS
    assert lib.apply_sqrt(X.mat, S.mat) == ERR_DIMS and lib.apply_rectified_linear_deriv(X.mat, S.mat, T.mat) == ERR_DIMS
    same(X.get(), x), same(Y.get(), x + 1), same(S.get(), x[:11]), same(T.get(), np.full(12, MARK, np.float32))      # a refused call changes nothing


# ======== b. row / column vectors ============================================================================================================
def _rowcol_calls(lib, rows, cols, mis, rng):
    """every (name, call, restatement or (exact, bound)) of one shape; the operands as numpy, the call on fresh device tensors"""
    a = rng.standard_normal((cols, rows)).astype(np.float32)
    rowv = (rng.standard_normal(cols) + 3).astype(np.float32)          # one per column; away from 0: also a divisor
    colv = (rng.standard_normal(rows) + 3).astype(np.float32)          # one per row
    out = []
    for mult in (1.0, -1.0, 0.5):
        out.append((f"add_row_mult {mult}", lambda A, V, T, m=mult: lib.add_row_mult(A, V, T, m), "row", R.add_row_mult(a, rowv, mult)))
        out.append((f"add_col_mult {mult}", lambda A, V, T, m=mult: lib.add_col_mult(A, V, T, m), "col", R.add_col_mult(a, colv, mult)))
    out.append(("add_row_mult 0.3", lambda A, V, T: lib.add_row_mult(A, V, T, 0.3), "row", R.vec_f64(a, rowv, 0.3, "row")))
    out.append(("add_col_mult 0.3", lambda A, V, T: lib.add_col_mult(A, V, T, 0.3), "col", R.vec_f64(a, colv, 0.3, "col")))
    out.append(("add_row_vec", lib.add_row_vec, "row", R.add_row_mult(a, rowv)))
    out.append(("add_col_vec", lib.add_col_vec, "col", R.add_col_mult(a, colv)))
    out.append(("div_by_col_vec", lib.div_by_col_vec, "col", R.div_by_col_vec(a, colv)))
    out.append(("mult_by_row_vec", lib.mult_by_row_vec, "row", R.mult_by_row_vec(a, rowv)))
    out.append(("div_by_row_vec", lib.div_by_row_vec, "row", R.div_by_row_vec(a, rowv)))
    return a, rowv, colv, out


@pytest.mark.parametrize("mis", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("rows", [1, 3, 4, 37, 256])
def test_row_and_column_vector_entries(lib, rows, mis):
    rng = np.random.default_rng([6, rows])
    for cols in (1, 5, 33):
        a, rowv, colv, calls = _rowcol_calls(lib, rows, cols, mis, rng)
        for k, (name, call, along, want) in enumerate(calls):
            in_place = k % 2 == 0
            A = Dev(a, rows, cols, mis)
            V = Dev(rowv, 1, cols, mis) if along == "row" else Dev(colv, rows, 1, mis)
            T = A if in_place else Dev(np.full((cols, rows), MARK), rows, cols, mis)
            assert call(A.mat, V.mat, T.mat) == 0, name
            if isinstance(want, tuple):
                within(T.get(), *want, name, rows, cols)
            else:
                same(T.get(), want, name, rows, cols, in_place)
            same(V.get(), rowv if along == "row" else colv, name, "vector")
            if not in_place:
                same(A.get(), a, name, "source")


@pytest.mark.parametrize("mis", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("colours", [1, 3])
def test_add_to_each_pixel(lib, colours, mis):
    rng = np.random.default_rng([7, colours])
    pixels = 7
    for cases in (1, 3, 4, 37, 256):
        a = rng.standard_normal((colours * pixels, cases)).astype(np.float32)
        noise = rng.standard_normal((colours, cases)).astype(np.float32)
        for mult, in_place in ((1.0, True), (-1.0, False), (0.5, True), (0.3, False)):
            A, V = Dev(a, cases, colours * pixels, mis), Dev(noise, cases, colours, mis)
            T = A if in_place else Dev(np.full(a.shape, MARK), cases, colours * pixels, mis)
            assert lib.add_to_each_pixel(A.mat, V.mat, T.mat, mult) == 0
            if mult == 0.3:
                v = np.repeat(np.float64(f32(mult)) * noise.astype(np.float64), pixels, axis=0)
                within(T.get(), a.astype(np.float64) + v, R.EPS * (np.abs(a) + np.abs(v)), cases, mult)
            else:
                same(T.get(), R.add_to_each_pixel(a, noise, mult), cases, mult)
            same(V.get(), noise)


def test_vector_entries_check_the_vector_axis(lib):
    a = np.arange(20, dtype=np.float32).reshape(5, 4)                   # (rows 4, cols 5)
    A, T = Dev(a, 4, 5), Dev(np.full((5, 4), MARK), 4, 5)
    row_as_col, col_as_row = Dev(np.ones(5), 5, 1), Dev(np.ones(4), 1, 4)
    for fn, args in ((lib.add_row_vec, ()), (lib.add_row_mult, (0.5,)), (lib.mult_by_row_vec, ()), (lib.div_by_row_vec, ())):
        assert fn(A.mat, row_as_col.mat, T.mat, *args) == ERR_DIMS and fn(A.mat, col_as_row.mat, T.mat, *args) == ERR_DIMS
    for fn, args in ((lib.add_col_vec, ()), (lib.add_col_mult, (0.5,)), (lib.div_by_col_vec, ())):
        assert fn(A.mat, col_as_row.mat, T.mat, *args) == ERR_DIMS and fn(A.mat, row_as_col.mat, T.mat, *args) == ERR_DIMS
    assert lib.add_to_each_pixel(A.mat, Dev(np.ones(6), 3, 2).mat, T.mat, 1.0) == ERR_DIMS       # another number of cases
    assert lib.add_to_each_pixel(A.mat, Dev(np.ones(12), 4, 3).mat, T.mat, 1.0) == ERR_DIMS      # 5 columns are no multiple of 3 colours
    same(A.get(), a), same(T.get(), np.full((5, 4), MARK, np.float32))


@pytest.mark.parametrize("mis", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("height", [8, 7, 260])
def test_shuffle_columns_on_both_sides_of_its_alignment_switch(lib, height, mis):
    import oracle
    rng = np.random.default_rng([8, height])
    for width in (2, 5, 6):
        a = rng.standard_normal((width, height)).astype(np.float32)
        perm = rng.permutation(width).astype(np.float32)
        A, P = Dev(a, height, width, mis), Dev(perm, 1, width)
        assert lib.shuffleColumns(A.mat, P.mat) == 0
        same(A.get(), oracle.port.shuffle_columns(a.copy(), perm), height, width)


# ======== c. sum_by_axis / sqsum_by_axis on every launch of axis_sum =========================================================================
UNTOUCHED = 12345.0          # where p == 0 the target's old content must not matter


def _axis_case(lib, rows, cols, mis, axis):
    t_shape = (1, cols) if axis == 0 else (rows, 1)
    for kind in ("int", "normal"):
        mat, target = R.axis_inputs(rows, cols, axis, kind)
        A = Dev(mat, rows, cols, mis)
        for sq, fn in ((False, lib.sum_by_axis), (True, lib.sqsum_by_axis)):
            for mult, p in R.MULT_P:
                start = target if p != 0 else np.full_like(target, UNTOUCHED)
                T = Dev(start, *t_shape, mis)
                assert fn(A.mat, T.mat, axis, mult, p) == 0
                got = T.get()
                if kind == "int":
                    same(got, R.sum_by_axis_exact(mat, target, axis, mult, p, sq), "sq" if sq else "sum", mult, p)
                else:
                    err = rel_err(got, R.sum_by_axis_f64(mat, target, axis, mult, p, sq))
                    print(rows, cols, "axis", axis, "sq" if sq else "sum", mult, p, "rel_err", err)
                    assert err < 1e-5, ("sq" if sq else "sum", mult, p, err)
        same(A.get(), mat, "the source")


@pytest.mark.parametrize("rows,cols,mis,path", R.AXIS0_SHAPES, ids=[f"{r}x{c}{'-misaligned' if m else ''}" for r, c, m, _ in R.AXIS0_SHAPES])
def test_column_sums_on_every_launch_path(lib, rows, cols, mis, path):
    _axis_case(lib, rows, cols, mis, 0)


@pytest.mark.parametrize("rows,cols,mis,path", R.AXIS1_SHAPES, ids=[f"{r}x{c}" for r, c, _, _ in R.AXIS1_SHAPES])
def test_row_sums(lib, rows, cols, mis, path):
    _axis_case(lib, rows, cols, mis, 1)


def test_axis_sums_refuse_a_wrong_target_or_axis(lib):
    a = np.arange(12, dtype=np.float32).reshape(4, 3)                   # (rows 3, cols 4)
    A = Dev(a, 3, 4)
    row4, col3, row3, col4 = Dev(np.full(4, MARK), 1, 4), Dev(np.full(3, MARK), 3, 1), Dev(np.full(3, MARK), 1, 3), Dev(np.full(4, MARK), 4, 1)
    for fn in (lib.sum_by_axis, lib.sqsum_by_axis):
        assert fn(A.mat, row3.mat, 0, 1.0, 0.0) == ERR_DIMS and fn(A.mat, col4.mat, 0, 1.0, 0.0) == ERR_DIMS
        assert fn(A.mat, col4.mat, 1, 1.0, 0.0) == ERR_DIMS and fn(A.mat, row3.mat, 1, 1.0, 0.0) == ERR_DIMS
        assert fn(A.mat, row4.mat, 2, 1.0, 0.0) == ERR_UNSUPPORTED and fn(A.mat, col3.mat, 2, 1.0, 0.0) == ERR_UNSUPPORTED
    for t in (row4, col3, row3, col4):
        assert np.all(t.get() == f32(MARK))


# ======== d. sum_all, vdot, euclid_norm ======================================================================================================
@pytest.mark.parametrize("mis", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_whole_matrix_reductions(lib, n, mis):
    err = ctypes.c_int(77)
    for kind in ("int", "normal"):
        x, y = R.reduce_inputs(n, kind)
        X, Y = flat(x, mis), flat(y, mis)
        got = {"sum_all": lib.sum_all(X.mat, ctypes.byref(err))}
        assert err.value == 0
        got["vdot"] = lib.vdot(X.mat, Y.mat, ctypes.byref(err))
        assert err.value == 0
        got["euclid_norm"] = lib.euclid_norm(X.mat, ctypes.byref(err))
        assert err.value == 0
        if kind == "int":
            k, q = x.astype(np.int64), y.astype(np.int64)
            assert f32(got["sum_all"]) == f32(int(k.sum())), (got["sum_all"], int(k.sum()))
            assert f32(got["vdot"]) == f32(int((k * q).sum())), (got["vdot"], int((k * q).sum()))
            assert f32(got["euclid_norm"]) == R.euclid_norm_from(int((k * k).sum())), (got["euclid_norm"], int((k * k).sum()))
        else:
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            for name, exact, scale in (("sum_all", x64.sum(), np.abs(x64).sum()), ("vdot", (x64 * y64).sum(), np.abs(x64 * y64).sum()),
                                       ("euclid_norm", np.sqrt((x64 * x64).sum()), np.sqrt((x64 * x64).sum()))):
                e = abs(got[name] - exact) / scale
                print(n, name, "relative to the sum of absolute terms", e)
                assert e < 1e-5, (name, n, got[name], exact, e)
        same(X.get(), x), same(Y.get(), y)
    short = flat(np.ones(max(n - 1, 2)), mis)
    assert lib.vdot(X.mat, short.mat, ctypes.byref(err)) == 0.0 and err.value == ERR_DIMS


# ======== e. the row-norm limit, alone and fused with the SGD step; the column-norm limit ====================================================
TARGET_MARK = -77.0


def _normlimit_both_ways(lib, mat, rows, cols, mis, axis, norm, constraint, what):
    want = R.normlimit(mat, norm, constraint, axis)
    W = Dev(mat, rows, cols, mis)
    assert lib.normlimit_by_axis(W.mat, W.mat, axis, norm, int(constraint)) == 0
    same(W.get(), want, *what, "in place")
    W, T = Dev(mat, rows, cols, mis), Dev(np.full(mat.shape, TARGET_MARK), rows, cols, mis)
    assert lib.normlimit_by_axis(W.mat, T.mat, axis, norm, int(constraint)) == 0
    same(T.get(), want, *what, "into a target")                        # every element written, factor-1 rows included
    same(W.get(), mat, *what, "the source")
    return want


@pytest.mark.parametrize("constraint", [False, True], ids=["limit", "constraint"])
@pytest.mark.parametrize("rows,cols,mis", R.NORMLIMIT_SHAPES, ids=[f"{r}x{c}{'-misaligned' if m else ''}" for r, c, m in R.NORMLIMIT_SHAPES])
def test_row_norm_limit_equals_the_float32_restatement(lib, rows, cols, mis, constraint):
    for mode in ("above", "below", "mixed"):
        mat, norm = R.normlimit_inputs(rows, cols, mode)
        want = _normlimit_both_ways(lib, mat, rows, cols, mis, 1, norm, constraint, (mode,))
        if mode == "below" and not constraint:
            same(want, mat)                                            # nothing to limit: bit-identical
        elif mode == "mixed" and not constraint:
            split = R.normlimit_split(rows)
            same(want[:, :split], mat[:, :split])
            assert not np.array_equal(want[:, split:], mat[:, split:])


def test_row_norm_limit_with_a_doubled_chunk(lib):
    rows, cols = R.NORMLIMIT_HUGE
    mat, norm = R.normlimit_inputs(rows, cols, "above")
    W = Dev(mat, rows, cols)
    assert lib.normlimit_by_axis(W.mat, W.mat, 1, norm, 0) == 0
    same(W.get(), R.normlimit(mat, norm, False))


@pytest.mark.parametrize("constraint", [False, True], ids=["limit", "constraint"])
@pytest.mark.parametrize("rows,cols", R.NORMCOLS_SHAPES)
def test_column_norm_limit_equals_the_float32_restatement(lib, rows, cols, constraint):
    for mode in ("above", "below"):
        mat, norm = R.normlimit_inputs(rows, cols, mode, axis=0)
        _normlimit_both_ways(lib, mat, rows, cols, False, 0, norm, constraint, (mode,))


@pytest.mark.parametrize("mis", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("rows,cols", R.SGD_NORMLIMIT_SHAPES)
def test_sgd_step_with_norm_limit_equals_restatement_and_the_two_separate_entries(lib, rows, cols, mis):
    g, w, h = R.sgd_inputs(rows, cols)
    for l2, clip in R.SGD_CORNERS:
        _, w1, _ = R.sgd_step(g, w, h, l2, clip, 0.5, 0.5)
        norms = np.sqrt((w1.astype(np.float64) ** 2).sum(axis=0))
        norm = float(f32(np.median(norms)))                             # about half of the rows exceed it
        for constraint in (0, 1):
            want = R.sgd_step(g, w, h, l2, clip, 0.5, 0.5, norm_limit=0 if constraint else norm, norm_constraint=norm if constraint else 0)
            if not constraint:
                unscaled = np.all(want[1] == w1, axis=0)
                assert 0 < unscaled.sum() < rows
            fused = [Dev(a, rows, cols, mis) for a in (g, w, h)]
            assert lib.sgd_momentum_step_normlimit(*(d.mat for d in fused), l2, clip, 0.5, 0.5, norm, constraint) == 0
            apart = [Dev(a, rows, cols, mis) for a in (g, w, h)]
            assert lib.sgd_momentum_step(*(d.mat for d in apart), l2, clip, 0.5, 0.5) == 0
            assert lib.normlimit_by_axis(apart[1].mat, apart[1].mat, 1, norm, constraint) == 0
            for what, a, b, v in zip(("gradient", "parameter", "history"), fused, apart, want):
                got = a.get()
                same(got, v, what, l2, clip, constraint, "against the restatement")
                same(got, b.get(), what, l2, clip, constraint, "against the separate entries")


# ======== f. the softmax family ==============================================================================================================
SOFTMAX_SHAPES = [(1, 1), (1, 2), (33, 10), (31, 33), (64, 31), (100, 1000)]
P_TOL = dict(rtol=1e-5, atol=1e-12)      # the tolerance of test_softmax_family_and_fused


def _logits(rows, cols):
    """3 x N(0, 1) on the grid of 2^-10 (so that adding 80 rounds nothing), and labels that include 0 and cols - 1"""
    rng = np.random.default_rng([9, rows, cols])
    z = (np.rint(3 * rng.standard_normal((cols, rows)) * 1024) / 1024).astype(np.float32)
    labels = rng.integers(0, cols, rows).astype(np.float32)
    labels[2::4] = np.argmax(z, axis=0)[2::4]                          # a quarter of the rows are classified correctly
    labels[0], labels[-1] = 0, cols - 1
    return z, labels


def _close(got, want, *what):
    assert np.all(np.isfinite(got)), what
    assert np.allclose(got, want, **P_TOL), (*what, float(np.abs(got / want - 1).max()))


@pytest.mark.parametrize("rows,cols", SOFTMAX_SHAPES)
def test_softmax_rows(lib, rows, cols):
    z, _ = _logits(rows, cols)
    p64 = R.softmax_f64(z)
    Z = Dev(z, rows, cols)
    assert lib.softmax_row_major(Z.mat, Z.mat) == 0
    p = Z.get()
    _close(p, p64, "in place")
    assert np.abs(p.astype(np.float64).sum(axis=0) - 1).max() < 1e-6
    Z, T = Dev(z, rows, cols), Dev(np.full(z.shape, MARK), rows, cols)
    assert lib.softmax_row_major(Z.mat, T.mat) == 0
    same(T.get(), p, "out of place against in place")
    same(Z.get(), z)
    for shift in (80.0, -80.0):                                        # large logits: the row maximum is subtracted first
        moved = z + f32(shift)
        assert np.array_equal(moved.astype(np.float64), z.astype(np.float64) + shift)
        Z = Dev(moved, rows, cols)
        assert lib.softmax_row_major(Z.mat, Z.mat) == 0
        _close(Z.get(), p64, "shifted by", shift)


def _tied_logits(rows, cols):
    """small integers with exact ties for the row maximum; even rows are labelled with the first maximum, odd rows with the last one"""
    rng = np.random.default_rng([10, rows, cols])
    z = rng.integers(0, 3, (cols, rows)).astype(np.float32)
    first = np.argmax(z, axis=0)
    last = cols - 1 - np.argmax(z[::-1], axis=0)
    labels = np.where(np.arange(rows) % 2 == 0, first, last).astype(np.float32)
    return z, labels


@pytest.mark.parametrize("rows,cols", SOFTMAX_SHAPES)
def test_first_maximum_wins_a_tie(lib, rows, cols):
    z, labels = _tied_logits(rows, cols)
    want = R.softmax_correct(z, labels)
    if cols > 2 and rows > 2:
        assert 0 < want.sum() < rows                                    # some labels sit on a later tie
    Z, L, T = Dev(z, rows, cols), Dev(labels, rows, 1), Dev(np.full(rows, MARK), rows, 1)
    assert lib.get_softmax_correct_row_major(Z.mat, L.mat, T.mat) == 0
    same(T.get(), want)
    P, C = Dev(np.zeros_like(z), rows, cols), Dev(np.zeros(1), 1, 1)
    assert lib.softmax_ce_grad_correct(Z.mat, L.mat, P.mat, None, C.mat, 1.0) == 0
    assert C.get()[0] == want.sum()
    same(Z.get(), z), same(L.get(), labels)


@pytest.mark.parametrize("rows,cols", SOFTMAX_SHAPES)
def test_fused_softmax_ce_grad_correct(lib, rows, cols):
    z, labels = _logits(rows, cols)
    p64 = R.softmax_f64(z)
    count = R.softmax_correct(z, labels).sum()

    def run(deriv=True, correct=True, scale=1.0, calls=1):
        Z, L = Dev(z, rows, cols), Dev(labels, rows, 1)
        P, D, C = Dev(np.full(z.shape, MARK), rows, cols), Dev(np.full(z.shape, MARK), rows, cols), Dev(np.zeros(1), 1, 1)
        for _ in range(calls):
            assert lib.softmax_ce_grad_correct(Z.mat, L.mat, P.mat, D.mat if deriv else None, C.mat if correct else None, scale) == 0
        same(Z.get(), z), same(L.get(), labels)
        return P.get(), D.get(), C.get()[0]

    p, d, c = run()
    _close(p, p64, "probabilities")
    same(d, R.softmax_grad(p, labels), "derivative")                    # p, with exactly 1 subtracted at the label
    assert c == count
    p2, d2, c2 = run(calls=2)
    same(p2, p), same(d2, d)
    assert c2 == 2 * count                                              # the count accumulates over calls
    p3, d3, c3 = run(scale=0.25)
    same(p3, p), same(d3, f32(0.25) * d, "deriv_scale")
    assert c3 == count
    p4, d4, c4 = run(deriv=False)
    same(p4, p), same(d4, np.full(z.shape, MARK, np.float32), "an absent derivative")
    assert c4 == count
    p5, d5, c5 = run(correct=False)
    same(p5, p), same(d5, d)
    assert c5 == 0


@pytest.mark.parametrize("rows,cols", SOFTMAX_SHAPES)
def test_cross_entropy_and_its_derivative_on_probabilities(lib, rows, cols):
    z, labels = _logits(rows, cols)
    p = R.softmax_f64(z).astype(np.float32)
    lab = labels.astype(np.int64)
    p[lab[::3], np.arange(rows)[::3]] = 0                                # a probability of exactly 0 at the label
    tiny = 1e-10
    P, L, T = Dev(p, rows, cols), Dev(labels, rows, 1), Dev(np.full(rows, MARK), rows, 1)
    assert lib.get_softmax_cross_entropy_row_major(P.mat, L.mat, T.mat, tiny) == 0
    ce = T.get()
    err = rel_err(ce, R.softmax_ce_f64(p, labels, tiny))
    assert err < 1e-5, err                                              # the bound of test_softmax_family_and_fused
    assert np.all(np.abs(ce[::3].astype(np.float64) + np.log(np.float64(f32(tiny)))) <= 1e-5 * -np.log(tiny)), ce[::3]
    same(P.get(), p)
    want = R.softmax_grad(p, labels)
    assert lib.apply_softmax_grad_row_major(P.mat, L.mat, P.mat) == 0
    same(P.get(), want, "in place")
    P, T = Dev(p, rows, cols), Dev(np.full(p.shape, MARK), rows, cols)
    assert lib.apply_softmax_grad_row_major(P.mat, L.mat, T.mat) == 0
    same(T.get(), want, "into a target"), same(P.get(), p), same(L.get(), labels)


@pytest.mark.parametrize("rows,cols,k", [(33, 10, 2), (31, 33, 3), (5, 12, 4), (64, 31, 1)])
def test_softmax_multi_reads_the_bytes_as_numslices_columns(lib, rows, cols, k):
    z, _ = _logits(rows, cols)
    Z = Dev(z, rows, cols)
    assert lib.softmax_row_major(Z.mat, Z.mat) == 0
    want = Z.get()
    Zk, T = Dev(z, rows * k, cols // k), Dev(np.full(z.shape, MARK), rows * k, cols // k)
    assert lib.softmax_row_major_multi(Zk.mat, cols, T.mat) == 0
    same(T.get(), want)
    _close(T.get(), R.softmax_f64(z))
    same(Zk.get(), z)
    if rows * cols % 7:
        assert lib.softmax_row_major_multi(Zk.mat, 7, T.mat) == ERR_DIMS
    assert lib.softmax_row_major_multi(Zk.mat, 0, T.mat) == ERR_DIMS
    same(T.get(), want)


# ======== g. the random entries ==============================================================================================================
N_RNG = (1 << 20) + 3          # the last group of four draws is ragged


@pytest.fixture()
def rnd(lib):
    """a generator state of the test's own: the stream Matrix._rnd hands later tests stays where it is"""
    from convnet_amd import _lib

    def make(seed):
        st = _lib.rnd_struct()
        assert lib.init_random(ctypes.byref(st), seed) == 0
        return st
    return make


def test_uniform_and_normal_fills(lib, rnd):
    n = N_RNG
    st = rnd(1234)
    U = flat(np.full(n, MARK))
    assert lib.fill_with_rand(ctypes.byref(st), U.mat) == 0
    u1 = U.get().copy()
    assert u1.min() >= 0 and u1.max() < 1
    assert abs(u1.astype(np.float64).mean() - 0.5) < 6 / np.sqrt(12 * n)
    assert lib.fill_with_rand(ctypes.byref(st), U.mat) == 0
    u2 = U.get().copy()
    assert not np.array_equal(u1, u2)
    assert abs(np.corrcoef(u1.astype(np.float64), u2.astype(np.float64))[0, 1]) < 6 / np.sqrt(n)
    G = flat(np.full(n, MARK), mis=True)
    assert lib.fill_with_randn(ctypes.byref(st), G.mat) == 0
    g1 = G.get().astype(np.float64)
    assert np.all(np.isfinite(g1))
    assert abs(g1.mean()) < 6 / np.sqrt(n) and abs(g1.var() - 1) < 6 * np.sqrt(2 / n)
    assert lib.fill_with_randn(ctypes.byref(st), G.mat) == 0
    g2 = G.get().astype(np.float64)
    assert not np.array_equal(g1, g2) and abs(np.corrcoef(g1, g2)[0, 1]) < 6 / np.sqrt(n)
    # the same seed replays the stream; another seed does not
    again, other = rnd(1234), rnd(1235)
    assert lib.fill_with_rand(ctypes.byref(again), U.mat) == 0
    same(U.get(), u1, "re-seeded")
    assert lib.fill_with_rand(ctypes.byref(other), U.mat) == 0
    assert not np.array_equal(U.get(), u1)


@pytest.mark.parametrize("p", [0.0, 0.25, 1.0])
def test_sample_bernoulli(lib, rnd, p):
    n = N_RNG
    st = rnd(99)
    for in_place in (False, True):
        Pm = flat(np.full(n, p))
        T = Pm if in_place else flat(np.full(n, MARK), mis=True)
        assert lib.sample_bernoulli(ctypes.byref(st), Pm.mat, T.mat) == 0
        x = T.get()
        assert np.all((x == 0) | (x == 1))
        assert abs(x.astype(np.float64).mean() - p) <= 6 * np.sqrt(p * (1 - p) / n), (p, x.mean())
        if not in_place:
            same(Pm.get(), np.full(n, p, np.float32))
    assert lib.sample_bernoulli(ctypes.byref(st), Pm.mat, flat(np.zeros(5)).mat) == ERR_DIMS


def test_sample_bernoulli_compares_strictly_with_its_draw(lib, rnd):
    """target = (draw < p), as the reference's `p > uniform`.  The stream is keyed by (seed, call counter, element index) and the uniform
    fill writes the draws themselves, so the first call of a re-seeded state draws what the first fill of that seed wrote: with p equal
    to the draw, element for element, nothing fires; with p one ulp above it, everything does.  (A draw equal to p has probability 2^-24
    per element otherwise, which no statistic sees.)"""
    n = N_RNG
    U = flat(np.zeros(n))
    assert lib.fill_with_rand(ctypes.byref(rnd(4321)), U.mat) == 0
    u = U.get().copy()
    T = flat(np.full(n, MARK), mis=True)
    assert lib.sample_bernoulli(ctypes.byref(rnd(4321)), U.mat, T.mat) == 0
    same(T.get(), np.zeros(n, np.float32), "p equal to the draw")
    above = flat(np.maximum(np.nextafter(u, f32(2)), f32(2.0 ** -25)))          # (no denormal above a draw of 0)
    assert lib.sample_bernoulli(ctypes.byref(rnd(4321)), above.mat, T.mat) == 0
    same(T.get(), np.ones(n, np.float32), "p one ulp above the draw")


def test_dropout_writes_its_fill_value(lib, rnd):
    n, p = N_RNG, 0.4
    x = (1 + np.random.default_rng(11).random(n)).astype(np.float32)    # in [1, 2): x * scale is never the fill value
    X = flat(x)
    assert lib.dropout(ctypes.byref(rnd(7)), X.mat, p, -3.0, 2.0) == 0
    y = X.get()
    dropped = y == f32(-3)
    assert abs(dropped.mean() - p) < 6 * np.sqrt(p * (1 - p) / n)
    same(y[~dropped], (x * f32(2))[~dropped])


# ======== h. copies and views ================================================================================================================
def test_slice_copies_move_exactly_their_columns(M, lib):
    rows, cols = 5, 9
    vals = np.arange(rows * cols, dtype=np.float32).reshape(cols, rows) + 100
    for start, end in ((0, 1), (3, 7), (8, 9)):
        m = M(rows, cols)
        m.FromNumpy(np.full((cols, rows), -1.0))                        # the device holds the marker; data_host now points at m's host mirror
        m.GetHostData()[:] = vals
        assert lib.copy_to_device_slice(m.GetMat(), start, end) == 0
        want = np.full((cols, rows), -1.0, np.float32)
        want[start:end] = vals[start:end]
        same(m.ToNumpy(), want, "to device", start, end)
        m.FromNumpy(vals)
        m.GetHostData()[:] = -5.0
        assert lib.copy_to_host_slice(m.GetMat(), start, end) == 0
        want = np.full((cols, rows), -5.0, np.float32)
        want[start:end] = vals[start:end]
        same(m.GetHostData().copy(), want, "to host", start, end)
    # csrc/state.hip: the device-bound copy refuses an empty or out-of-range slice with ERROR_GENERIC (cudamat.cu:325-347), the host-bound
    # one an out-of-range or reversed slice with ERROR_INCOMPATIBLE_DIMENSIONS, and copies nothing for an empty one
    assert lib.copy_to_device_slice(m.GetMat(), 3, 3) == ERR_GENERIC and lib.copy_to_device_slice(m.GetMat(), 4, 3) == ERR_GENERIC
    assert lib.copy_to_device_slice(m.GetMat(), 8, 10) == ERR_GENERIC
    assert lib.copy_to_host_slice(m.GetMat(), 8, 10) == ERR_DIMS and lib.copy_to_host_slice(m.GetMat(), 4, 3) == ERR_DIMS
    assert lib.copy_to_host_slice(m.GetMat(), 3, 3) == 0
    same(m.GetHostData().copy(), want)
    same(m.ToNumpy(), vals)


def test_reshape_and_slices(M, lib):
    rows, cols = 5, 9
    vals = np.arange(rows * cols, dtype=np.float32).reshape(cols, rows)
    m = M(rows, cols)
    m.FromNumpy(vals)
    size = lambda: (m.mat_.size[0], m.mat_.size[1])      # noqa: E731
    assert lib.reshape(m.GetMat(), -1, 15) == 0 and size() == (3, 15)
    assert lib.reshape(m.GetMat(), 9, -1) == 0 and size() == (9, 5)
    assert lib.reshape(m.GetMat(), -1, -1) == ERR_GENERIC and size() == (9, 5)
    assert lib.reshape(m.GetMat(), 4, 7) == ERR_DIMS and lib.reshape(m.GetMat(), -1, 7) == ERR_DIMS and lib.reshape(m.GetMat(), 7, -1) == ERR_DIMS
    assert size() == (9, 5)
    assert lib.reshape(m.GetMat(), rows, cols) == 0
    same(m.ToNumpy(), vals)                                             # a reshape moves nothing
    s = M()
    for first, last in ((3, 3), (4, 3), (8, 10), (9, 10)):
        assert lib.get_slice(m.GetMat(), s.GetMat(), first, last) == ERR_DIMS
    s1, s2 = M(), M()
    m.GetSlice(s1, 2, 8)
    s1.GetSlice(s2, 1, 3)                                               # columns [3, 5) of m
    assert (s2.GetRows(), s2.GetCols()) == (rows, 2) and s2.mat_.data_device == m.mat_.data_device + 4 * rows * 3
    s2.Set(9.0)
    s2.WriteValue(1, 1, -2.0)                                           # row 1 of column 4 of m
    want = vals.copy()
    want[3:5] = 9.0
    want[4, 1] = -2.0
    same(m.ToNumpy(), want)
    same(s1.ToNumpy(), want[2:8])


def test_library_owned_allocations_round_trip(M, lib):
    from convnet_amd import _lib
    host = np.arange(12, dtype=np.float32)
    a = _lib.cudamat()
    lib.init_from_array(ctypes.byref(a), host.ctypes.data_as(_lib.c_float_p), 3, 4)
    assert (a.size[0], a.size[1], a.on_device, a.on_host, a.owns_data) == (3, 4, 0, 1, 1)
    assert lib.copy_to_device(ctypes.byref(a)) == 0 and a.on_device == 1          # the first copy allocates
    b = _lib.cudamat()
    assert lib.init_empty(ctypes.byref(b), 3, 4) == 0 and b.on_device == 1 and b.owns_data == 1
    assert lib.copy_on_device(ctypes.byref(a), ctypes.byref(b)) == 0
    assert lib.add_scalar(ctypes.byref(b), 0.5, ctypes.byref(b)) == 0
    back = np.zeros(12, np.float32)
    b.data_host = back.ctypes.data_as(_lib.c_float_p)
    assert lib.copy_to_host(ctypes.byref(b)) == 0
    same(back, host + f32(0.5))
    c = _lib.cudamat()
    c.size[0], c.size[1] = 2, 6
    assert lib.allocate_device_memory(ctypes.byref(c)) == 0 and c.on_device == 1
    c.owns_data = 1
    assert lib.copy_on_device(ctypes.byref(a), ctypes.byref(c)) == ERR_DIMS
    for m in (a, b, c):
        assert lib.free_device_memory(ctypes.byref(m)) == 0 and m.on_device == 0
