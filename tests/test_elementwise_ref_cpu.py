"""CPU: the numpy restatements of tests/elementwise_ref.py against the oracle's compiled C (oracle.port), and the preconditions of the
exact-arithmetic cases of tests/test_elementwise_gpu.py, proved on the very arrays that file uses.

Why the exact cases are exact: when every term of a sum is an integer multiple of one unit u and the sum of the terms' magnitudes is
below 2^24 u, every partial sum in every order is such a multiple below 2^24 u, hence a float32, hence computed without rounding: a
float32 sum in ANY order (any tree, any number of lanes) equals the integer sum.  The tests assert the bound and also sum in random
orders."""
import numpy as np
import pytest

import elementwise_ref as R
import oracle
from golden_cases import rel_err

f32 = np.float32
LIMIT = 1 << 24
RAGGED = [(1, 1), (3, 5), (7, 4), (37, 50), (33, 130)]      # (cols, rows)


def rnd(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


# ---- 1. restatement == oracle.port, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RAGGED)
def test_vector_and_clamp_restatements_equal_the_oracle_bit_for_bit(shape):
    rng = np.random.default_rng(31)
    cols, rows = shape
    a, rowv, colv = rnd(rng, shape), rnd(rng, cols), rnd(rng, rows)
    assert np.array_equal(R.add_row_mult(a, rowv), oracle.port.add_row_vec(a.copy(), rowv))
    for mult in (1.0, -1.0, 0.5, 0.3):
        assert np.array_equal(R.add_col_mult(a, colv, mult), oracle.port.add_col_mult(a.copy(), colv, mult))
    assert np.array_equal(R.div_by_col_vec(a, colv), oracle.port.div_by_col_vec(a.copy(), colv))
    assert np.array_equal(R.mult_by_row_vec(a, rowv), oracle.port.mult_by_row_vec(a.copy(), rowv))
    assert np.array_equal(R.lower_bound_scalar(a, 0.0), oracle.port.lower_bound(a.copy(), 0.0))
    assert np.array_equal(R.lower_bound_scalar(a, -0.25), oracle.port.lower_bound(a.copy(), -0.25))
    assert np.array_equal(R.upper_bound_mod_scalar(a, 0.4), oracle.port.upper_bound_mod(a.copy(), 0.4))
    st = np.maximum(rnd(rng, shape), 0)
    got, want = R.relu_deriv(a, st), oracle.port.relu_deriv(a.copy(), st)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("colours,pixels,cases", [(1, 7, 5), (3, 7, 5), (3, 1, 1), (2, 13, 33)])
def test_add_to_each_pixel_restatement_equals_the_oracle(colours, pixels, cases):
    rng = np.random.default_rng(32)
    a, noise = rnd(rng, (colours * pixels, cases)), rnd(rng, (colours, cases))
    for mult in (1.0, 0.3):
        assert np.array_equal(R.add_to_each_pixel(a, noise, mult), oracle.port.add_to_each_pixel(a.copy(), noise, mult))


@pytest.mark.parametrize("shape", RAGGED)
def test_sum_by_axis_restatements_equal_the_oracle(shape):
    """integer data: bit for bit (the oracle sums in double, which is exact here too); N(0, 1): the bound of the existing reductions test"""
    rng = np.random.default_rng(33)
    cols, rows = shape
    for axis, n in ((0, cols), (1, rows)):
        a, t = R.integer_data(rng, shape, 8), R.integer_data(rng, n, 8)
        for mult, p in R.MULT_P:
            want = oracle.port.sum_by_axis(a, (t if p else np.zeros_like(t)).copy(), axis, mult, p)
            assert np.array_equal(R.sum_by_axis_exact(a, t, axis, mult, p), want)
        a, t = rnd(rng, shape), rnd(rng, n)
        for mult, p in R.MULT_P:
            want = oracle.port.sum_by_axis(a, (t if p else np.zeros_like(t)).copy(), axis, mult, p)
            assert rel_err(R.sum_by_axis_f64(a, t, axis, mult, p).astype(np.float32), want) < 1e-5


@pytest.mark.parametrize("shape", RAGGED)
def test_normlimit_and_sgd_restatements_equal_the_oracle_bit_for_bit(shape):
    rng = np.random.default_rng(34)
    cols, rows = shape
    for a in (rnd(rng, shape), R.grid_data(rng, shape) + f32(0.125)):
        for lim, con in ((0.8, False), (1.5, True), (100.0, False)):
            assert np.array_equal(R.normlimit(a, lim, con), oracle.port.normlimit_rows(a.copy(), lim, con))
    for l2, clip, limit, constraint in ((0.0, 0.0, 0.0, 0.0), (0.01, 0.3, 0.0, 0.0), (0.01, 0.0, 0.9, 0.0), (0.0, 0.3, 0.0, 1.1), (0.25, 2.0, 1.0, 0.0)):
        g, w, h = rnd(rng, shape), rnd(rng, shape), rnd(rng, shape)
        want = [g.copy(), w.copy(), h.copy()]
        oracle.port.sgd_step(*want, l2, clip, 0.05, 0.9, limit, constraint)
        got = R.sgd_step(g, w, h, l2, clip, 0.05, 0.9, limit, constraint)
        for what, x, y in zip(("gradient", "parameter", "history"), got, want):
            assert np.array_equal(x, y), (what, l2, clip, limit, constraint, rel_err(x, y))


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 2), (5, 3), (33, 10), (31, 33)])
def test_softmax_family_restatements_equal_the_oracle(rows, cols):
    rng = np.random.default_rng(35)
    z = 3 * rnd(rng, (cols, rows))
    labels = rng.integers(0, cols, rows).astype(np.float32)
    p = oracle.port.softmax_row_major(z.copy())
    assert np.allclose(R.softmax_f64(z), p, rtol=1e-5, atol=1e-12)            # the tolerance of test_softmax_family_and_fused
    assert np.allclose(R.softmax_f32(z), p, rtol=1e-5, atol=1e-12)
    assert np.array_equal(R.softmax_grad(p, labels), oracle.port.softmax_grad_row_major(p, labels))
    assert np.array_equal(R.softmax_correct(p, labels), oracle.port.softmax_correct_row_major(p, labels))
    ties = rng.integers(0, 3, (cols, rows)).astype(np.float32)               # exact ties for the maximum: the first one counts
    assert np.array_equal(R.softmax_correct(ties, labels), oracle.port.softmax_correct_row_major(ties, labels))
    assert rel_err(R.softmax_ce_f64(p, labels, 1e-10).astype(np.float32), oracle.port.softmax_ce_row_major(p, labels)) < 1e-5
    assert rel_err(R.softmax_ce_f32(p, labels, 1e-10), oracle.port.softmax_ce_row_major(p, labels)) < 1e-5


def test_normalize_columns_within_the_existing_tolerance():
    rng = np.random.default_rng(36)
    a = rnd(rng, (37, 50))
    want = (a.astype(np.float64) - a.astype(np.float64).mean(axis=1, keepdims=True)).astype(np.float32)
    assert rel_err(oracle.port.normalize_columns(a.copy()), want) < 1e-6


# ---- 2. the preconditions of the exact cases ------------------------------------------------------------------------------------------------
def _orders_agree(terms, want, rng, orders=2):
    """terms: (k, units) float32, summed over axis 0: numpy's pairwise tree, index order, and random orders, all in float32"""
    assert np.array_equal(terms.sum(axis=0, dtype=np.float32), want)
    assert np.array_equal(np.cumsum(terms, axis=0, dtype=np.float32)[-1], want)
    for _ in range(orders):
        assert np.array_equal(np.cumsum(terms[rng.permutation(terms.shape[0])], axis=0, dtype=np.float32)[-1], want)


@pytest.mark.parametrize("rows,cols,axis", [(s[0], s[1], 0) for s in R.AXIS0_SHAPES if not s[2]] + [(s[0], s[1], 1) for s in R.AXIS1_SHAPES])
def test_axis_sum_cases_are_exact_in_any_order(rows, cols, axis):
    mat, target = R.axis_inputs(rows, cols, axis, "int")
    rng = np.random.default_rng(41)
    for sq in (False, True):
        terms = (mat * mat if sq else mat)
        terms = terms.T if axis == 0 else terms                      # summed over axis 0 of `terms`
        total = R.axis_total_exact(mat, axis, sq)
        assert int(np.abs(terms.astype(np.int64)).sum(axis=0).max()) < LIMIT          # in units of 1
        if sq:
            assert 64 * (rows if axis == 0 else cols) < LIMIT
        _orders_agree(np.ascontiguousarray(terms), total.astype(np.float32), rng)
        # p*target + mult*sum: multiples of 1/4 whose magnitudes sum below 2^24 quarters, so neither product nor the sum rounds
        for mult, p in R.MULT_P:
            quarters = 4 * (p * np.abs(target.astype(np.float64)) + mult * np.abs(total))
            assert np.array_equal(quarters, np.rint(quarters)) and quarters.max() < LIMIT
            want = p * target.astype(np.float64) + mult * total
            assert np.array_equal(R.sum_by_axis_exact(mat, target, axis, mult, p, sq).astype(np.float64), want)


@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_whole_matrix_reduction_cases_are_exact_in_any_order(n):
    x, y = R.reduce_inputs(n, "int")
    rng = np.random.default_rng(42)
    for terms in (x, x * y, x * x):
        assert R.abs_total_in_units(terms, 1.0) < LIMIT
        want = f32(int(terms.astype(np.int64).sum()))
        _orders_agree(terms.reshape(-1, 1), np.array([want]), rng)


def _unit_sums(mat, axis):
    """squares of grid data per row (axis 1) or column (axis 0): terms (k, units) and their exact sums"""
    m = mat if axis == 1 else np.ascontiguousarray(mat.T)
    sq = m * m
    unit = 1.0 / (R.GRID * R.GRID)
    k = np.rint(sq.astype(np.float64) / unit).astype(np.int64)
    assert np.array_equal(k * unit, sq.astype(np.float64))            # the fp32 squares are exact and on the grid of 1/64
    assert int(k.sum(axis=0).max()) < LIMIT
    return sq, (k.sum(axis=0) * unit).astype(np.float32)


@pytest.mark.parametrize("rows,cols,axis", [(r, c, 1) for r, c, _ in R.NORMLIMIT_SHAPES] + [(r, c, 0) for r, c in R.NORMCOLS_SHAPES])
def test_normlimit_cases_have_exact_sums_of_squares(rows, cols, axis):
    rng = np.random.default_rng(43)
    for mode in ("above", "below") + (("mixed",) if axis == 1 else ()):
        mat, norm = R.normlimit_inputs(rows, cols, mode, axis)
        sq, want = _unit_sums(mat, axis)
        assert want.min() > 0                                          # no all-zero row
        _orders_agree(sq, want, rng)
        s = np.sqrt(want)
        above = s > f32(norm)
        if mode == "above":
            assert above.all()
        elif mode == "below":
            assert not above.any()
            assert np.array_equal(R.normlimit(mat, norm, False, axis), mat)
        else:
            split = R.normlimit_split(rows)
            assert 0 < split < rows and not above[:split].any() and above[split:].all()


def test_the_chunk_doubling_case_has_exact_sums_of_squares():
    rows, cols = R.NORMLIMIT_HUGE
    assert -(-rows // 256) * -(-cols // 64) > 4096 >= -(-rows // 256) * -(-cols // 128)      # 64-column chunks are too many, 128 are not
    mat, norm = R.normlimit_inputs(rows, cols, "above")
    assert 64 * cols < LIMIT                                           # squares are at most 64 units of 1/64
    sq, want = _unit_sums(mat, 1)
    _orders_agree(sq, want, np.random.default_rng(44), orders=1)
    assert (np.sqrt(want) > f32(norm)).all()


@pytest.mark.parametrize("rows,cols", R.SGD_NORMLIMIT_SHAPES)
def test_sgd_normlimit_cases_step_exactly_and_have_exact_sums_of_squares(rows, cols):
    assert cols <= 400
    rng = np.random.default_rng(45)
    for l2, clip in R.SGD_CORNERS:
        g, w, h = R.sgd_inputs(rows, cols)
        g1, w1, h1 = R.sgd_step(g, w, h, l2, clip, 0.5, 0.5)
        g64, w64, h64 = (a.astype(np.float64) for a in (g, w, h))
        if l2 > 0:
            g64 = g64 + l2 * w64
        if clip > 0:
            g64 = np.clip(g64, -clip, clip)
        g64 = g64 * 0.5
        h64 = 0.5 * h64 + g64
        w64 = w64 - h64
        for got, want in ((g1, g64), (w1, w64), (h1, h64)):             # no statement of the step rounds
            assert np.array_equal(got.astype(np.float64), want) and np.array_equal(want * 8, np.rint(want * 8))
        assert np.abs(w1).max() <= 8.5
        sq = w1 * w1
        k = np.rint(sq.astype(np.float64) * 64).astype(np.int64)
        assert np.array_equal(k / 64.0, sq.astype(np.float64)) and int(k.sum(axis=0).max()) < LIMIT
        _orders_agree(sq, (k.sum(axis=0) / 64.0).astype(np.float32), rng)
        assert (k.sum(axis=0) > 0).all()
