"""CPU: the float64 reference of tests/pool_norm_ref.py against the oracle's compiled C (oracle.port), on the arrays
tests/test_pool_norm_gpu.py uses — which also shows that the bounds of that file admit a correct float32 implementation — and the
preconditions of its exact cases.

Why the exact cases are exact: every pooling input, derivative and target of those cases is a small integer and every scale one of
0, 1, -2, 0.5.  Every routed sum and every st * t0 + so * v is then an integer multiple of 1/2 whose terms' magnitudes add up to less
than 2^23, so every partial result in every order (and through an fma or not) is a float32: computed without rounding
(the argument tests/test_elementwise_ref_cpu.py makes for its sums).

The oracle's pool undo assumes square maps and windows (NOTES.md, reference quirks): it is compared on the square geometries only; the
rectangular ones have the float64 reference alone."""
import numpy as np
import pytest

import oracle
import pool_norm_ref as P

f32 = np.float32


def _within(got, exact, bound, *what):
    err = np.abs(np.asarray(got, np.float64) - exact)
    assert np.all(err <= bound), (*what, float((err - bound).max()), int((err > bound).sum()))


@pytest.mark.parametrize("name", P.SQUARE_CASES)
def test_pooling_reference_agrees_with_the_oracle_on_square_geometries(name):
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    for x in (d["xi"], d["x5"], d["xn"]):
        got = oracle.port.max_pool(g, x).reshape(P.shape_out(g))
        assert np.array_equal(got, P.max_fwd(g, x)), "max pool"
    for st in P.UNDO_SCALES:
        got = oracle.port.max_pool_undo(g, d["xi"], d["dyi"], d["yi"], d["ti_in"].copy(), st).reshape(P.shape_in(g))
        assert np.array_equal(got, P.max_undo(g, d["xi"], d["dyi"], d["yi"], d["ti_in"], st)), ("max undo", st)
    for x in (d["xn"], d["xw"]):
        for st, so in P.SCALES:
            got = oracle.port.avg_pool(g, x, d["tn_out"].copy(), st, so).reshape(P.shape_out(g))
            _within(got, *P.avg_fwd(g, x, d["tn_out"], st, so), "avg pool", st, so)
    for dy in (d["dyn"], d["dyw"]):
        for st in P.UNDO_SCALES:
            got = oracle.port.avg_pool_undo(g, dy, d["tn_in"].copy(), st).reshape(P.shape_in(g))
            exact, bound, covered = P.avg_undo(g, dy, d["tn_in"], st)
            _within(got, exact, bound, "avg undo", st)
            assert np.array_equal(got[~covered], (f32(st) * d["tn_in"])[~covered]), "a pixel no window covers is exactly st * t0"


@pytest.mark.parametrize("name", list(P.POOL_GEOMS))
def test_exact_pooling_cases_are_exact_in_any_float32_order(name):
    g, d = P.POOL_GEOMS[name], P.pool_data(name)
    for a in (d["xi"], d["dyi"], d["ti_in"], d["ti_out"], d["x5"]):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 5
    n, m = P.box_sizes(g)
    # forward: |st * t0| + |so * max| with |values| <= 5, |scales| <= 2: a multiple of 1/2 below 2^23
    for x in (d["xi"], d["x5"]):
        for st, so in P.SCALES:
            r = P.max_fwd(g, x, d["ti_out"], st, so)
            assert np.array_equal(2 * r, np.round(2 * r))
            assert (abs(st) * np.abs(d["ti_out"]) + abs(so) * np.abs(P.max_fwd(g, x))).max() * 2 < 1 << 24
    # undo: at most m routed integer derivatives plus |st * t0|: the sum of magnitudes bounds every partial sum of every order
    mag = np.abs(d["dyi"]).max() * m.max() + 2 * np.abs(d["ti_in"]).max()
    assert mag < 1 << 24
    for st in P.UNDO_SCALES:
        for relu in (False, True):
            r = P.max_undo(g, d["xi"], d["dyi"], d["yi"], d["ti_in"], st, relu)
            assert np.array_equal(r, np.round(r)) and np.abs(r).max() <= mag
            assert np.array_equal(r.astype(f32).astype(np.float64), r)
    # MaxPoolUndoRelu masks the accumulated target too
    r = P.max_undo(g, d["xi"], d["dyi"], d["yi"], d["ti_in"], 1.0, True)
    assert np.all(r[d["xi"] <= 0] == 0) and np.any(d["ti_in"][d["xi"] <= 0] != 0)
    # the data do what the cases are there for: negative maxima, ties, an all-negative tensor whose padded taps must not count as 0
    assert (d["yi"] < 0).any() and np.all(P.max_fwd(g, d["x5"]) == -5.0)
    assert (P.max_undo(g, d["xi"], np.ones_like(d["dyi"]), d["yi"]).sum() > d["yi"].size), "no ties in the integer data"


@pytest.mark.parametrize("name", list(P.RNORM_CASES))
def test_response_norm_reference_and_bound_against_the_oracle(name):
    """the error scale is sound: the fp32 oracle's error in units of 2^-24 * s_j is finite (exact zeros where s = 0) and, on N(0, 1)
    data, small.  The GPU file allows 4 * (this figure) + 34 on the same arrays."""
    size_f, blocked, shape, _ = P.RNORM_CASES[name]
    d = P.rnorm_data(name)
    for a, b in P.PARAMS:
        for kind in ("n", "w"):
            x, dy = d["x" + kind], d["dy" + kind]
            exact, s = P.rnorm_fwd(x, size_f, a, b, blocked)
            e_f = P.units(oracle.port.rnorm(x, size_f, a, b, blocked), exact, s)
            exact, s = P.rnorm_undo(dy, x, size_f, a, b, blocked)
            e_u = P.units(oracle.port.rnorm_undo(dy, x, size_f, a, b, blocked), exact, s)
            print(f"E_case {name} ({a}, {b}) {'N(0,1)' if kind == 'n' else 'wide'}: forward {e_f:.1f} undo {e_u:.1f} units")
            assert np.isfinite(e_f) and np.isfinite(e_u)
            if kind == "n":
                assert e_f <= 40 and e_u <= 120, (e_f, e_u)     # twice the figures measured when the bound was set (20, 57)


def test_case_lists_reach_every_kernel_and_launch_form():
    reached = set()
    for name, mis in P.POOL_CASES:
        reached |= set(P.pool_paths(name, mis).values())
    for name in P.RNORM_CASES:
        reached |= set(P.rnorm_paths(name).values())
    missing = [p for p in P.REQUIRED_PATHS if p not in reached]
    assert not missing, (missing, sorted(reached))
    # single rows, worked out by hand from the dispatch
    assert P.rnorm_paths("fast64_C100") == {"rnorm_fwd": "rnorm_fwd_fast_kernel<32, 8, 64>", "rnorm_undo": "rnorm_undo_fast_kernel<32, 8, 64>"}
    assert P.rnorm_paths("fast24_C90")["rnorm_fwd"] == "rnorm_fwd_fast_kernel<64, 12, 24>"
    assert P.rnorm_paths("lds_C160_w5") == {"rnorm_fwd": "rnorm_fwd_lds_kernel<64>/vec", "rnorm_undo": "rnorm_undo_lds_kernel<16>/512/vec"}
    assert P.rnorm_paths("lds_C520_w5")["rnorm_undo"] == "rnorm_undo1_kernel+rnorm_undo2_kernel/vec" and P._rn_segments(36, 520, 5) == (8, 65)
    assert P._rn_segments(8, 800, 64) == (67, 12) and P._rn_segments(6, 800, 64) == (67, 12)
    g = P.POOL_GEOMS["blk_43x41_C2"]
    assert (g.My, g.Mx) == (21, 20) and P.pool_paths("blk_43x41_C2", False)["max_fwd"] == "pool_fwd_max32_block_kernel/grid3d"
    assert P.pool_paths("blk_21x20_p1_C3", False)["max_fwd"].startswith("pool_fwd_fixed_kernel<max, 3, 2>")
    assert P.pool_paths("blk_21x20_p1_C3", False)["max_undo"] == "pool_undo_max32_block_kernel/grid3d"
