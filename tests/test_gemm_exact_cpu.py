"""tests/gemm_exact.py without a GPU: its float64 reference against the fp32 oracle (oracle.port, exact on these integers) and
tests/local_ref.py, the exactness condition on every (row, family) tests/test_gemm_exact_gpu.py runs, the h / m / l planes of the
*_hm families under a numpy restatement of the bf16 split, and the guard checker on a numpy stand-in for a kernel."""
import numpy as np
import pytest

import gemm_exact as E
import local_ref as L
import oracle
from split_cases import CASES

ORACLE_MACS = 5e8       # the rows the plain-loop oracle evaluates whole in a second or two
SMALL = [c for c in CASES if E.macs(c) <= ORACLE_MACS or c.entry.startswith("local_strided")]
BY_ID = {c.id: c for c in CASES}


def test_every_row_runs_with_at_least_the_h_family():
    for c in CASES:
        fams = E.families(c)
        assert fams[0] == "h" and (fams == E.FAMILIES or fams == ("h",)), (c.id, fams)
        assert (fams == ("h",)) == (c.id in E.H_ONLY), (c.id, "only the rows above MAX_MACS give up their *_hm families")
    assert set(E.H_ONLY) == {"dgrad_mask_tail", "fwd_gpw_tail"}
    ops = {c.op for c in SMALL}
    assert {"fprop", "dgrad", "wgrad", "fc_nt", "fc_nn", "fc_tn", "local_up", "local_down", "local_outp"} <= ops, ops


def test_the_value_grid_of_the_epilogue_factors():
    assert E.grid(BY_ID["fwd_gfc"]) == 1.0 and E.grid(BY_ID["fwd_gfc_accumulate"]) == 1.0       # 0.75 * 4 j = 3 j
    assert E.grid(BY_ID["wgrad_wg_64"]) == 0.25 and E.grid(BY_ID["wgrad_bias_fallback"]) == 1.0   # so = 0.25; st = 0.5, so = 2
    assert E.radius(BY_ID["wgrad_reduce_two_level"], "a_hm") == 1 and E.radius(BY_ID["wgrad_reduce_two_level"], "h") == 4
    assert all(E.radius(c, f) for c in CASES for f in E.FAMILIES)


RUNS = [(c, f) for c in CASES for f in E.families(c)]


@pytest.mark.parametrize("case,family", RUNS, ids=[f"{c.id}-{f}" for c, f in RUNS])
def test_the_exactness_condition_holds_on_every_row_and_family(case, family):
    row = E.reference(E.operands(case, family))     # asserts the condition and that the reference is an fp32 value
    assert 0 < row.condition < E.LIMIT
    assert row.want.dtype == np.float32 and np.all(np.isfinite(row.want))
    r = E.radius(case, family)
    for v, wide in ((row.a, family == "a_hm"), (row.b, family == "b_hm")):
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() == (257 * r if wide else r), (case.id, family)
    assert np.all(row.t0 % 4 == 0) if case.st else np.all(row.t0 == E.STALE)
    if row.mask is not None:
        assert {-1.0, 0.0, 1.0} <= set(np.sign(row.mask).reshape(-1)[:4096])
    if case.relu or row.mask is not None:
        assert (row.want == 0).any() and (row.want != 0).any()


@pytest.mark.parametrize("family", E.FAMILIES)
@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_float64_reference_equals_the_fp32_oracle_on_the_integer_families(case, family):
    row = E.operands(case, family)
    g = row.g
    acc = E.product64(case, g, row.a, row.b)
    if case.op.startswith("local"):
        ref = {"local_up": L.up, "local_down": L.down, "local_outp": L.outp}[case.op](g, row.a, row.b)
    elif case.op.startswith("fc"):
        ta, tb = {"fc_nt": (False, True), "fc_nn": (False, False), "fc_tn": (True, False)}[case.op]
        ref = oracle.port.dot(row.a, row.b, np.zeros(acc.shape, np.float32), 0.0, 1.0, ta, tb)
    else:
        ref = {"fprop": oracle.port.conv_up, "dgrad": oracle.port.conv_down, "wgrad": oracle.port.conv_outp}[case.op](g, row.a, row.b)
    assert np.array_equal(acc, np.asarray(ref, np.float64).reshape(acc.shape))
    # and with the row's own epilogue where the oracle has it (scaleTargets, scaleOutput)
    if case.op in ("wgrad", "fc_nt", "fc_nn", "fc_tn") and row.bias is None and row.mask is None:
        want = E.epilogue64(case, acc, row.t0)
        t = row.t0.copy()
        if case.op == "wgrad":
            got = oracle.port.conv_outp(g, row.a, row.b, t, case.st, case.so)
        else:
            got = oracle.port.dot(row.a, row.b, t, case.st, case.so, ta, tb)
        assert np.array_equal(want, got.astype(np.float64))


def test_hm_families_have_nonzero_h_and_m_planes_and_a_zero_l_plane():
    for cid in ("fwd_ggp_r128", "wgrad_reduce_two_level", "wgrad_bias_fallback", "fc_nn_r96"):
        for family, pick in (("a_hm", "a"), ("b_hm", "b")):
            row = E.operands(BY_ID[cid], family)
            for name in ("a", "b"):
                v = getattr(row, name)
                h, m, l = E.split3(v)
                assert np.array_equal(h.astype(np.float64) + m + l, v) and not l.any(), (cid, family, name)
                assert h.any()
                assert m.any() == (name == pick), (cid, family, name, "only the wide operand has an m plane")
    # the restatement itself: ties to even, and a value that needs all three planes
    assert E.bf16_rne(np.float32(257.0)) == 256.0 and E.bf16_rne(np.float32(259.0)) == 260.0 and E.bf16_rne(np.float32(-770.0)) == -768.0
    h, m, l = E.split3(np.float32(1.0 + 2.0 ** -9 + 2.0 ** -18))
    assert (h, m, l) == (1.0, 2.0 ** -9, 2.0 ** -18)


def test_guard_checker_finds_a_planted_overrun_and_a_planted_outside_read():
    rng = np.random.default_rng(3)
    a = rng.integers(-4, 5, 24).astype(np.float32)
    for lead in (1, 2, 20):
        # a target: an intact buffer passes, a store one float behind / before the tensor is found, also one that stores 7.0's neighbour
        buf = E.guarded(a, lead, E.TAIL, E.TARGET_GUARD)
        assert buf.size == lead + a.size + E.TAIL and E.damaged(buf, lead, a.size, E.TARGET_GUARD) == []
        over = buf.copy()
        over[lead + a.size] = 0.0
        over[lead - 1] = -7.0
        over[-1] = np.nan
        assert E.damaged(over, lead, a.size, E.TARGET_GUARD) == [-1, a.size, a.size + E.TAIL - 1]
        inside = buf.copy()
        inside[lead] += 1
        assert E.damaged(inside, lead, a.size, E.TARGET_GUARD) == [] and E.first_mismatch(inside[lead:lead + a.size], a)[:2] == (1, (0,))
        # a source: a kernel stand-in that reads one float too many under a zero weight poisons its exact output
        src = E.guarded(a, lead, E.TAIL, np.nan)
        assert E.damaged(src, lead, a.size, np.nan) == []
        w = np.ones(a.size + 1, np.float32)
        w[-1] = 0.0
        good = np.float32(np.dot(src[lead:lead + a.size], w[:-1]))
        outside = np.float32(np.dot(src[lead:lead + a.size + 1], w))
        assert E.first_mismatch([good], [a.sum()]) is None and E.first_mismatch([outside], [a.sum()]) is not None
        written = src.copy()
        written[lead - 1] = 0.0
        assert E.damaged(written, lead, a.size, np.nan) == [-1]
    # bit equality, not value equality: -0.0 is not 0.0, and a NaN equals only the same NaN
    assert E.first_mismatch([0.0], [-0.0]) is not None and E.first_mismatch([np.nan], [np.nan]) is None
