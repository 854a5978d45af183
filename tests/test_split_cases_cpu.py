"""The table of split-build precision rows (tests/split_cases.py) stays complete and well formed — no GPU.

* Every kernel family that has a bf16-split build in convnet_amd/csrc/*.hip (a timer name carrying ",split", or local_conv.hip's
  names[] table) has a row that expects one of its split builds, or an exemption with a reason.  A family added later without a
  precision row fails here.
* Every conv row's shape passes the checks conv_geo makes (gather_gemm.hip; local_geo for the local rows), so a row cannot be a shape
  the library refuses."""
import os
import re

import split_cases
from split_cases import CASES, EXEMPT, FAMILIES

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "convnet_amd", "csrc")


def _key(name):
    """family of a timer name; gg_kernel counts as two families, its r-contiguous (rc) and k-contiguous (kc) builds"""
    fam = split_cases.family(name)
    if fam == "gg_kernel":
        return "gg_kernel kc" if ",kc" in name else "gg_kernel rc"
    return fam


def split_families():
    """kernel families with a split build, read from the sources"""
    found = set()
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith(".hip"):
            continue
        src = open(os.path.join(CSRC, f)).read()
        literals = re.findall(r'"((?:\w+)_kernel<[^"]*)"', src)
        for lit in literals:                 # whole timer names: "gfc_kernel<96x128,split>", names[] of local_conv.hip
            if ",split" in lit:
                found.add(_key(lit))
        if '",split>"' in src:               # names built from a prefix and the ",split>" suffix (gather_gemm.hip's launchers)
            for lit in literals:
                if lit.endswith("<"):
                    fam = lit[:-1]
                    if fam == "gg_kernel" and '"kc" : "rc"' in src:
                        found.update({"gg_kernel rc", "gg_kernel kc"})
                    else:
                        found.add(fam)
    return found


def test_the_source_scan_finds_the_known_split_families():
    fams = split_families()
    assert {f.split()[0] for f in fams} >= set(FAMILIES), sorted(fams)
    assert {"gg_kernel rc", "gg_kernel kc"} <= fams


def test_every_split_family_has_a_precision_row_or_an_exemption():
    covered = {_key(n) for c in CASES if not c.fp32 for n in c.expect if ",split" in n}
    missing = sorted(f for f in split_families() if f not in covered and f not in EXEMPT)
    assert not missing, f"kernel families with a split build and no row in tests/split_cases.py: {missing}"
    for fam, reason in EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4, (fam, "an exemption states its reason")


def test_rows_are_well_formed():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)), "row ids are unique"
    entries = {"convUp", "convUpBiasAct", "convDown", "convDownMask", "convOutpGemm", "convOutpBias", "dot", "dotBiasAct", "dotMask",
               "localUp", "localUpBiasAct", "localDown", "localOutp"}
    for c in CASES:
        assert c.entry in entries, c.id
        assert c.expect, (c.id, "a row names the kernels it must run")
        main = c.expect[0]
        assert (",split" in main) != c.fp32, (c.id, "a split row expects a split build; an fp32 row pins a build without one")
        assert c.patch_mode in (-1, 0, 1, 2, 3, 4) and c.wgrad_tile in (-1, 0, 1), c.id
        assert c.axis, (c.id, "the cancellation family needs the axis the row reduces over")
        if c.entry.startswith("dot"):
            assert c.trans in ("NT", "NN", "TN") and len(c.shape) == 3 and min(c.shape) >= 1, c.id
            if c.entry != "dot":
                assert c.trans != "TN", (c.id, "dotBiasAct / dotMask refuse the TN shape")
        if c.relu or c.entry in ("convUpBiasAct", "dotBiasAct", "localUpBiasAct"):
            assert c.direction == "fwd", c.id
    # the rows the issue asks for by name
    names = {n for c in CASES for n in c.expect}
    for n in ("gfc_kernel<96x128,split>", "ggp_kernel<1,4,3,64,split,pre>", "ggp_kernel<2,2,2,128,split,pre>", "ggp_kernel<2,2,1,128,split,pre>",
              "gg_kernel<1,4,1,128,rc,split>", "gpw_kernel<128x512,split,raw>", "gg_tail_fix_kernel", "gg_reduce_kernel", "wg_reduce_kernel",
              "gpv_kernel<96x512,split,raw>", "gpv_kernel<128x512,split,raw>", "gpp_kernel<2,2,2,128,split,raw>",
              "gpp_kernel<2,2,2,128,split,planes>", "wg_kernel<2,2,2,2,split>", "wg_kernel<2,2,5,3,x16,split>", "wg_kernel<4,1,1,3,split>",
              "wg_kernel<4,1,1,2,split>", "wg_kernel<4,1,1,1,split>", "ggp_kernel<2,2,2,128,split>", "gg_kernel<4,1,1,64,rc,split>",
              "gg_kernel<2,2,2,128,kc,split>", "gg_kernel<1,4,3,64,kc,split>", "gg_kernel<2,2,1,128,kc,split>", "gg_kernel<1,4,1,128,kc,split>",
              "gg_kernel<4,1,1,64,kc,split>", "lc_kernel<up,split>", "lc_kernel<down,split>", "lc_kernel<outp,split>", "dot_generic_kernel"):
        assert n in names, n


def _conv_geo_ok(N, C, H, W, F, Ky, Kx, sy, sx, pad):
    """conv_geo's checks (gather_gemm.hip) for a shape the test builds consistently: the output size formula, positive sizes, and the
    32-bit element offsets of the activation tensors"""
    if min(N, C, H, W, F, Ky, Kx, sy, sx) < 1 or pad < 0:
        return False
    My, Mx = (H + 2 * pad - Ky) // sy + 1, (W + 2 * pad - Kx) // sx + 1
    return My >= 1 and Mx >= 1 and N * H * W * C < 2 ** 31 and N * My * Mx * F < 2 ** 31


def test_every_conv_and_local_row_is_a_shape_the_library_accepts():
    for c in CASES:
        if c.entry.startswith("dot"):
            continue
        assert len(c.shape) == 10 and _conv_geo_ok(*c.shape), (c.id, c.shape)
        N, C, H, W, F, Ky, Kx, sy, sx, pad = c.shape
        if c.entry.startswith("local"):
            My, Mx = (H + 2 * pad - Ky) // sy + 1, (W + 2 * pad - Kx) // sx + 1
            assert N * My * Mx * F < 2 ** 31 and F * My * Mx * C * Ky * Kx < 2 ** 31, c.id
        if c.fp32 and c.entry.startswith("conv"):
            assert N % 4 != 0, (c.id, "the non-vector gg_kernel runs only where N % 4 != 0")


def test_the_rows_reach_the_dispatch_branches_they_name():
    """the shape rules of the dispatch (gather_gemm.hip gg_run / wg_launch, fewc_conv.hip gfc_try) that the expected names rely on"""
    for c in CASES:
        main = c.expect[0]
        if main == "gfc_kernel<96x128,split>":
            N, C, H, W, F, Ky, Kx, sy, sx, pad = c.shape
            assert (C, Ky, Kx, sy, sx) == (3, 7, 7, 2, 2) and N % 32 == 0 and F % 8 == 0 and F <= 96 and c.st == 0, c.id
        if c.entry.startswith("conv") and main.startswith("ggp_kernel") and ",pre" in main:
            N, C, H, W, F, Ky, Kx, sy, sx, pad = c.shape
            R = F if c.op == "fprop" else C
            tile = "<2,2,2,128," if R > 96 else "<1,4,3,64," if R > 64 else "<2,2,1,128,"
            assert R > 32 and main.startswith("ggp_kernel" + tile), (c.id, "gg_run's row tile for R rows")
        if c.id == "dgrad_many_classes":
            assert c.shape[7] * c.shape[8] > 16, "more stride classes than kMaxClasses (gather_gemm.h)"
        if c.id == "wgrad_bias_fallback":
            N, C, H, W, F, Ky, Kx, sy, sx, pad = c.shape
            assert (C * Ky * Kx) % 128 == 0 and F == 128, "K fills the 128-row k tile: no spare row for the bias"
        if c.id == "wgrad_reduce_two_level":
            N, C, H, W, F, Ky, Kx, sy, sx, pad = c.shape
            My, Mx = (H + 2 * pad - Ky) // sy + 1, (W + 2 * pad - Kx) // sx + 1
            chunks = My * Mx * ((N + 31) // 32)
            splits = min(512 // 2, chunks // 16)
            assert splits > 64, "more than 64 splits: the two-level reduce"
