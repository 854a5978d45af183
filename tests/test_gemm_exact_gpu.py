"""Every GEMM kernel build, bit for bit over the whole tensor, on guarded views of its operands (tests/gemm_exact.py has the data, the
float64 reference, the exactness condition and the operand factory; tests/split_cases.py the rows).

Each row of split_cases.CASES x operand family (h, a_hm, b_hm; gemm_exact.families says which rows run h only) x layout x matrix
path (1 = bf16 split, 0 = fp32 instruction):

  aligned           every operand a view whose base is 16-byte aligned and no more (leads of 36, 20 and 12 floats).  The whole target, and
                    the bias gradient where the entry has one, bit-equal to the reference; the 7.0 guards around the targets intact;
                    the sources and their NaN guards unwritten; on the split path every timer name of the row present, so a view
                    selects the build a whole matrix selects; on the rows pinned to the fp32 instruction no split build of that family.
  params_unaligned  activations and derivatives as above; banks, bank gradients, biases, bias gradients and masks one float into their
                    allocation (4-byte aligned only), once more two floats in (8-byte aligned), and once with the bank and its gradient
                    aligned and only biases, bias gradients and masks one float in (an edge's slices of the package's flat
                    buffers).  Bit-equality and intact guards.
                    The dispatch may take another build there: the names that ran are in profiles/gemm_exact_views.txt
                    (python tests/gemm_exact.py rewrites it), not asserted.

Every call runs twice on fresh operands and must give the same bits.  Nothing is sampled and there is no tolerance: any tiling, split-K
plan or summation order of a correct kernel gives these bits (gemm_exact.py: the exactness condition, asserted per row and family)."""
import numpy as np
import pytest

import gemm_exact as E
import split_cases
from split_cases import CASES

pytestmark = pytest.mark.gpu

LAYOUTS = {"aligned": (E.ALIGNED,), "params_unaligned": E.UNALIGNED}
ROWS = [(c, f, l, p) for c in CASES for f in E.families(c) for l in LAYOUTS for p in (1, 0)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return True


def _exact(row, leads, path):
    """one call of the row on guarded views: its timer names, after the bit-for-bit, guard and source checks"""
    ops = E.Guarded(leads)
    out, db, names = E.run(row, ops, path)          # Guarded.read has checked the targets' guards
    tag = (row.case.id, row.family, leads, "split" if path else "fp32", sorted(names))
    bad = E.first_mismatch(out, row.want)
    assert bad is None, tag + ("(differing elements, first index, got, want)", bad)
    if row.want_db is not None:
        bad = E.first_mismatch(db, row.want_db)
        assert bad is None, tag + ("bias gradient: (differing elements, first index, got, want)", bad)
    assert ops.sources_intact(), tag + ("a source operand or its guard was written",)
    return out, db, names


@pytest.mark.parametrize("case,family,layout,path", ROWS, ids=[f"{c.id}-{f}-{l}-{'split' if p else 'fp32'}" for c, f, l, p in ROWS])
def test_every_gemm_build_is_bit_exact_on_guarded_views(gpu, case, family, layout, path):
    row = E.row(case, family)
    assert row.condition < E.LIMIT
    for i, leads in enumerate(LAYOUTS[layout]):
        out, db, names = _exact(row, leads, path)
        if i == 0:
            out2, db2, _ = _exact(row, leads, path)
            assert np.array_equal(E.bits(out), E.bits(out2)) and (db is None or np.array_equal(E.bits(db), E.bits(db2)))
        if layout == "aligned":
            fam = split_cases.family(case.expect[0])
            if path == 1:
                missing = [n for n in case.expect if n not in names]
                assert not missing, (case.id, "a view selects another build than a whole matrix", missing, sorted(names))
            if case.fp32:
                assert not any(",split" in n for n in names if split_cases.family(n) == fam), sorted(names)
