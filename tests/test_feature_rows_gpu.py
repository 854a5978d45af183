"""GPU: feature_rows (include/convnet_hip.h, csrc/feature_rows.hip) through the C ABI.

N (cases) in {1, 3, 4, 33, 65} x D (dims) in {1, 10, 63, 64, 65, 1000, 4099}: one element, tails that are no multiple of 4, the 64-wide
tile's edges on either side, more than one tile both ways.  Every operand is a get_slice view of a flat buffer between guard floats of
7.0, once from float 0 (16-byte base: the 16-byte loads along N when N % 4 == 0, the 16-byte stores along D when D % 4 == 0) and once
from float 1 (a base that is 4-byte aligned only: the scalar paths at the same shapes).

 * passes = 1, group = 1: the numpy transpose, bit for bit; rows behind ``cases`` keep their sentinel.
 * passes in {2, 10}, group = 1: the device's own add_elementwise into a zeroed matrix x passes, then divide_by_scalar, bit for bit.
 * group in {2, 3, 5, N, N + 1, 2N + 1}, three consecutive calls: row count and carry as the restatement (tests/datawriter_ref.py) says,
   every value within (passes + group + 2) * 2^-24 * sum|x| / (passes * group) of its float64 result — the first-order bound of ANY
   summation order of those terms (passes - 1 additions, the division, group additions, the product by and the rounding of 1 / group),
   so it cannot excuse a wrong order or a wrong member.  N(0, 1) inputs, and a 1e8 entry beside them.
 * every case twice: the same bits."""
import numpy as np
import pytest

from datawriter_ref import DataWriterRef

pytestmark = pytest.mark.gpu

NS, DS = [1, 3, 4, 33, 65], [1, 10, 63, 64, 65, 1000, 4099]
SHAPES = [(n, d) for n in NS for d in DS]
IDS = [f"N{n}-D{d}" for n, d in SHAPES]
SENTINEL, GUARD = 3.25, 7.0
ERR_DIMS, ERR_TRANSPOSED = -1, -5
U = 2.0 ** -24


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


class View:
    """A (rows, cols) device matrix that is a get_slice view of a flat buffer, ``lead`` guard floats in front and 5 behind."""

    def __init__(self, M, a, rows, cols, lead):
        a = np.asarray(a, np.float32).reshape(-1)
        assert a.size == rows * cols
        self.full, self.m, self.lead, self.n = M(), M(), lead, a.size
        self.full.AllocateGPUMemory(1, lead + a.size + 5)
        self.full.FromNumpy(np.concatenate([np.full(lead, GUARD, np.float32), a, np.full(5, GUARD, np.float32)]))
        self.full.GetSlice(self.m, lead, lead + a.size)
        self.m.Reshape(rows, cols)

    @property
    def mat(self):
        return self.m.GetMat()

    def get(self):
        x = self.full.ToNumpy().reshape(-1)
        assert np.all(x[:self.lead] == GUARD) and np.all(x[self.lead + self.n:] == GUARD), "guard floats overwritten"
        return x[self.lead:self.lead + self.n].copy()


def states(N, D, count, seed, huge=False):
    """``count`` states as numpy (D, N): the memory of an (N, D) case-fastest matrix."""
    x = np.random.default_rng([23, N, D, seed]).standard_normal((count, D, N)).astype(np.float32)
    if huge:
        x[count // 2, D // 2, N // 2] = 1e8
    return x


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def call(lib, state, sum_, p, passes, cases, carry, consumed, group, rows):
    return lib.feature_rows(state.mat, sum_.mat if sum_ is not None else None, p, passes, cases, carry.mat if carry is not None else None,
                            consumed, group, rows.mat)


@pytest.mark.parametrize("N,D", SHAPES, ids=IDS)
def test_one_pass_is_the_exact_transpose(M, lib, N, D):
    x = states(N, D, 1, 0)[0]
    for lead in (0, 1):
        for cases in sorted({N, max(1, N - 2), 1}):
            outs = []
            for _ in range(2):
                s, rows = View(M, x, N, D, lead), View(M, np.full(D * N, SENTINEL), D, N, lead)
                assert call(lib, s, None, 0, 1, cases, None, 0, 1, rows) == 0
                outs.append(rows.get().reshape(N, D))
                assert np.array_equal(bits(s.get()), bits(x))
            assert np.array_equal(bits(outs[0][:cases]), bits(x.T[:cases])), (lead, cases)
            assert np.all(outs[0][cases:] == SENTINEL), (lead, cases)
            assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("N,D", SHAPES, ids=IDS)
def test_averaged_passes_equal_the_device_add_and_divide(M, lib, N, D):
    for passes in (2, 10):
        xs = states(N, D, passes, passes)
        buf, m = M(), M()                                     # buf.Set(0); buf.Add(m) ...; buf.Divide(passes) (src/datawriter.cc:138-145)
        buf.AllocateGPUMemory(N, D)
        m.AllocateGPUMemory(N, D)
        buf.Set(0.0)
        partial = []
        for x in xs:
            m.FromNumpy(x)
            buf.Add(m)
            partial.append(buf.ToNumpy().reshape(D, N))
        buf.Divide(passes)
        want = buf.ToNumpy().reshape(D, N).T
        for lead in (0, 1):
            cases = N if lead == 0 else max(1, N - 1)
            outs = []
            for _ in range(2):
                sum_ = View(M, np.full(N * D, SENTINEL), N, D, lead)
                rows = View(M, np.full(D * N, SENTINEL), D, N, lead)
                for p, x in enumerate(xs):
                    assert call(lib, View(M, x, N, D, lead), sum_, p, passes, cases, None, 0, 1, rows) == 0
                    if p < passes - 1:                        # sum = the running sum, nothing else touched
                        assert np.array_equal(bits(sum_.get()), bits(partial[p])), (passes, lead, p)
                        assert np.all(rows.get() == SENTINEL)
                assert np.array_equal(bits(sum_.get()), bits(partial[passes - 2]))      # the last pass leaves the sum alone
                outs.append(rows.get().reshape(N, D))
            assert np.array_equal(outs[0][:cases], want[:cases]), (passes, lead)
            assert np.array_equal(bits(outs[0][:cases]), bits(want[:cases])), (passes, lead)
            assert np.all(outs[0][cases:] == SENTINEL)
            assert np.array_equal(bits(outs[0]), bits(outs[1]))


def run_groups(M, lib, xs, N, D, passes, group, lead, cases_of_call):
    """Three consecutive calls (of ``passes`` passes each) on one stream: [rows of each call], carry, consumed."""
    sum_ = View(M, np.zeros(N * D), N, D, lead) if passes > 1 else None
    carry = View(M, np.zeros(D), D, 1, lead)
    consumed, out = 0, []
    for c, cases in enumerate(cases_of_call):
        R = (consumed + cases) // group
        rows = View(M, np.full(D * (R + 1), SENTINEL), D, R + 1, lead)
        for p in range(passes):
            assert call(lib, View(M, xs[c * passes + p], N, D, lead), sum_, p, passes, cases, carry, consumed, group, rows) == 0
        got = rows.get().reshape(R + 1, D)
        assert np.all(got[R:] == SENTINEL), (c, "a row behind the emitted ones was written")
        out.append(got[:R])
        consumed = (consumed + cases) % group
    return np.concatenate(out, axis=0), carry.get(), consumed


@pytest.mark.parametrize("N,D", SHAPES, ids=IDS)
def test_groups_of_consecutive_cases_across_calls(M, lib, N, D):
    cases_of_call = [N, max(1, N - 1), N]
    for passes, huge in ((1, False), (2, True)):
        xs = states(N, D, 3 * passes, 7 + passes, huge)
        for group in sorted({2, 3, 5, N, N + 1, 2 * N + 1} - {1}):
            ref, ref_abs = (DataWriterRef({"f": (passes, group)}, 1 << 30) for _ in range(2))
            for c, cases in enumerate(cases_of_call):
                for p in range(passes):
                    x = xs[c * passes + p].T.astype(np.float64)[:cases]
                    ref.Write({"f": x}, cases)
                    ref_abs.Write({"f": np.abs(x)}, cases)
            want, scale = ref.Rows("f") if ref.streams_["f"].rows else np.zeros((0, D)), None
            s, sa = ref.streams_["f"], ref_abs.streams_["f"]
            scale = ref_abs.Rows("f") if sa.rows else np.zeros((0, D))            # sum|x| / (passes * group) of every value
            bound = (passes + group + 2) * U
            for lead in (0, 1):
                runs = [run_groups(M, lib, xs, N, D, passes, group, lead, cases_of_call) for _ in range(2)]
                got, carry, consumed = runs[0]
                assert got.shape == want.shape and consumed == s.consumed, (passes, group, lead, got.shape, want.shape)
                err = np.abs(got.astype(np.float64) - want)
                assert np.all(err <= bound * scale), (passes, group, lead, float((err / np.maximum(scale, 1e-300)).max() / U))
                want_carry = s.seq_buf if s.consumed else np.zeros(D)
                cerr = np.abs(carry.astype(np.float64) - want_carry)
                assert np.all(cerr <= bound * (sa.seq_buf if s.consumed else np.zeros(D))), (passes, group, lead, "carry")
                assert np.array_equal(bits(got), bits(runs[1][0])) and np.array_equal(bits(carry), bits(runs[1][1]))


def test_error_codes(M, lib):
    N, D = 4, 10
    x = states(N, D, 1, 0)[0]
    s, sum_, carry = View(M, x, N, D, 0), View(M, x, N, D, 0), View(M, np.zeros(D), D, 1, 0)
    rows = View(M, np.zeros(D * N), D, N, 0)
    assert call(lib, s, sum_, 1, 2, N, carry, 1, 2, rows) == 0
    assert call(lib, s, View(M, np.zeros(N * (D + 1)), N, D + 1, 0), 0, 2, N, None, 0, 1, rows) == ERR_DIMS       # sum is not state's shape
    assert call(lib, s, None, 0, 1, N, None, 0, 1, View(M, np.zeros((D + 1) * N), D + 1, N, 0)) == ERR_DIMS       # rows of another width
    assert call(lib, s, None, 0, 1, N, None, 0, 1, View(M, np.zeros(D * (N - 1)), D, N - 1, 0)) == ERR_DIMS       # too few rows
    assert call(lib, s, None, 0, 1, N + 1, None, 0, 1, rows) == ERR_DIMS                                           # more cases than the state holds
    assert call(lib, s, None, 0, 1, N, View(M, np.zeros(D + 1), D + 1, 1, 0), 0, 2, rows) == ERR_DIMS              # carry is not (D, 1)
    assert lib.feature_rows(s.m.GetMatTranspose(), None, 0, 1, N, None, 0, 1, rows.mat) == ERR_TRANSPOSED
    assert lib.feature_rows(s.mat, None, 0, 1, N, None, 0, 1, rows.m.GetMatTranspose()) == ERR_TRANSPOSED
    assert np.all(rows.get().reshape(N, D)[2:] == 0.0)                                                             # the refused calls wrote nothing
