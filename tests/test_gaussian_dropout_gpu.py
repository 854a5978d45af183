"""GPU: gaussian_dropout, gaussian_dropout_noise and gaussian_dropout_undo of include/convnet_hip.h through the C ABI, on generator
states of the test's own, against tests/gaussian_dropout_ref.py in float32 on the DEVICE's own normals (fill_with_randn) and, for the
logistic activation, the device's own apply_sigmoid — every comparison is bit for bit — and against the unfused entry sequence run
on a second generator state with the same seed.

Element counts: 1, 2, 3, 4, 5, 7, 1023 (heads, tails, less than one 16-byte group), 2^20 + 3 (the RNG tests' size) and 2^21 + 5 (one
grid pass is 2048 blocks x 256 lanes x 4 floats = 2^21: the grid-stride loop takes a second trip), each as a 16-byte aligned view
between guard floats of 7.0; and get_slice views of a 67-row matrix from columns 1, 2 and 3, which start 3, 2 and 1 floats past a
16-byte boundary: there the RNG's groups of four (counted from the view's first element) and the kernel's 16-byte groups differ."""
import ctypes

import numpy as np
import pytest

import gaussian_dropout_ref as ref
from test_logistic_gpu import same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED, STDDEV = 1234, 0.5
GRID_PASS = 2048 * 256 * 4
# (rows, cols, guard columns in front): rows = 1 with 4 guard floats is 16-byte aligned; 67 rows from column c start 67 c floats in
CASES = [(1, n, 4) for n in (1, 2, 3, 4, 5, 7, 1023, (1 << 20) + 3, 2 * GRID_PASS // 2 + 5)] + [(67, 33, 1), (67, 33, 2), (67, 33, 3)]
IDS = [f"n{c}" if r == 1 else f"view67x{c}_from_col{g}" for r, c, g in CASES]
ERROR_DIMS, ERROR_GENERIC, ERROR_NOT_ON_DEVICE, ERROR_UNSUPPORTED = -1, -6, -8, -9
MARK = 3.25


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    from convnet_amd._lib import lib
    return lib


class Dev:
    """``a`` as a (rows, cols) device matrix: a get_slice view behind ``front`` guard columns of 7.0 and in front of one."""

    def __init__(self, a, rows, cols, front):
        from hip_adapter import _mat
        self.m, self.full = _mat(np.asarray(a, np.float32).reshape(-1), rows, cols, guard=(front, 1))
        self.rows, self.front = rows, front

    @property
    def mat(self):
        return self.m.GetMat()

    def offset(self):
        return (self.m.mat_.data_device % 16) // 4

    def get(self):
        x = self.full.ToNumpy().reshape(-1)
        lo = self.rows * self.front
        assert np.all(x[:lo] == 7.0) and np.all(x[-self.rows:] == 7.0), "guard floats overwritten"
        return x[lo:-self.rows].copy()


def state(lib, seed=SEED, advance=0):
    """a generator state of the test's own, its call counter at ``advance``"""
    from convnet_amd import _lib
    from hip_adapter import _mat
    st = _lib.rnd_struct()
    assert lib.init_random(ctypes.byref(st), seed) == 0
    one = _mat(np.zeros(1, f32), 1, 1)
    for _ in range(advance):
        assert lib.fill_with_rand(ctypes.byref(st), one.GetMat()) == 0
    return st


def counter_is(lib, st, count, seed=SEED):
    """The state's next uniform fill equals the one of a fresh state advanced to ``count``.  (Advances both by one.)"""
    from hip_adapter import _mat
    a, b = _mat(np.zeros(64, f32), 1, 64), _mat(np.zeros(64, f32), 1, 64)
    fresh = state(lib, seed, count)
    assert lib.fill_with_rand(ctypes.byref(st), a.GetMat()) == 0 and lib.fill_with_rand(ctypes.byref(fresh), b.GetMat()) == 0
    return np.array_equal(a.ToNumpy(), b.ToNumpy())


def inputs(rows, cols, seed, scale=3.0):
    return (np.random.default_rng([23, rows, cols, seed]).standard_normal(rows * cols) * scale).astype(f32)


def device_noise(lib, case, call_id, stddev=STDDEV):
    rows, cols, front = case
    T = Dev(np.full(rows * cols, MARK, f32), rows, cols, front)
    st = state(lib)
    assert lib.gaussian_dropout_noise(ctypes.byref(st), call_id, stddev, T.mat) == 0
    return T.get()


def test_the_views_start_where_the_cases_say(lib):
    for (rows, cols, front), want in zip(CASES[-4:], (0, 3, 2, 1)):
        assert Dev(np.zeros(rows * cols), rows, cols, front).offset() == want


# ---- 1. the noise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_noise_is_fill_with_randn_times_stddev_plus_one(lib, case):
    rows, cols, front = case
    c = 2
    Z = Dev(np.full(rows * cols, MARK, f32), rows, cols, front)
    assert lib.fill_with_randn(ctypes.byref(state(lib, advance=c)), Z.mat) == 0      # the normals of call c, on a view of the same offset
    T = Dev(np.full(rows * cols, MARK, f32), rows, cols, front)
    st = state(lib)                                                                   # counter 0: the call id is an argument
    assert lib.gaussian_dropout_noise(ctypes.byref(st), c, STDDEV, T.mat) == 0
    n = T.get()
    same_bits(n, ref.noise(Z.get(), STDDEV), "noise vs fill_with_randn * stddev + 1", case)
    assert lib.gaussian_dropout_noise(ctypes.byref(st), c, STDDEV, T.mat) == 0
    same_bits(T.get(), n, "noise, second call", case)
    assert counter_is(lib, st, 0), "gaussian_dropout_noise moved the call counter"
    if rows * cols > 4:
        assert not np.array_equal(device_noise(lib, case, c + 1), n)


# ---- 2. forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_act", [-1.0, 2.0], ids=["noclip", "clip2"])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_equals_the_reference_and_the_unfused_sequence(lib, case, act, max_act):
    rows, cols, front = case
    x = inputs(rows, cols, act)
    c = 1
    fused_st, plain_st = state(lib, advance=c), state(lib, advance=c)
    F, U, N = (Dev(x, rows, cols, front) for _ in range(3))
    call_id = ctypes.c_ulonglong(99)
    assert lib.gaussian_dropout(ctypes.byref(fused_st), F.mat, STDDEV, max_act, act, ctypes.byref(call_id)) == 0
    assert call_id.value == c                                       # the counter before the call ...
    # the unfused sequence, src/layer.cc:369-377 behind the activation entry
    if act == 1:
        assert lib.lower_bound_scalar(U.mat, 0.0, U.mat) == 0
    if act == 2:
        assert lib.apply_sigmoid(U.mat, U.mat) == 0
    activated = U.get()
    assert lib.fill_with_randn(ctypes.byref(plain_st), N.mat) == 0
    assert lib.mult_by_scalar(N.mat, STDDEV, N.mat, 0.0) == 0 and lib.add_scalar(N.mat, 1.0, N.mat) == 0
    assert lib.mult_elementwise(U.mat, N.mat, U.mat, 0.0) == 0
    if max_act > 0:
        assert lib.upper_bound_mod_scalar(U.mat, max_act, U.mat) == 0
    got = F.get()
    same_bits(got, U.get(), "gaussian_dropout vs the unfused sequence", case, act, max_act)
    noise = device_noise(lib, case, c)
    same_bits(noise, N.get(), "gaussian_dropout_noise vs the sequence's noise matrix", case)
    # numpy fp32 on the device's noise; the logistic case on the device's own sigmoid
    want = ref.forward(activated, noise, 0, max_act) if act == 2 else ref.forward(x, noise, act, max_act)
    same_bits(got, want, "gaussian_dropout vs numpy fp32", case, act, max_act)
    if max_act > 0 and act == 0 and rows * cols > 1000:
        assert got.max() == f32(max_act) and got.min() == -f32(max_act)      # both clips were reached
    assert counter_is(lib, fused_st, c + 1), "gaussian_dropout must advance the counter once"      # ... and one higher after
    assert counter_is(lib, plain_st, c + 1)


def test_forward_takes_a_null_call_id(lib):
    rows, cols, front = 1, 1023, 4
    x = inputs(rows, cols, 5)
    st = state(lib, advance=3)
    F = Dev(x, rows, cols, front)
    assert lib.gaussian_dropout(ctypes.byref(st), F.mat, STDDEV, -1.0, 0, None) == 0
    same_bits(F.get(), ref.forward(x, device_noise(lib, (rows, cols, front), 3), 0), "NULL call_id")
    assert counter_is(lib, st, 4)


# ---- 3. undo ----------------------------------------------------------------------------------------------------------------------------
def _undo_case(lib, dcase, scase, act, restore):
    rows, cols, _ = dcase
    c = 5
    noise = device_noise(lib, dcase, c)
    assert not (noise == 0).any(), "premise: the drawn noise holds no exact 0 (about 2^-24 per element; the seed is fixed)"
    d, s = inputs(rows, cols, 7, 1.0), inputs(rows, cols, 8, 2.0)
    if act == 2:
        s = (ref.activation(s, 2) * noise).astype(f32)               # a logistic layer's state: sigmoid times the noise
    D, S = Dev(d, *dcase), Dev(s, *scase)
    st = state(lib, advance=1)
    assert lib.gaussian_dropout_undo(ctypes.byref(st), c, STDDEV, D.mat, S.mat, act, restore) == 0
    want_d, want_s = ref.backward(d, s, noise, act)
    same_bits(D.get(), want_d, "derivative", dcase, scase, act, restore)
    same_bits(S.get(), want_s if restore else s, "state", dcase, scase, act, restore)
    assert counter_is(lib, st, 1), "gaussian_dropout_undo moved the call counter"
    return noise


@pytest.mark.parametrize("restore", [0, 1])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_undo_equals_the_reference(lib, case, act, restore):
    noise = _undo_case(lib, case, case, act, restore)
    if noise.size > 1000:
        assert (noise < 0).any()                 # stddev 0.5: a 2.3 % share of the noise is negative, the ReLU' sees restored states


@pytest.mark.parametrize("act", [1, 2])
def test_undo_on_operands_that_disagree_in_alignment(lib, act):
    """derivative and state 3 and 2 floats past a 16-byte boundary: no common 16-byte grouping, the kernel goes four bytes at a time"""
    _undo_case(lib, (67, 33, 1), (67, 33, 2), act, 1)
    _undo_case(lib, (1, 1023, 4), (1, 1023, 3), act, 0)


def test_undo_equals_the_unfused_backward_sequence(lib):
    rows, cols, front = 67, 33, 1
    c = 4
    d, s = inputs(rows, cols, 1, 1.0), inputs(rows, cols, 2, 2.0)
    for act, entry in ((1, lib.apply_rectified_linear_deriv), (2, lib.apply_logistic_deriv)):
        D, S, D2, S2, N = (Dev(a, rows, cols, front) for a in (d, s, d, s, d))
        st = state(lib)
        assert lib.gaussian_dropout_undo(ctypes.byref(st), c, STDDEV, D.mat, S.mat, act, 1) == 0
        assert lib.gaussian_dropout_noise(ctypes.byref(st), c, STDDEV, N.mat) == 0
        assert lib.mult_elementwise(D2.mat, N.mat, D2.mat, 0.0) == 0 and lib.divide_elementwise(S2.mat, N.mat, S2.mat) == 0
        assert entry(D2.mat, S2.mat, D2.mat) == 0
        same_bits(D.get(), D2.get(), "undo vs Mult, Divide, activation'", act)
        same_bits(S.get(), S2.get(), "restored state vs Divide", act)


# ---- 4. statistics ----------------------------------------------------------------------------------------------------------------------
def test_noise_statistics(lib):
    n = (1 << 20) + 3
    a, b = (device_noise(lib, (1, n, 4), c).astype(np.float64) for c in (0, 1))
    assert abs(a.mean() - 1) < 6 * 0.5 / np.sqrt(n)
    assert abs(a.var() - 0.25) < 6 * 0.25 * np.sqrt(2 / n)
    assert not np.array_equal(a, b)
    assert abs(np.corrcoef(a, b)[0, 1]) < 6 / np.sqrt(n)


# ---- 5. error codes ---------------------------------------------------------------------------------------------------------------------
def test_error_codes_launch_nothing_and_leave_the_counter(lib):
    from convnet_amd import _lib
    st = state(lib, advance=2)
    A, B, C = Dev(np.full(15, MARK, f32), 3, 5, 1), Dev(np.full(15, MARK, f32), 3, 5, 1), Dev(np.full(15, MARK, f32), 5, 3, 1)
    blank = _lib.rnd_struct()                                          # never initialised: no {seed, counter} behind it
    host = _lib.cudamat()
    ctypes.memmove(ctypes.byref(host), ctypes.byref(A.m.mat_), ctypes.sizeof(_lib.cudamat))
    host.on_device = 0
    huge = _lib.cudamat()                                              # 2^31 floats (nothing is launched, so nothing is touched)
    ctypes.memmove(ctypes.byref(huge), ctypes.byref(A.m.mat_), ctypes.sizeof(_lib.cudamat))
    huge.size[0], huge.size[1] = 1 << 16, 1 << 15
    R, H, G = ctypes.byref(st), ctypes.byref(host), ctypes.byref(huge)
    call_id = ctypes.c_ulonglong(77)
    for rnd, code in ((None, ERROR_GENERIC), (ctypes.byref(blank), ERROR_GENERIC)):
        assert lib.gaussian_dropout(rnd, A.mat, 0.5, -1.0, 0, ctypes.byref(call_id)) == code
        assert lib.gaussian_dropout_noise(rnd, 0, 0.5, A.mat) == code
        assert lib.gaussian_dropout_undo(rnd, 0, 0.5, A.mat, B.mat, 0, 1) == code
    assert lib.gaussian_dropout(R, H, 0.5, -1.0, 0, ctypes.byref(call_id)) == ERROR_NOT_ON_DEVICE
    assert lib.gaussian_dropout_noise(R, 0, 0.5, H) == ERROR_NOT_ON_DEVICE
    assert lib.gaussian_dropout_undo(R, 0, 0.5, H, B.mat, 0, 1) == ERROR_NOT_ON_DEVICE
    assert lib.gaussian_dropout_undo(R, 0, 0.5, A.mat, H, 0, 1) == ERROR_NOT_ON_DEVICE
    assert lib.gaussian_dropout_undo(R, 0, 0.5, A.mat, C.mat, 0, 1) == ERROR_DIMS                  # (3, 5) against (5, 3)
    for act in (-1, 3):
        assert lib.gaussian_dropout(R, A.mat, 0.5, -1.0, act, ctypes.byref(call_id)) == ERROR_UNSUPPORTED
        assert lib.gaussian_dropout_undo(R, 0, 0.5, A.mat, B.mat, act, 1) == ERROR_UNSUPPORTED
    assert lib.gaussian_dropout(R, G, 0.5, -1.0, 0, ctypes.byref(call_id)) == ERROR_UNSUPPORTED
    assert lib.gaussian_dropout_noise(R, 0, 0.5, G) == ERROR_UNSUPPORTED
    assert lib.gaussian_dropout_undo(R, 0, 0.5, G, G, 0, 1) == ERROR_UNSUPPORTED
    assert call_id.value == 77
    for m in (A, B, C):
        assert np.all(m.get() == MARK)
    assert counter_is(lib, st, 2), "an error moved the call counter"
