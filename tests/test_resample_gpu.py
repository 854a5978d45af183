"""GPU: UpSampleGemm, DownSampleGemm and RGBToYUV (include/convnet_hip.h; convnet_amd/csrc/resample.hip) through the C ABI, against the
restatements of tests/resample_ref.py.

Shapes: N in {1, 4, 5, 64, 130} (one lane, one whole quad, a ragged quad, a wave, more than one block with a ragged quad), images 1 x 1,
3 x 5 (not square) and 8 x 8, C in {1, 3, 5}, factor in {1 .. 5}: the compile-time builds 2, 3, 4 and the generic kernel on both sides of
them.  Every tensor sits between guard floats in one allocation (tests/test_pool_norm_gpu.py: Dev): "aligned" on a 16-byte base,
"misaligned" one float in, where only the scalar arm is legal.  After every call the library's report of what it launched is read.

 * upsample: bit for bit the restatement for scaleTargets 0, 1 and 0.75 (a product that rounds), NaN targets at 0;
 * downsample: bit for bit AvgPoolGemm with kernel = stride = factor on the same operands, and within (f*f + 1) * 2^-24 * mean|x| of
   float64 per element — f*f - 1 additions and one division, each rounding at most 2^-24 of sum|x| / (f*f) to first order, with slack;
 * colour transform: within 3 * 2^-24 * (|a R| + |b G| + |c B|) of float64 per element: two fused steps and one product."""
import ctypes

import numpy as np
import pytest

import resample_ref as ref
from hip_adapter import last_kernel
from test_pool_norm_gpu import Dev, lib, same, within  # noqa: F401  (lib: the module fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32

NS = (1, 4, 5, 64, 130)
IMAGES = ((1, 1), (3, 5), (8, 8))       # (H, W)
CHANNELS = (1, 3, 5)
FACTORS = (1, 2, 3, 4, 5)


def _data(shape, seed, scale_spread=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(f32)
    if scale_spread:
        x *= np.exp2(rng.integers(-6, 7, shape)).astype(f32)
    return x


def _kernel(entry, f, vec):
    if entry == "downsample" and f == 2 and vec:
        return "pool_fwd_fixed_kernel<avg, 2, 2>"      # the one geometry the entry hands to the pool code (csrc/resample.hip: downsample)
    build = str(f) if f in (2, 3, 4) else "generic"
    return f"{entry}_kernel<{build}>/{'vec' if vec else 'scalar'}"


def _cases():
    for H, W in IMAGES:
        for C in CHANNELS:
            yield H, W, C


def _up(lib, X, T, f, st):
    lib.UpSampleGemm(X.mat, T.mat, X.s4, T.s4, f, st)


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("N", NS)
def test_upsample_equals_the_restatement_bit_for_bit(lib, N, f, mis):
    for H, W, C in _cases():
        x = _data((C, H, W, N), 1000 * N + 10 * f + C, scale_spread=True)
        t0 = _data((C, H * f, W * f, N), 77 + N + f)
        X = Dev(x, mis)
        for st in (0.0, 1.0, 0.75):
            T = Dev(t0, mis)
            _up(lib, X, T, f, st)
            assert last_kernel()[0] == _kernel("upsample", f, N % 4 == 0 and not mis)
            same(T.get().view(np.uint32), ref.upsample(x, f, t0, f32(st)).view(np.uint32), "upsample", (N, H, W, C, f, st))
        # scaleTargets 0 does not read the target: NaNs in it do not survive
        T = Dev(np.full((C, H * f, W * f, N), np.nan), mis)
        _up(lib, X, T, f, 0.0)
        same(T.get().view(np.uint32), ref.upsample(x, f).view(np.uint32), "upsample over NaN", (N, H, W, C, f))
        same(X.get(), x, "input")


def test_upsample_through_the_alias_and_twice_gives_the_same_bits(lib):
    x = _data((3, 3, 5, 130), 5)
    t0 = _data((3, 9, 15, 130), 6)
    X = Dev(x)
    runs = []
    for fn in (lib.UpSampleGemm, lib.UpSampleGemm, lib.UpSample):
        T = Dev(t0)
        fn(X.mat, T.mat, X.s4, T.s4, 3, 1.0)
        runs.append(T.get().copy())
    same(runs[0].view(np.uint32), runs[1].view(np.uint32), "run to run")
    same(runs[0].view(np.uint32), runs[2].view(np.uint32), "UpSample is UpSampleGemm")


def _avg_desc(C, f):
    from convnet_amd.matrix import make_conv_desc
    return make_conv_desc(C, C, f, f, f, f, 0, 0)


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("N", NS)
def test_downsample_equals_avg_pool_bit_for_bit_and_float64_within_the_bound(lib, N, f, mis):
    for H, W, C in _cases():
        x = _data((C, H * f, W * f, N), 2000 * N + 10 * f + C, scale_spread=True)
        X = Dev(x, mis)
        T, P = Dev(np.full((C, H, W, N), np.nan), mis), Dev(np.full((C, H, W, N), np.nan), mis)
        lib.DownSampleGemm(X.mat, T.mat, X.s4, T.s4, f)
        assert last_kernel()[0] == _kernel("downsample", f, N % 4 == 0 and not mis)
        lib.AvgPoolGemm(X.mat, P.mat, X.s4, P.s4, _avg_desc(C, f), 0.0, 1.0)
        got = T.get()
        same(got.view(np.uint32), P.get().view(np.uint32), "downsample vs AvgPoolGemm", (N, H, W, C, f))
        bound = (f * f + 1) * 2.0 ** -24 * ref.downsample64(np.abs(x), f)
        within(got, ref.downsample64(x, f), bound, "downsample", (N, H, W, C, f))
        same(X.get(), x, "input")


def test_downsample_through_the_alias_and_twice_gives_the_same_bits(lib):
    x = _data((5, 12, 20, 130), 8)
    X = Dev(x)
    runs = []
    for fn in (lib.DownSampleGemm, lib.DownSampleGemm, lib.DownSample):
        T = Dev(np.zeros((5, 3, 5, 130)))
        fn(X.mat, T.mat, X.s4, T.s4, 4)
        runs.append(T.get().copy())
    same(runs[0].view(np.uint32), runs[1].view(np.uint32), "run to run")
    same(runs[0].view(np.uint32), runs[2].view(np.uint32), "DownSample is DownSampleGemm")


class Flat:
    """a (N, cols) matrix between guard floats, without a Shape4D"""

    def __init__(self, a, N, mis=False):
        from hip_adapter import _mat
        a = np.asarray(a, f32)
        self.g = 1 if mis else 4
        self.m, self.full = _mat(a.reshape(-1), 1, a.size, guard=(self.g, self.g))
        self.m.Reshape(N, a.size // N)
        self.shape = a.shape

    @property
    def mat(self):
        return self.m.GetMat()

    def get(self):
        x = self.full.ToNumpy().reshape(-1)
        assert np.all(x[:self.g] == 7.0) and np.all(x[-self.g:] == 7.0), "guard floats overwritten"
        return x[self.g:-self.g].reshape(self.shape)


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("N", NS)
def test_rgb_to_yuv_is_within_the_bound_of_float64(lib, N, mis):
    for H, W in IMAGES + ((16, 16),):
        x = _data((3, H, W, N), 31 * N + H, scale_spread=True)
        X, T = Flat(x, N, mis), Flat(np.full(x.shape, np.nan), N, mis)
        lib.RGBToYUV(X.mat, T.mat)
        assert last_kernel()[0] == f"rgb_to_yuv_kernel/{'vec' if (H * W * N) % 4 == 0 and not mis else 'scalar'}"
        exact, mag = ref.rgb_to_yuv64(x)
        first = T.get().copy()
        within(first, exact, 3 * 2.0 ** -24 * mag, "rgb to yuv", (N, H, W))
        same(X.get(), x, "input")
        lib.RGBToYUV(X.mat, T.mat)
        same(T.get().view(np.uint32), first.view(np.uint32), "run to run")
        lib.RGBToYUV(X.mat, X.mat)            # in place
        same(X.get().view(np.uint32), first.view(np.uint32), "in place")


def test_rgb_to_yuv_maps_grey_to_luma_alone_within_the_bound(lib):
    """R = G = B = v: Y = v (the row sums to 1), U = V = 0 up to the bound — the rows of the reference, not some other YUV matrix."""
    v = np.linspace(-2, 2, 3 * 7 * 4, dtype=f32).reshape(1, 3, 7, 4)
    x = np.concatenate([v, v, v])
    X, T = Flat(x, 4), Flat(np.zeros(x.shape), 4)
    lib.RGBToYUV(X.mat, T.mat)
    exact, mag = ref.rgb_to_yuv64(x)
    within(T.get(), exact, 3 * 2.0 ** -24 * mag, "grey")
    assert np.allclose(T.get()[0], v[0], atol=1e-6) and np.abs(T.get()[1:]).max() < 1e-6


# ---- views ----------------------------------------------------------------------------------------------------------------------------
def test_channel_views_of_a_layer_at_odd_batch_are_served_and_their_neighbours_left_alone(lib):
    """get_slice channel views as Layer.SetupSlices cuts them: channels [1, 3) of a 4-channel layer at N = 5 start 75 (coarse) and 675
    (fine) floats in: bases that are 4-byte aligned only."""
    from convnet_amd.matrix import Matrix
    N, H, W, f = 5, 3, 5, 3
    small, large = _data((4, H, W, N), 1), _data((4, H * f, W * f, N), 2)
    S, L = Dev(small), Dev(large)

    def view(dev, h, w):
        v = Matrix()
        dev.m.GetSlice(v, h * w * 1, h * w * 3)
        v.SetShape4D(N, w, h, 2)
        assert v.mat_.data_device % 16 != 0 and v.mat_.data_device % 4 == 0
        return v
    sv, lv = view(S, H, W), view(L, H * f, W * f)
    lib.UpSampleGemm(sv.GetMat(), lv.GetMat(), ctypes.byref(sv.shape_), ctypes.byref(lv.shape_), f, 1.0)
    assert last_kernel()[0] == "upsample_kernel<3>/scalar"
    want = large.copy()
    want[1:3] = ref.upsample(small[1:3], f, large[1:3], 1.0)
    same(L.get().view(np.uint32), want.view(np.uint32), "upsample on views")
    lib.DownSampleGemm(lv.GetMat(), sv.GetMat(), ctypes.byref(lv.shape_), ctypes.byref(sv.shape_), f)
    assert last_kernel()[0] == "downsample_kernel<3>/scalar"
    got = S.get()
    same(got[[0, 3]], small[[0, 3]], "channels outside the view")
    within(got[1:3], ref.downsample64(want[1:3], f), (f * f + 1) * 2.0 ** -24 * ref.downsample64(np.abs(want[1:3]), f), "downsample on views")
    # the colour transform on a 3-channel view of a 5-channel layer
    x = _data((5, H, W, N), 3)
    Xd, Td = Dev(x), Dev(np.zeros((5, H, W, N)))
    xv, tv = Matrix(), Matrix()
    Xd.m.GetSlice(xv, H * W, 4 * H * W)
    Td.m.GetSlice(tv, H * W, 4 * H * W)
    assert xv.mat_.data_device % 16 != 0
    lib.RGBToYUV(xv.GetMat(), tv.GetMat())
    assert last_kernel()[0] == "rgb_to_yuv_kernel/scalar"
    exact, mag = ref.rgb_to_yuv64(x[1:4])
    got = Td.get()
    within(got[1:4], exact, 3 * 2.0 ** -24 * mag, "rgb to yuv on views")
    assert np.all(got[[0, 4]] == 0)


# ---- error states ---------------------------------------------------------------------------------------------------------------------
def _error(lib):
    return lib.get_last_cuda_error().decode()


def test_bad_arguments_leave_an_error_text_and_launch_nothing(lib):
    N, H, W, C, f = 4, 3, 5, 2, 2
    x, t0 = _data((C, H, W, N), 1), _data((C, H * f, W * f, N), 2)
    X, T = Dev(x), Dev(t0)
    lib.UpSampleGemm(X.mat, T.mat, X.s4, T.s4, f, 0.0)            # a good call: what the report must keep saying
    good = last_kernel()
    want = T.get().copy()
    assert good[0] == "upsample_kernel<2>/vec"

    def shaped(dev, n, w, h, c):
        s = type(dev.m.shape_)()
        s.shape[0], s.shape[1], s.shape[2], s.shape[3] = n, w, h, c
        return ctypes.byref(s)

    def transposed(dev):
        m = type(dev.m.mat_)()
        ctypes.memmove(ctypes.byref(m), ctypes.byref(dev.m.mat_), ctypes.sizeof(m))
        m.is_trans = 1
        return ctypes.byref(m)
    wide = Dev(_data((C, H * f, W * f + 1, N), 3))
    up = [("NULL operand", lambda: lib.UpSampleGemm(None, T.mat, X.s4, T.s4, f, 0.0)),
          ("NULL operand", lambda: lib.UpSampleGemm(X.mat, None, X.s4, T.s4, f, 0.0)),
          ("NULL operand", lambda: lib.UpSampleGemm(X.mat, T.mat, None, T.s4, f, 0.0)),
          ("transposed operand", lambda: lib.UpSampleGemm(transposed(X), T.mat, X.s4, T.s4, f, 0.0)),
          ("transposed operand", lambda: lib.UpSampleGemm(X.mat, transposed(T), X.s4, T.s4, f, 0.0)),
          ("factor < 1", lambda: lib.UpSampleGemm(X.mat, T.mat, X.s4, T.s4, 0, 0.0)),
          ("factor < 1", lambda: lib.UpSampleGemm(X.mat, T.mat, X.s4, T.s4, -1, 0.0)),
          ("not factor x", lambda: lib.UpSampleGemm(X.mat, T.mat, X.s4, T.s4, 3, 0.0)),
          ("not factor x", lambda: lib.UpSampleGemm(X.mat, wide.mat, X.s4, wide.s4, f, 0.0)),
          ("not factor x", lambda: lib.UpSampleGemm(X.mat, T.mat, X.s4, shaped(T, N, H * f, W * f, C), f, 0.0)),     # axes swapped
          ("channel counts differ", lambda: lib.UpSampleGemm(X.mat, T.mat, X.s4, shaped(T, N, W * f, H * f, C + 1), f, 0.0)),
          ("image counts differ", lambda: lib.UpSampleGemm(X.mat, T.mat, X.s4, shaped(T, N + 1, W * f, H * f, C), f, 0.0)),
          ("size of its shape", lambda: lib.UpSampleGemm(X.mat, T.mat, shaped(X, N, W, H, 1), shaped(T, N, W * f, H * f, 1), f, 0.0))]
    down = [("NULL operand", lambda: lib.DownSampleGemm(None, X.mat, T.s4, X.s4, f)),
            ("transposed operand", lambda: lib.DownSampleGemm(transposed(T), X.mat, T.s4, X.s4, f)),
            ("factor < 1", lambda: lib.DownSampleGemm(T.mat, X.mat, T.s4, X.s4, 0)),
            ("not factor x", lambda: lib.DownSampleGemm(T.mat, X.mat, T.s4, X.s4, 3)),
            ("not factor x", lambda: lib.DownSampleGemm(X.mat, T.mat, X.s4, T.s4, f)),                                  # the operands swapped
            ("channel counts differ", lambda: lib.DownSampleGemm(T.mat, X.mat, T.s4, shaped(X, N, W, H, C + 1), f))]
    rows7 = Flat(np.zeros(7 * N), N)
    rows6, rows9 = Flat(np.zeros(6 * N), N), Flat(np.zeros(9 * N), N)
    yuv = [("NULL operand", lambda: lib.RGBToYUV(None, rows6.mat)),
           ("transposed operand", lambda: lib.RGBToYUV(transposed(rows6), rows6.mat)),
           ("differ in size", lambda: lib.RGBToYUV(rows6.mat, rows9.mat)),
           ("not divisible by 3", lambda: lib.RGBToYUV(rows7.mat, rows7.mat))]
    for entry, cases in (("UpSampleGemm", up), ("DownSampleGemm", down), ("RGBToYUV", yuv)):
        for words, call in cases:
            call()
            msg = _error(lib)
            assert msg.startswith(entry + ": ") and words in msg, (entry, words, msg)
            assert last_kernel() == good, (entry, words, "something was launched")
    same(T.get().view(np.uint32), want.view(np.uint32), "targets after the refused calls")
    same(X.get(), x, "images after the refused calls")
    assert np.all(rows6.get() == 0) and np.all(rows7.get() == 0) and np.all(rows9.get() == 0)


def test_the_matrix_wrappers_refuse_what_the_entries_refuse(lib):
    from convnet_amd.matrix import Matrix, MatrixError
    x = _data((2, 3, 5, 4), 1)
    X, T, Z = Dev(x), Dev(_data((2, 6, 10, 4), 2)), Dev(_data((2, 2, 5, 4), 3))      # Z: 20 columns, not 3 planes
    for call in (lambda: Matrix.ConvUpSample(X.m, T.m, 3, 0), lambda: Matrix.ConvUpSample(X.m, T.m, 0, 0),
                 lambda: Matrix.ConvDownSample(X.m, T.m, 2), lambda: Matrix.ConvRGBToYUV(X.m, T.m), lambda: Matrix.ConvRGBToYUV(Z.m, Z.m)):
        with pytest.raises(MatrixError):
            call()
    Matrix.ConvUpSample(X.m, T.m, 2, 0)
    same(T.get().view(np.uint32), ref.upsample(x, 2).view(np.uint32), "ConvUpSample")
    X.m.Set(0.0)
    Matrix.ConvDownSample(T.m, X.m, 2)
    same(X.get().view(np.uint32), x.view(np.uint32), "the mean of four equal values is the value")
    Y = Dev(np.zeros((3, 2, 5, 4)))
    Matrix.ConvRGBToYUV(Dev(_data((3, 2, 5, 4), 4)).m, Y.m)
    assert np.all(Y.get() != 0)


# ---- matrix paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["default", "split", "fp32"])
def test_the_entries_do_not_depend_on_the_matrix_path(lib, path):
    x, t0 = _data((3, 8, 8, 64), 11), _data((3, 16, 16, 64), 12)
    before = lib.convnet_hip_get_matrix_path()
    try:
        if path != "default":
            lib.convnet_hip_set_matrix_path({"split": 1, "fp32": 0}[path])
        X, T = Dev(x), Dev(t0)
        lib.UpSampleGemm(X.mat, T.mat, X.s4, T.s4, 2, 1.0)
        up = T.get().copy()
        same(up.view(np.uint32), ref.upsample(x, 2, t0, 1.0).view(np.uint32), "upsample", path)
        D, P = Dev(np.zeros(x.shape)), Dev(np.zeros(x.shape))
        lib.DownSampleGemm(T.mat, D.mat, T.s4, D.s4, 2)
        lib.AvgPoolGemm(T.mat, P.mat, T.s4, P.s4, _avg_desc(3, 2), 0.0, 1.0)
        same(D.get().view(np.uint32), P.get().view(np.uint32), "downsample", path)
        Y = Flat(np.zeros(x.shape), 64)
        lib.RGBToYUV(X.mat, Y.mat)
        exact, mag = ref.rgb_to_yuv64(x)
        within(Y.get(), exact, 3 * 2.0 ** -24 * mag, "rgb to yuv", path)
    finally:
        lib.convnet_hip_set_matrix_path(before)


# ---- offsets past 2^31 ----------------------------------------------------------------------------------------------------------------
def test_upsample_and_downsample_address_a_tensor_of_more_than_2_to_the_31_floats(lib):
    """17 x 256 x 256 x 128 upsampled by 4: 2.28e9 floats, so the last planes lie past a 32-bit element offset.  Checked on the device."""
    import torch
    from convnet_amd.matrix import Matrix
    N, C, S, f = 128, 17, 256, 4
    small, large, back = Matrix(), Matrix(), Matrix()
    small.AllocateGPUMemory(N, S * S * C)
    large.AllocateGPUMemory(N, S * S * C * f * f)
    back.AllocateGPUMemory(N, S * S * C)
    small.SetShape4D(N, S, S, C)
    back.SetShape4D(N, S, S, C)
    large.SetShape4D(N, S * f, S * f, C)
    assert large.GetNumEls() > 2 ** 31
    xs = small.tensor()
    xs.copy_(torch.arange(xs.numel(), device=xs.device, dtype=torch.float32).remainder_(8191.0).sub_(4095.0))
    large.tensor().fill_(float("nan"))
    torch.cuda.synchronize()
    lib.UpSampleGemm(small.GetMat(), large.GetMat(), ctypes.byref(small.shape_), ctypes.byref(large.shape_), f, 0.0)
    lib.DownSampleGemm(large.GetMat(), back.GetMat(), ctypes.byref(large.shape_), ctypes.byref(back.shape_), f)
    lib.cuda_sync_threads()
    torch.cuda.synchronize()
    blocks = large.tensor().view(C, S, f, S, f, N)
    assert bool((blocks == xs.view(C, S, 1, S, 1, N)).all())
    assert torch.equal(back.tensor(), xs)      # the mean of 16 equal integers is the integer
