"""GPU: stage_patches_u8 — one batch out of a byte chunk (cast + mean/std of the source pixel + crop + flip + transpose to CHWN) —
bit for bit equal to the float pipeline it replaces: add_col_mult(-1), div_by_col_vec, extract_patches on the float cast of the same
bytes, on the committed oracle port AND on the three existing GPU entries run in sequence."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402

# N, colours, image W x H, patch W x H, jitter
SHAPES = [
    (33, 3, 9, 7, 6, 5, True),       # N and patch width off every tile size; odd image width: source rows are not 4-byte aligned
    (5, 3, 35, 37, 32, 33, True),    # a full 32-wide run beside a ragged height, N below one tile
    (64, 1, 28, 28, 28, 28, False),  # NULL offsets: the no-jitter transpose
    (40, 3, 41, 41, 35, 35, True),   # the existing staging test's geometry
    (70, 2, 80, 6, 70, 4, True),     # more than one 64-wide tile in both the patch width and N
]
EXTRA_CASES = 7     # the chunk is wider than the batch


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _case(shape):
    N, colors, W, H, pw, ph, jitter = shape
    rng = np.random.default_rng(N * 1000 + W)
    dims, cases = colors * W * H, N + EXTRA_CASES
    chunk = rng.integers(0, 256, (cases, dims), dtype=np.uint8)
    idx = rng.permutation(cases)[:N]
    idx[0] = cases - 1                # the last column of the chunk
    idx[2] = idx[1]                   # a repeated column
    if np.all(np.diff(idx) > 0):      # non-monotone (a permutation's head practically always is)
        idx[3], idx[4] = idx[4], idx[3]
    wo = np.floor(rng.random(N) * (W - pw + 1)).astype(np.float32) + np.float32(0.25)   # rounded down by the kernels' int()
    ho = np.floor(rng.random(N) * (H - ph + 1)).astype(np.float32) + np.float32(0.25)
    wo[0], ho[0], wo[1], ho[1] = 0.0, H - ph, W - pw, 0.0    # 0 and the maximum, both ways
    flip = rng.random(N).astype(np.float32)
    flip[0], flip[1] = 0.9, 0.1
    if not jitter:
        wo[:], ho[:], flip[:] = 0.0, 0.0, 0.0
    mean = (rng.random(dims) * 255).astype(np.float32)
    std = ((rng.random(dims) + 0.5) * 60).astype(np.float32)
    return chunk, idx, wo, ho, flip, mean, std


def _stage(Matrix, shape, chunk, idx, wo, ho, flip, mean, std):
    import torch
    from hip_adapter import _mat
    N, colors, W, H, pw, ph, jitter = shape
    dims, cases = chunk.shape[1], chunk.shape[0]
    dev = torch.from_numpy(chunk).cuda().view(-1)
    dst = Matrix()
    dst.AllocateGPUMemory(N, colors * ph * pw)
    offs = (_mat(wo, 1, N), _mat(ho, 1, N), _mat(flip, 1, N)) if jitter else (None, None, None)
    Matrix.StagePatchesU8(dev, dims, cases, _mat(idx.astype(np.float32), 1, N), _mat(mean, dims, 1) if mean is not None else None,
                          _mat(std, dims, 1) if std is not None else None, dst, *offs, H, W, ph, pw)
    return dst.ToNumpy().reshape(colors, ph, pw, N)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_c%d_%dx%d_to_%dx%d%s" % (s[:6] + ("" if s[6] else "_nojitter",)))
def test_stage_patches_u8_equals_the_float_pipeline_bit_for_bit(gpu, shape, normalize):
    from hip_adapter import HipImpl
    N, colors, W, H, pw, ph, jitter = shape
    chunk, idx, wo, ho, flip, mean, std = _case(shape)
    got = _stage(gpu, shape, chunk, idx, wo, ho, flip, mean if normalize else None, std if normalize else None)
    images = np.ascontiguousarray(chunk[idx].astype(np.float32))       # the reference's host cast of the batch's rows
    for impl in (oracle.port, HipImpl()):
        x = images.copy()
        if normalize:
            x = impl.div_by_col_vec(impl.add_col_mult(x, mean, -1.0), std)
        ref = impl.extract_patches(np.ascontiguousarray(x), wo, ho, flip, W, H, pw, ph)
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))
        assert bad.size == 0, (getattr(impl, "kind", "oracle"), bad.size, bad[:8].tolist())


def test_stage_patches_u8_clamps_what_it_is_given(gpu):
    """A case index, an offset or a flip bit outside its range reads the nearest valid column / row / pixel, never outside the chunk."""
    shape = (33, 3, 9, 7, 6, 5, True)
    N, colors, W, H, pw, ph, _ = shape
    chunk, idx, wo, ho, flip, mean, std = _case(shape)
    cases = chunk.shape[0]
    wild = idx.astype(np.float32)
    wild[0], wild[1], wild[2] = -5.0, 1e9, cases + 3
    wo2, ho2 = wo.copy(), ho.copy()
    wo2[3], ho2[4], wo2[5] = 1e6, -40.0, -3.0
    got = _stage(gpu, shape, chunk, wild, wo2, ho2, flip, None, None)
    col = np.clip(wild.astype(np.int64), 0, cases - 1)
    img = chunk[col].astype(np.float32).reshape(N, colors, H, W)
    for n in range(N):
        sc = int(wo2[n]) + np.arange(pw)
        if flip[n] > 0.5:
            sc = W - sc - 1
        sc, sr = np.clip(sc, 0, W - 1), np.clip(int(ho2[n]) + np.arange(ph), 0, H - 1)
        assert np.array_equal(got[..., n], img[n][:, sr][:, :, sc]), n


def test_stage_patches_u8_shape_errors_return_the_code_and_launch_nothing(gpu):
    import torch
    from convnet_amd._lib import lib
    from hip_adapter import _mat
    N, colors, W, H, pw, ph = 8, 3, 9, 7, 6, 5
    dims, cases = colors * W * H, 12
    dev = torch.zeros(dims * cases, dtype=torch.uint8, device="cuda")
    ptr = ctypes.c_void_p(dev.data_ptr())
    vecN = lambda n=N: _mat(np.zeros(n, np.float32), 1, n)                # noqa: E731
    col = lambda d=dims: _mat(np.ones(d, np.float32), d, 1)               # noqa: E731
    dst = _mat(np.full(N * colors * ph * pw, 7.0, np.float32), N, colors * ph * pw)
    ok = dict(chunk=ptr, dims=dims, cases=cases, idx=vecN(), mean=col(), std=col(), dst=dst, wo=vecN(), ho=vecN(), fl=vecN(), W=W, H=H, pw=pw, ph=ph)

    def call(**kw):
        a = dict(ok, **kw)
        m = lambda x: x.GetMat() if x is not None else None               # noqa: E731
        return lib.stage_patches_u8(a["chunk"], a["dims"], a["cases"], m(a["idx"]), m(a["mean"]), m(a["std"]), m(a["dst"]), m(a["wo"]), m(a["ho"]),
                                    m(a["fl"]), a["W"], a["H"], a["pw"], a["ph"])

    DIM, UNSUPPORTED, NOT_ON_DEVICE = -1, -9, -8
    wrong_dst = _mat(np.zeros(N * (colors * ph * pw + 1), np.float32), N, colors * ph * pw + 1)
    errors = [
        (dict(dst=wrong_dst), DIM), (dict(idx=vecN(N + 1)), DIM), (dict(mean=col(dims - 1)), DIM), (dict(std=None), DIM),
        (dict(mean=_mat(np.ones(dims, np.float32), 1, dims)), DIM), (dict(wo=vecN(N - 1)), DIM), (dict(fl=None), DIM),
        (dict(pw=W + 1), DIM), (dict(ph=H + 1), DIM), (dict(dims=dims + 1), DIM), (dict(W=0), DIM), (dict(cases=0), DIM),
        (dict(wo=None, ho=None, fl=None), DIM),          # no jitter, but the patch is not the whole image
        (dict(cases=(1 << 24) + 1), UNSUPPORTED), (dict(chunk=None), NOT_ON_DEVICE),
    ]
    for kw, code in errors:
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert np.all(dst.ToNumpy() == 7.0)                   # nothing ran
    assert call() == 0
    assert np.all(dst.ToNumpy() == -1.0)                  # the same arguments, unbroken: zero bytes, mean 1, std 1
