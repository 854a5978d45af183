"""GPU: stage_clips_u8 — one batch of clips out of a byte buffer that holds every frame once (cast + mean/std of the source pixel inside
the frame + crop + flip + transpose to CHWN with time outermost) — bit for bit equal to the float pipeline on the MATERIALISED clips:
add_col_mult(-1), div_by_col_vec, extract_patches with the frames as extra colours and mean / std tiled, on the committed oracle port
AND on the three existing GPU entries run in sequence; on both of the kernel's grids."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402

# N, clip frames, colours, image W x H, patch W x H, jitter
SHAPES = [
    (33, 3, 3, 9, 7, 6, 5, True),        # everything ragged; odd width: source rows at odd byte addresses
    (5, 2, 1, 35, 37, 32, 33, True),     # ragged patch height; N below one tile
    (64, 4, 1, 28, 28, 28, 28, False),   # NULL offsets: the no-jitter transpose
    (70, 2, 2, 80, 6, 70, 4, True),      # more than one 64-wide tile in both the patch width and N
    (8, 16, 3, 12, 12, 8, 8, True),      # video_small's clip length
    (36, 2, 2, 9, 7, 6, 5, True),        # N a multiple of 4 (16-byte stores) that fills the tile's last image group only partly
    (96, 2, 1, 70, 5, 66, 4, True),      # 16-byte stores in a full tile beside a tail tile of 32 images, two tiles of patch columns
]
EXTRA_FRAMES = 7     # the buffer holds N + T + 7 frames


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _case(shape):
    N, T, colors, W, H, pw, ph, jitter = shape
    rng = np.random.default_rng(N * 1000 + W + T)
    fd, F = colors * W * H, N + T + EXTRA_FRAMES
    frames = rng.integers(0, 256, (F, fd), dtype=np.uint8)
    first = rng.integers(0, F - T + 1, N)
    first[0] = 3
    first[1] = first[0] + 1           # an overlapping pair
    first[2] = first[1]               # a repeat
    first[3], first[4] = F - T, 0     # the last valid start, and 0 behind it: non-monotone
    wo = np.floor(rng.random(N) * (W - pw + 1)).astype(np.float32) + np.float32(0.25)   # rounded down by the kernels' int()
    ho = np.floor(rng.random(N) * (H - ph + 1)).astype(np.float32) + np.float32(0.25)
    wo[0], ho[0], wo[1], ho[1] = 0.0, H - ph, W - pw, 0.0    # 0 and the maximum, both ways
    flip = rng.random(N).astype(np.float32)
    flip[0], flip[1] = 0.9, 0.1
    if not jitter:
        wo[:], ho[:], flip[:] = 0.0, 0.0, 0.0
    mean = (rng.random(fd) * 255).astype(np.float32)
    std = ((rng.random(fd) + 0.5) * 60).astype(np.float32)
    return frames, first, wo, ho, flip, mean, std


def _stage(Matrix, shape, frames, first, wo, ho, flip, mean, std):
    import torch
    from hip_adapter import _mat
    N, T, colors, W, H, pw, ph, jitter = shape
    F, fd = frames.shape
    dev = torch.from_numpy(frames).cuda().view(-1)
    dst = Matrix()
    dst.AllocateGPUMemory(N, T * colors * ph * pw)
    offs = (_mat(wo, 1, N), _mat(ho, 1, N), _mat(flip, 1, N)) if jitter else (None, None, None)
    Matrix.StageClipsU8(dev, fd, F, _mat(np.asarray(first, np.float32), 1, N), T, _mat(mean, fd, 1) if mean is not None else None,
                        _mat(std, fd, 1) if std is not None else None, dst, *offs, H, W, ph, pw)
    return dst.ToNumpy().reshape(T * colors, ph, pw, N)


_REFERENCES = {}


def _references(shape, normalize):
    """The float pipeline's result on the materialised clips, on the oracle port and on the GPU entries: computed once per case."""
    key = (shape, normalize)
    if key not in _REFERENCES:
        from hip_adapter import HipImpl
        N, T, colors, W, H, pw, ph, jitter = shape
        frames, first, wo, ho, flip, mean, std = _case(shape)
        clips = np.ascontiguousarray(np.stack([frames[f:f + T].reshape(-1) for f in first]).astype(np.float32))   # frames concatenated
        refs = []
        for impl in (oracle.port, HipImpl()):
            x = clips.copy()
            if normalize:
                x = impl.div_by_col_vec(impl.add_col_mult(x, np.tile(mean, T), -1.0), np.tile(std, T))
            refs.append((getattr(impl, "kind", "oracle"), impl.extract_patches(np.ascontiguousarray(x), wo, ho, flip, W, H, pw, ph)))   # T * colours colours
        _REFERENCES[key] = refs
    return _REFERENCES[key]


@pytest.mark.parametrize("grid", [1, 2], ids=["clip_per_block", "plane_per_block"])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_T%d_c%d_%dx%d_to_%dx%d%s" % (s[:7] + ("" if s[7] else "_nojitter",)))
def test_stage_clips_u8_equals_the_float_pipeline_bit_for_bit(gpu, shape, normalize, grid):
    from convnet_amd._lib import lib
    frames, first, wo, ho, flip, mean, std = _case(shape)
    lib.convnet_hip_set_stage_clips_grid(grid)
    try:
        got = _stage(gpu, shape, frames, first, wo, ho, flip, mean if normalize else None, std if normalize else None)
    finally:
        lib.convnet_hip_set_stage_clips_grid(0)
    for kind, ref in _references(shape, normalize):
        assert ref.shape == got.shape
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))
        assert bad.size == 0, (kind, bad.size, bad[:8].tolist())


@pytest.mark.parametrize("normalize", [True, False])
def test_one_frame_clips_equal_stage_patches_u8(gpu, normalize):
    import torch
    from hip_adapter import _mat
    shape = (33, 1, 3, 9, 7, 6, 5, True)
    N, T, colors, W, H, pw, ph, _ = shape
    frames, first, wo, ho, flip, mean, std = _case(shape)
    got = _stage(gpu, shape, frames, first, wo, ho, flip, mean if normalize else None, std if normalize else None)
    F, fd = frames.shape
    dst = gpu()
    dst.AllocateGPUMemory(N, colors * ph * pw)
    norm = (_mat(mean, fd, 1), _mat(std, fd, 1)) if normalize else (None, None)
    gpu.StagePatchesU8(torch.from_numpy(frames).cuda().view(-1), fd, F, _mat(first.astype(np.float32), 1, N), *norm, dst, _mat(wo, 1, N),
                       _mat(ho, 1, N), _mat(flip, 1, N), H, W, ph, pw)
    assert np.array_equal(got.reshape(-1).view(np.uint32), dst.ToNumpy().reshape(-1).view(np.uint32))


def test_stage_clips_u8_clamps_what_it_is_given(gpu):
    """A first frame below 0 or beyond F - T, an offset or a flip bit outside its range read the nearest valid frame / row / pixel:
    frame column min(max((int)first, 0) + t, F - 1), never outside the buffer."""
    shape = (33, 3, 3, 9, 7, 6, 5, True)
    N, T, colors, W, H, pw, ph, _ = shape
    frames, first, wo, ho, flip, mean, std = _case(shape)
    F = frames.shape[0]
    wild = first.astype(np.float32)
    wild[0], wild[1], wild[2], wild[5] = -5.0, 1e9, F - 1, F - T + 1
    wo2, ho2 = wo.copy(), ho.copy()
    wo2[3], ho2[4], wo2[5] = 1e6, -40.0, -3.0
    got = _stage(gpu, shape, frames, wild, wo2, ho2, flip, None, None).reshape(T, colors, ph, pw, N)
    img = frames.astype(np.float32).reshape(F, colors, H, W)
    for n in range(N):
        sc = int(wo2[n]) + np.arange(pw)
        if flip[n] > 0.5:
            sc = W - sc - 1
        sc, sr = np.clip(sc, 0, W - 1), np.clip(int(ho2[n]) + np.arange(ph), 0, H - 1)
        for t in range(T):
            f = min(max(int(wild[n]), 0) + t, F - 1)
            assert np.array_equal(got[t, ..., n], img[f][:, sr][:, :, sc]), (n, t)


def test_stage_clips_u8_shape_errors_return_the_code_and_launch_nothing(gpu):
    import torch
    from convnet_amd._lib import lib
    from hip_adapter import _mat
    N, T, colors, W, H, pw, ph = 8, 3, 3, 9, 7, 6, 5
    fd, F = colors * W * H, 12
    dev = torch.zeros(fd * F, dtype=torch.uint8, device="cuda")
    ptr = ctypes.c_void_p(dev.data_ptr())
    vecN = lambda n=N: _mat(np.zeros(n, np.float32), 1, n)                # noqa: E731
    col = lambda d=fd: _mat(np.ones(d, np.float32), d, 1)                 # noqa: E731
    width = T * colors * ph * pw
    dst = _mat(np.full(N * width, 7.0, np.float32), N, width)
    ok = dict(frames=ptr, fd=fd, F=F, first=vecN(), T=T, mean=col(), std=col(), dst=dst, wo=vecN(), ho=vecN(), fl=vecN(), W=W, H=H, pw=pw, ph=ph)

    def call(**kw):
        a = dict(ok, **kw)
        m = lambda x: x.GetMat() if x is not None else None               # noqa: E731
        return lib.stage_clips_u8(a["frames"], a["fd"], a["F"], m(a["first"]), a["T"], m(a["mean"]), m(a["std"]), m(a["dst"]), m(a["wo"]),
                                  m(a["ho"]), m(a["fl"]), a["W"], a["H"], a["pw"], a["ph"])

    DIM, UNSUPPORTED, NOT_ON_DEVICE = -1, -9, -8
    wrong_dst = _mat(np.zeros(N * (width + 1), np.float32), N, width + 1)
    errors = [
        (dict(dst=wrong_dst), DIM), (dict(first=vecN(N + 1)), DIM), (dict(mean=col(fd - 1)), DIM), (dict(std=None), DIM),
        (dict(mean=col(fd * T), std=col(fd * T)), DIM),                    # mean / std are per FRAME pixel
        (dict(mean=_mat(np.ones(fd, np.float32), 1, fd)), DIM), (dict(wo=vecN(N - 1)), DIM), (dict(fl=None), DIM),
        (dict(pw=W + 1), DIM), (dict(ph=H + 1), DIM), (dict(fd=fd + 1), DIM), (dict(W=0), DIM), (dict(F=0), DIM),
        (dict(T=0), DIM), (dict(T=T + 1), DIM), (dict(T=-1), DIM),
        (dict(wo=None, ho=None, fl=None), DIM),          # no jitter, but the patch is not the whole image
        (dict(F=(1 << 24) + 1), UNSUPPORTED), (dict(frames=None), NOT_ON_DEVICE), (dict(first=None), NOT_ON_DEVICE),
    ]
    for kw, code in errors:
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert np.all(dst.ToNumpy() == 7.0)                   # nothing ran
    assert call() == 0
    assert np.all(dst.ToNumpy() == -1.0)                  # the same arguments, unbroken: zero bytes, mean 1, std 1
