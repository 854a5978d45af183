"""GPU: resize_frames_u8 — frames of one geometry stretched to stored planar bytes, one launch — through Matrix.ResizeFramesU8 against two
references: a restatement of include/convnet_hip.h's formula (h(y), then result) in int64, with the entry's clamps of the source indices,
and crop_images_u8 on equivalent tables (one image-table row per frame, all pointing at one shared tap block, cases {n, 0, 0, mirrored}):
the route that existed before.  Seeded random frames, both mirror values, 1, 3 and 65 frames; the source starts 3 bytes past an aligned
address and the output lies at an odd offset inside a buffer of a fill byte whose other bytes must not change.  Exact; every input is
inside the buffers by the entry's own contract."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import image_ref  # noqa: E402

FILL = 0xA5
# name -> (w, h, W, H, frame counts)
GEOMETRIES = {
    "5x7-70x66": (5, 7, 70, 66, [1, 3, 65]),       # upsizing, shared source rows; H * W and the frame size no multiples of 4; misaligned bases
    "70x66-5x7": (70, 66, 5, 7, [3]),              # downsizing by more than 2x; an output row narrower than one lane group
    "5x7-5x7": (5, 7, 5, 7, [3]),                  # identity taps
    "1x1-9x4": (1, 1, 9, 4, [3]),                  # every clamp
    "1100x3-1030x3": (1100, 3, 1030, 3, [2]),      # wider than one column tile, and a tail of two columns
    "9x300-9x20": (9, 300, 9, 20, [3]),            # many row tiles, nothing shared
    "9x20-9x300": (9, 20, 9, 300, [3]),            # many row tiles, every source row shared
    "700x5-150x3": (700, 5, 150, 3, [2]),          # a width shrunk past what a tile stages: the scalar arm
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _taps(w, h, W, H):
    return np.asarray(image_ref.taps(w, W) + image_ref.taps(h, H), np.int32)


def restated(frames, taps, W, H, mirrored):
    """(N, 3 * H * W) bytes by the definition in int64: frames is (N, h, w, 3); the source indices of ``taps`` clamped as the entry does."""
    N, h, w, _ = frames.shape
    p = frames.astype(np.int64)
    t = taps.astype(np.int64)
    ct, rt = t[:W], t[W:]
    if mirrored:
        ct = ct[::-1]
    sx, sy = np.clip(ct[:, 0], 0, w - 1), np.clip(rt[:, 0], 0, h - 1)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    a0, a1 = ct[:, 1][None, None, :, None], ct[:, 2][None, None, :, None]
    hy = ((((2048 * ((p[:, :, sx] * a0 + p[:, :, sx1] * a1) >> 4)) >> 16) + 2) >> 2)                  # (N, h, W, 3)
    b0, b1 = rt[:, 1][None, :, None, None], rt[:, 2][None, :, None, None]
    out = ((((b0 * ((2048 * hy[:, sy]) >> 4)) >> 16) + ((b1 * ((2048 * hy[:, sy1]) >> 4)) >> 16) + 2) >> 2)
    return (out & 255).astype(np.uint8).transpose(0, 3, 1, 2).reshape(N, 3 * H * W)


_FRAMES = {}


def _frames(name):
    """65 (or fewer) seeded frames of a geometry, made once and shared."""
    if name not in _FRAMES:
        w, h, W, H, counts = GEOMETRIES[name]
        _FRAMES[name] = np.random.default_rng(len(name) + 7 * w + h).integers(0, 256, (max(counts), h, w, 3), dtype=np.uint8)
    return _FRAMES[name]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _source(frames):
    """The frames on the device, three bytes in front: no frame starts at an aligned address unless its size says so."""
    return _dev(np.concatenate([np.zeros(3, np.uint8), frames.reshape(-1)]))


def _resize(gpu, frames, taps, W, H, mirrored, before=65, after=64):
    import torch
    N, h, w, _ = frames.shape
    dims = 3 * H * W
    out = torch.full((before + N * dims + after,), FILL, dtype=torch.uint8, device="cuda")
    gpu.ResizeFramesU8(_source(frames)[3:], N, h, w, _dev(taps), out[before:before + N * dims], H, W, mirrored)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:before] == FILL).all() and (got[before + N * dims:] == FILL).all()
    return got[before:before + N * dims].reshape(N, dims)


def _crop(gpu, frames, taps, W, H, mirrored):
    """The same bytes by crop_images_u8: every frame an image of the table, one shared tap block."""
    import torch
    N, h, w, _ = frames.shape
    table = np.asarray([[3 + n * w * h * 3, w, h, W, H, 0] for n in range(N)], np.int64)
    cases = np.asarray([[n, 0, 0, int(mirrored)] for n in range(N)], np.int32)
    rows = torch.empty(N * 3 * H * W, dtype=torch.uint8, device="cuda")
    gpu.CropImagesU8(_source(frames), _dev(table), _dev(taps), _dev(cases), rows, H, W)
    return rows.cpu().numpy().reshape(N, 3 * H * W)


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8].tolist(), got[got != want][:8].tolist(), want[got != want][:8].tolist())


CASES = [(name, n, m) for name, g in GEOMETRIES.items() for n in g[4] for m in (False, True)]


@pytest.mark.parametrize("name,N,mirrored", CASES, ids=[f"{a}-{n}-{'mirrored' if m else 'plain'}" for a, n, m in CASES])
def test_resize_frames_u8_equals_the_definition_and_crop_images_u8(gpu, name, N, mirrored):
    w, h, W, H, _ = GEOMETRIES[name]
    frames, taps = _frames(name)[:N], _taps(w, h, W, H)
    got = _resize(gpu, frames, taps, W, H, mirrored)
    _same(got, restated(frames, taps, W, H, mirrored))
    _same(got, _crop(gpu, frames, taps, W, H, mirrored))
    if (w, h) == (W, H):
        plain = frames.transpose(0, 3, 1, 2)
        _same(got, np.ascontiguousarray(plain[:, :, :, ::-1] if mirrored else plain).reshape(N, -1))


def test_the_restatement_is_the_scalar_reference(gpu):
    """The vectorised restatement above against tests/image_ref.py's scalar loops, so that both references of this file are pinned."""
    w, h, W, H, _ = GEOMETRIES["5x7-70x66"]
    frames = _frames("5x7-70x66")[:1]
    big = image_ref.height_pass(image_ref.width_pass(frames[0], W), H)
    _same(restated(frames, _taps(w, h, W, H), W, H, True), image_ref.planar_crop(big, 0, 0, H, W, True)[None])


@pytest.mark.parametrize("name", ["5x7-70x66", "70x66-5x7", "1100x3-1030x3", "9x300-9x20"])
def test_wild_source_indices_are_clamped(gpu, name):
    w, h, W, H, _ = GEOMETRIES[name]
    rng = np.random.default_rng(len(name))
    taps = _taps(w, h, W, H)
    taps[:, 0] = rng.integers(-2 ** 31, 2 ** 31, len(taps)) >> rng.integers(0, 24, len(taps))      # any sign, any size, any order
    frames = _frames(name)[:2]
    for mirrored in (False, True):
        got = _resize(gpu, frames, taps, W, H, mirrored, before=66)
        _same(got, restated(frames, taps, W, H, mirrored))
        _same(got, _crop(gpu, frames, taps, W, H, mirrored))


def test_the_wrapper_refuses_tensors_that_do_not_fit(gpu):
    import torch
    from convnet_amd.matrix import MatrixError
    w, h, W, H, _ = GEOMETRIES["5x7-5x7"]
    frames, taps = _frames("5x7-5x7")[:2], _dev(_taps(w, h, W, H))
    src, rows = _dev(frames.reshape(-1)), torch.empty(2 * 3 * H * W, dtype=torch.uint8, device="cuda")
    with pytest.raises(MatrixError, match="rows holds"):
        gpu.ResizeFramesU8(src, 2, h, w, taps, rows[:-1], H, W, False)
    with pytest.raises(MatrixError, match="the tap table has"):
        gpu.ResizeFramesU8(src, 2, h, w, taps[:-1], rows, H, W, False)
    with pytest.raises(MatrixError, match="tap table must be a contiguous"):
        gpu.ResizeFramesU8(src, 2, h, w, taps.to(torch.int64), rows, H, W, False)
    with pytest.raises(MatrixError, match="Error resizing frames"):
        gpu.ResizeFramesU8(src[:-1], 2, h, w, taps, rows, H, W, False)                       # one byte short: the entry's own check


def test_every_error_code_is_returned_with_the_output_untouched(gpu):
    import torch
    from convnet_amd._lib import lib
    w, h, W, H, _ = GEOMETRIES["5x7-70x66"]
    N = 3
    frames, taps = _frames("5x7-70x66")[:N], _taps(w, h, W, H)
    keep = [_dev(frames.reshape(-1)), _dev(taps)]
    out = torch.full((N * 3 * H * W,), FILL, dtype=torch.uint8, device="cuda")
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in keep + [out]]
    ok = dict(data=ptr[0], nbytes=frames.size, n=N, w=w, h=h, taps=ptr[1], W=W, H=H, mirrored=0, rows=ptr[2])

    def call(**kw):
        a = dict(ok, **kw)
        return lib.resize_frames_u8(a["data"], a["nbytes"], a["n"], a["w"], a["h"], a["taps"], a["W"], a["H"], a["mirrored"], a["rows"])

    DIM, GENERIC, UNSUPPORTED = -1, -6, -9
    errors = [(dict(data=None), GENERIC), (dict(taps=None), GENERIC), (dict(rows=None), GENERIC), (dict(data=None, n=0), GENERIC),
              (dict(n=0), DIM), (dict(n=-1), DIM), (dict(w=0), DIM), (dict(h=0), DIM), (dict(W=0), DIM), (dict(H=-2), DIM),
              (dict(nbytes=frames.size - 1), DIM), (dict(nbytes=0), DIM), (dict(n=2 ** 31 - 1, w=2 ** 31 - 1, h=2 ** 31 - 1), DIM),
              (dict(n=2 ** 31 - 1, W=2 ** 30, H=2 ** 30), DIM), (dict(W=2 ** 30, H=2 ** 30), UNSUPPORTED)]
    for kw, code in errors:
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()                  # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    _same(out.cpu().numpy().reshape(N, -1), restated(frames, taps, W, H, False))
