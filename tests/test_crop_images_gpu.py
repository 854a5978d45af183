"""GPU: crop_images_u8 — the crops of decoded images kept at their original sizes as stored bytes (8-bit bilinear resize of the crop's
pixels, crop, mirror, planar split, one launch) — through the C ABI against tests/image_ref.py (scalar loops: resize the whole image,
crop, mirror, planar).  Synthetic buffers and tables built here from image_ref's taps, not by the package.  The output always lies
inside a larger buffer of a fill byte whose other bytes must not change.  Exact; no table is out of range."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import image_ref  # noqa: E402

MAX_CASES = 65
FILL = 0xA5
# name -> (raw y, raw x, crop H, crop W, [(w, h) of the images]); image 0 is shared by the first ten cases (its ten positions)
GEOMETRIES = {
    "1x1": (2, 2, 1, 1, [(5, 4), (3, 7), (1, 3), (2, 2)]),                              # one pixel: a single byte per plane
    "5x7": (6, 9, 5, 7, [(13, 9), (6, 8), (1, 9), (11, 1), (5, 3), (30, 22), (9, 6)]),  # odd H * W: every plane, every second case misaligned
    "4x8": (4, 8, 4, 8, [(11, 9), (6, 8), (1, 5), (9, 1), (4, 2), (25, 13), (8, 4)]),   # all aligned; (8, 4): no resample
    "3x67": (4, 68, 3, 67, [(90, 8), (70, 9), (33, 2), (1, 2), (40, 1), (140, 9)]),     # ragged past a 64-column tile, two groups per lane
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


_CASES = {}


def _case(name):
    """Buffers, tables and the reference crops of a geometry for MAX_CASES cases, computed once and shared; tests take some of them."""
    if name in _CASES:
        return _CASES[name]
    raw_y, raw_x, H, W, sizes = GEOMETRIES[name]
    rng = np.random.default_rng(len(name) + 41)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    resized = [image_ref.resize(im, raw_y, raw_x) for im in images]
    table, taps, offset = [], [], 3                       # (three bytes in front: no image starts at an aligned address)
    for im, big in zip(images, resized):
        h, w = im.shape[:2]
        new_h, new_w = big.shape[:2]
        table.append([offset, w, h, new_w, new_h, len(taps)])
        taps += image_ref.taps(w, new_w) + image_ref.taps(h, new_h)
        offset += im.size
    data = np.concatenate([np.zeros(3, np.uint8)] + [im.reshape(-1) for im in images])
    cases = np.zeros((MAX_CASES, 4), np.int32)
    crops = np.zeros((MAX_CASES, 3 * H * W), np.uint8)
    for n in range(MAX_CASES):
        k = 0 if n < 10 else (n - 10) % len(images) if n < 10 + 2 * len(images) else int(rng.integers(0, len(images)))
        new_h, new_w = resized[k].shape[:2]
        if n < 10:
            left, top, mirrored = image_ref.coordinates(new_w, new_h, n, H, W)
        else:
            left, top, mirrored = int(rng.integers(0, new_w - W + 1)), int(rng.integers(0, new_h - H + 1)), bool(rng.integers(0, 2))
        cases[n] = (k, left, top, mirrored)
        crops[n] = image_ref.planar_crop(resized[k], left, top, H, W, mirrored)
    _CASES[name] = c = dict(data=data, table=np.asarray(table, np.int64), taps=np.asarray(taps, np.int32), cases=cases, crops=crops)
    return c


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _crop(name, cases, before=64, after=64):
    """The rows of ``cases`` through the C ABI, written ``before`` bytes into a buffer of FILL; the bytes around them are checked."""
    import torch
    from convnet_amd._lib import lib
    raw_y, raw_x, H, W, _ = GEOMETRIES[name]
    c, N, dims = _case(name), len(cases), 3 * H * W
    keep = [_dev(c["data"]), _dev(c["table"]), _dev(c["taps"]), _dev(cases)]
    out = torch.full((before + N * dims + after,), FILL, dtype=torch.uint8, device="cuda")
    ptr = lambda t, at=0: ctypes.c_void_p(t.data_ptr() + at)                # noqa: E731
    rc = lib.crop_images_u8(ptr(keep[0]), c["data"].size, ptr(keep[1]), len(c["table"]), ptr(keep[2]), len(c["taps"]), ptr(keep[3]), N,
                            ptr(out, before), W, H)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:before] == FILL).all() and (got[before + N * dims:] == FILL).all()
    return got[before:before + N * dims].reshape(N, dims)


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8].tolist(), got[got != want][:8].tolist(), want[got != want][:8].tolist())


@pytest.mark.parametrize("before", [64, 67], ids=["aligned", "odd_base"])
@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_crop_images_u8_equals_resize_and_crop(gpu, name, N, before):
    c = _case(name)
    _same(_crop(name, c["cases"][:N], before), c["crops"][:N])


def test_the_matrix_wrapper_and_unaligned_views(gpu):
    import torch
    raw_y, raw_x, H, W, _ = GEOMETRIES["5x7"]
    c, N, dims = _case("5x7"), 33, 3 * H * W
    for before in (0, 1, 2, 3):
        out = torch.full((before + N * dims + 5,), FILL, dtype=torch.uint8, device="cuda")
        gpu.CropImagesU8(_dev(c["data"]), _dev(c["table"]), _dev(c["taps"]), _dev(c["cases"][:N]), out[before:before + N * dims], H, W)
        got = out.cpu().numpy()
        _same(got[before:before + N * dims].reshape(N, dims), c["crops"][:N])
        assert (got[:before] == FILL).all() and (got[before + N * dims:] == FILL).all()
    from convnet_amd.matrix import MatrixError
    with pytest.raises(MatrixError, match="rows holds"):
        gpu.CropImagesU8(_dev(c["data"]), _dev(c["table"]), _dev(c["taps"]), _dev(c["cases"][:N]), out[:N * dims - 1], H, W)


@pytest.mark.parametrize("name", ["5x7", "3x67"])
def test_ten_cases_share_one_image_and_a_shuffled_case_table(gpu, name):
    c = _case(name)
    assert (c["cases"][:10, 0] == 0).all() and c["cases"][5:10, 3].all() and not c["cases"][:5, 3].any()
    got = _crop(name, c["cases"][:10])
    _same(got, c["crops"][:10])
    raw_y, raw_x, H, W, _ = GEOMETRIES[name]
    planes = got.reshape(10, 3, H, W)
    assert np.array_equal(planes[5][:, :, ::-1], planes[0])               # the mirrored centre is the centre, columns reversed
    order = np.random.default_rng(5).permutation(MAX_CASES)[:41]
    _same(_crop(name, c["cases"][order], before=65), c["crops"][order])


def test_a_one_pixel_wide_and_a_one_pixel_high_source(gpu):
    for name in ("5x7", "4x8"):
        raw_y, raw_x, H, W, _ = GEOMETRIES[name]
        c = _case(name)
        narrow = np.flatnonzero(c["table"][c["cases"][:, 0], 1] == 1)
        flat = np.flatnonzero(c["table"][c["cases"][:, 0], 2] == 1)
        assert narrow.size >= 2 and flat.size >= 2
        got = _crop(name, c["cases"][narrow])
        _same(got, c["crops"][narrow])
        planes = got.reshape(-1, 3, H, W)
        assert (planes == planes[:, :, :, :1]).all()          # every column of a row is the same source pixel
        got = _crop(name, c["cases"][flat])
        _same(got, c["crops"][flat])
        planes = got.reshape(-1, 3, H, W)
        assert (planes == planes[:, :, :1, :]).all()          # every row is the one source row


def test_an_upscaled_and_a_downscaled_source_in_one_call(gpu):
    c = _case("5x7")
    t = c["table"][c["cases"][:, 0]]
    up = np.flatnonzero((t[:, 3] > t[:, 1]) & (t[:, 4] > t[:, 2]))[:3]
    down = np.flatnonzero((t[:, 3] < t[:, 1]) & (t[:, 4] < t[:, 2]))[:3]
    assert up.size == 3 and down.size == 3
    pick = np.stack([up, down], axis=1).reshape(-1)           # alternating
    _same(_crop("5x7", c["cases"][pick], before=66), c["crops"][pick])


@pytest.mark.parametrize("name", ["5x7", "3x67"])
def test_the_rows_are_the_chunk_stage_patches_u8_takes(gpu, name):
    """The produced bytes, read as a dims x cases chunk, give stage_patches_u8 the patches stage_images_u8 makes from the buffers."""
    import torch
    from hip_adapter import _mat
    raw_y, raw_x, H, W, _ = GEOMETRIES[name]
    ph, pw = H - 1, W - 2
    c, N, dims = _case(name), 37, 3 * H * W
    rng = np.random.default_rng(9)
    mean, std = (rng.random(dims) * 255).astype(np.float32), ((rng.random(dims) + 0.5) * 60).astype(np.float32)
    wo = np.floor(rng.random(N) * (W - pw + 1)).astype(np.float32)
    ho = np.floor(rng.random(N) * (H - ph + 1)).astype(np.float32)
    flip = rng.random(N).astype(np.float32)
    rows = torch.empty(N * dims, dtype=torch.uint8, device="cuda")
    tensors = [_dev(c["data"]), _dev(c["table"]), _dev(c["taps"]), _dev(c["cases"][:N])]
    gpu.CropImagesU8(*tensors, rows, H, W)
    outs = []
    for from_rows in (True, False):
        dst = gpu()
        dst.AllocateGPUMemory(N, 3 * ph * pw)
        args = (_mat(mean, dims, 1), _mat(std, dims, 1), dst, _mat(wo, 1, N), _mat(ho, 1, N), _mat(flip, 1, N), H, W, ph, pw)
        if from_rows:
            gpu.StagePatchesU8(rows, dims, N, _mat(np.arange(N, dtype=np.float32), 1, N), *args)
        else:
            gpu.StageImagesU8(*tensors, *args)
        outs.append(dst.ToNumpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.unique(outs[0]).size > 10


def test_every_error_code_is_returned_with_the_output_untouched(gpu):
    import torch
    from convnet_amd._lib import lib
    raw_y, raw_x, H, W, _ = GEOMETRIES["4x8"]
    c, N, dims = _case("4x8"), 8, 3 * H * W
    keep = [_dev(c["data"]), _dev(c["table"]), _dev(c["taps"]), _dev(c["cases"][:N])]
    out = torch.full((N * dims,), FILL, dtype=torch.uint8, device="cuda")
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in keep + [out]]
    ok = dict(data=ptr[0], nbytes=c["data"].size, table=ptr[1], images=len(c["table"]), taps=ptr[2], ntaps=len(c["taps"]), cases=ptr[3],
              n=N, rows=ptr[4], W=W, H=H)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.crop_images_u8(a["data"], a["nbytes"], a["table"], a["images"], a["taps"], a["ntaps"], a["cases"], a["n"], a["rows"],
                                  a["W"], a["H"])

    DIM, GENERIC, UNSUPPORTED = -1, -6, -9
    errors = [(dict(data=None), GENERIC), (dict(table=None), GENERIC), (dict(taps=None), GENERIC), (dict(cases=None), GENERIC),
              (dict(rows=None), GENERIC), (dict(nbytes=0), DIM), (dict(ntaps=0), DIM), (dict(ntaps=-3), DIM), (dict(images=0), DIM),
              (dict(n=0), DIM), (dict(n=-1), DIM), (dict(W=0), DIM), (dict(H=0), DIM), (dict(H=-1), DIM),
              (dict(images=(1 << 24) + 1), UNSUPPORTED)]
    for kw, code in errors:
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()                  # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    _same(out.cpu().numpy().reshape(N, dims), c["crops"][:N])
