"""GPU: stage_images_u8 — one batch out of decoded images kept at their original sizes: the 8-bit bilinear resize of the crop's pixels,
crop, mirror, cast, mean / std of the crop's pixel, patch offsets / flip and the transpose to CHWN in one launch — against
tests/image_ref.py (scalar loops: resize the whole image, crop, mirror, planar) plus numpy float32 for the normalisation and the patch.
Synthetic buffers and tables straight to the entry; the tables are built here from image_ref's taps, not by the package.  Exact."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import image_ref  # noqa: E402

MAX_CASES = 130
# name -> (raw y, raw x, crop H, crop W, patch h, patch w, [(w, h) of the images])
GEOMETRIES = {
    "small": (4, 6, 3, 4, 2, 3, [(9, 7), (6, 8), (13, 4), (5, 9), (1, 9), (8, 8), (6, 4)]),      # (1, 9): a 1-pixel-wide source; (6, 4): no resample
    "wide": (6, 80, 5, 72, 4, 70, [(90, 8), (70, 9), (80, 6), (33, 2)]),                         # a 70-column patch: past the 64-wide tile
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
    """Buffers, tables and the reference crops of a geometry for MAX_CASES cases, computed once; tests take the first N cases."""
    if name in _CASES:
        return _CASES[name]
    raw_y, raw_x, H, W, ph, pw, sizes = GEOMETRIES[name]
    rng = np.random.default_rng(len(name) + 17)
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
        k = 0 if n < 10 else int(rng.integers(0, len(images)))        # one image shared by the first ten cases: its ten positions
        new_h, new_w = resized[k].shape[:2]
        if n < 10:
            left, top, mirrored = image_ref.coordinates(new_w, new_h, n, H, W)
        else:
            left, top, mirrored = int(rng.integers(0, new_w - W + 1)), int(rng.integers(0, new_h - H + 1)), bool(rng.integers(0, 2))
        cases[n] = (k, left, top, mirrored)
        crops[n] = image_ref.planar_crop(resized[k], left, top, H, W, mirrored)
    dims = 3 * H * W
    c = dict(data=data, table=np.asarray(table, np.int64), taps=np.asarray(taps, np.int32), cases=cases, crops=crops,
             mean=(rng.random(dims) * 255).astype(np.float32), std=((rng.random(dims) + 0.5) * 60).astype(np.float32),
             wo=np.floor(rng.random(MAX_CASES) * (W - pw + 1)).astype(np.float32) + np.float32(0.25),
             ho=np.floor(rng.random(MAX_CASES) * (H - ph + 1)).astype(np.float32) + np.float32(0.25),
             flip=rng.random(MAX_CASES).astype(np.float32))
    c["wo"][:2], c["ho"][:2], c["flip"][:2] = (0.0, W - pw), (H - ph, 0.0), (0.9, 0.1)      # 0 and the maximum, both ways
    _CASES[name] = c
    return c


def _expect(name, crops, normalize, jitter, wo, ho, flip):
    raw_y, raw_x, H, W, ph, pw, _ = GEOMETRIES[name]
    c = _case(name)
    x = crops.astype(np.float32)
    if normalize:
        x = (x - c["mean"][None, :]) / c["std"][None, :]             # float32, one rounding each: add_col_mult(-1), div_by_col_vec
    N = len(crops)
    x = x.reshape(N, 3, H, W)
    if not jitter:
        return np.ascontiguousarray(x.transpose(1, 2, 3, 0))
    out = np.empty((3, ph, pw, N), np.float32)
    for n in range(N):
        sc = int(wo[n]) + np.arange(pw)
        if flip[n] > 0.5:
            sc = W - sc - 1
        out[..., n] = x[n][:, int(ho[n]) + np.arange(ph)][:, :, sc]
    return out


def _stage(Matrix, name, cases, normalize, jitter, wo, ho, flip):
    import torch
    from hip_adapter import _mat
    raw_y, raw_x, H, W, ph, pw, _ = GEOMETRIES[name]
    if not jitter:
        ph, pw = H, W
    c, N, dims = _case(name), len(cases), 3 * H * W
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                      # noqa: E731
    dst = Matrix()
    dst.AllocateGPUMemory(N, 3 * ph * pw)
    norm = (_mat(c["mean"], dims, 1), _mat(c["std"], dims, 1)) if normalize else (None, None)
    offs = (_mat(wo, 1, N), _mat(ho, 1, N), _mat(flip, 1, N)) if jitter else (None, None, None)
    Matrix.StageImagesU8(dev(c["data"]), dev(c["table"]), dev(c["taps"]), dev(cases), *norm, dst, *offs, H, W, ph, pw)
    return dst.ToNumpy().reshape(3, ph, pw, N)


def _same(got, want):
    assert got.shape == want.shape
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got.reshape(-1)[bad[:4]].tolist(), want.reshape(-1)[bad[:4]].tolist())


@pytest.mark.parametrize("jitter", [True, False], ids=["patch", "whole_crop"])
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("N", [1, 5, 64, 65, 130])
def test_stage_images_u8_equals_resize_crop_and_the_float_pipeline(gpu, N, normalize, jitter):
    c = _case("small")
    wo, ho, flip = c["wo"][:N], c["ho"][:N], c["flip"][:N]
    got = _stage(gpu, "small", c["cases"][:N], normalize, jitter, wo, ho, flip)
    _same(got, _expect("small", c["crops"][:N], normalize, jitter, wo, ho, flip))


@pytest.mark.parametrize("jitter", [True, False], ids=["patch", "whole_crop"])
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "plain"])
def test_a_patch_wider_than_the_tile(gpu, normalize, jitter):
    c, N = _case("wide"), 67
    wo, ho, flip = c["wo"][:N], c["ho"][:N], c["flip"][:N]
    got = _stage(gpu, "wide", c["cases"][:N], normalize, jitter, wo, ho, flip)
    _same(got, _expect("wide", c["crops"][:N], normalize, jitter, wo, ho, flip))


def test_ten_cases_share_one_image_and_a_shuffled_case_table(gpu):
    c = _case("small")
    assert (c["cases"][:10, 0] == 0).all() and c["cases"][5:10, 3].all() and not c["cases"][:5, 3].any()
    wo, ho, flip = c["wo"][:10], c["ho"][:10], c["flip"][:10]
    _same(_stage(gpu, "small", c["cases"][:10], True, True, wo, ho, flip), _expect("small", c["crops"][:10], True, True, wo, ho, flip))
    order = np.random.default_rng(5).permutation(MAX_CASES)[:77]          # the table's rows swapped about; offsets stay with the batch slot
    wo, ho, flip = c["wo"][:77], c["ho"][:77], c["flip"][:77]
    got = _stage(gpu, "small", c["cases"][order], True, True, wo, ho, flip)
    _same(got, _expect("small", c["crops"][order], True, True, wo, ho, flip))


def test_a_one_pixel_wide_source(gpu):
    c = _case("small")
    narrow = np.flatnonzero(c["table"][c["cases"][:, 0], 1] == 1)
    assert narrow.size >= 3
    zeros = np.zeros(narrow.size, np.float32)
    got = _stage(gpu, "small", c["cases"][narrow], False, False, zeros, zeros, zeros)
    _same(got, _expect("small", c["crops"][narrow], False, False, zeros, zeros, zeros))
    assert (got == got[:, :, :1, :]).all()                # every column of a row is the same source pixel


def test_stage_images_u8_shape_errors_return_the_code_and_launch_nothing(gpu):
    import torch
    from convnet_amd._lib import lib
    from hip_adapter import _mat
    raw_y, raw_x, H, W, ph, pw, _ = GEOMETRIES["small"]
    c, N, dims = _case("small"), 8, 3 * H * W
    keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["data"], c["table"], c["taps"], c["cases"][:N])]
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in keep]
    vecN = lambda n=N: _mat(np.zeros(n, np.float32), 1, n)                # noqa: E731
    col = lambda d=dims: _mat(np.ones(d, np.float32), d, 1)               # noqa: E731
    width = 3 * ph * pw
    dst = _mat(np.full(N * width, 7.0, np.float32), N, width)
    ok = dict(data=ptr[0], nbytes=c["data"].size, table=ptr[1], images=len(c["table"]), taps=ptr[2], ntaps=len(c["taps"]), cases=ptr[3],
              mean=col(), std=col(), dst=dst, wo=vecN(), ho=vecN(), fl=vecN(), W=W, H=H, pw=pw, ph=ph)

    def call(**kw):
        a = dict(ok, **kw)
        m = lambda x: x.GetMat() if x is not None else None               # noqa: E731
        return lib.stage_images_u8(a["data"], a["nbytes"], a["table"], a["images"], a["taps"], a["ntaps"], a["cases"], m(a["mean"]), m(a["std"]),
                                   m(a["dst"]), m(a["wo"]), m(a["ho"]), m(a["fl"]), a["W"], a["H"], a["pw"], a["ph"])

    DIM, GENERIC, UNSUPPORTED = -1, -6, -9
    wrong_dst = _mat(np.zeros(N * (width + 1), np.float32), N, width + 1)
    errors = [
        (dict(data=None), GENERIC), (dict(table=None), GENERIC), (dict(taps=None), GENERIC), (dict(cases=None), GENERIC), (dict(dst=None), GENERIC),
        (dict(dst=wrong_dst), DIM), (dict(mean=col(dims - 1)), DIM), (dict(std=None), DIM), (dict(mean=_mat(np.ones(dims, np.float32), 1, dims)), DIM),
        (dict(wo=vecN(N - 1)), DIM), (dict(fl=None), DIM), (dict(pw=W + 1), DIM), (dict(ph=H + 1), DIM), (dict(W=0), DIM), (dict(H=-1), DIM),
        (dict(nbytes=0), DIM), (dict(ntaps=0), DIM), (dict(images=0), DIM),
        (dict(wo=None, ho=None, fl=None), DIM),          # no jitter, but the patch is not the whole crop
        (dict(images=(1 << 24) + 1), UNSUPPORTED),
    ]
    for kw, code in errors:
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert np.all(dst.ToNumpy() == 7.0)                   # nothing ran
    assert call() == 0
    got = dst.ToNumpy().reshape(3, ph, pw, N)             # the same arguments, unbroken: offsets 0, no flip, mean 1, std 1
    x = c["crops"][:N].astype(np.float32).reshape(N, 3, H, W)[:, :, :ph, :pw] - np.float32(1)
    assert np.array_equal(got, x.transpose(1, 2, 3, 0))
