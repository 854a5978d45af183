"""GPU: stage_images_jitter_u8 — one batch out of decoded files under jitter_raw_image: the crop view, the two-pass resize, the
fixed-point rotation, the window, crop, mirror, cast, mean / std, patch offsets / flip and the transpose to CHWN in one launch — against
the host definition (convnet_amd/image_iterators.py, pinned by tests/test_image_jitter_cpu.py) through tests/jitter_scene.py, which lays
the tables out itself.  Files of 37 x 29, 29 x 37, 64 x 48, 50 x 50, 1 x 9 and 9 x 1 under eight hand-chosen jitter rows, raw 20 x 24,
image 16 x 18, patch 12 x 14.  Exact."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jitter_scene as js  # noqa: E402


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def _stage(Matrix, name, index, rotated, normalize, jitter):
    """Cases ``index`` of the scene through the entry into a pre-filled output; the result and what it must be."""
    import torch
    from hip_adapter import _mat
    s = js.scene(name)
    (H, W), (ph, pw) = s["image"], s["patch"]
    if not jitter:
        ph, pw = H, W
    N, dims = len(index), 3 * H * W
    wo, ho, flip = s["wo"][:N], s["ho"][:N], s["flip"][:N]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                      # noqa: E731
    dst = _mat(np.full(N * 3 * ph * pw, -777.0, np.float32), N, 3 * ph * pw)               # pre-filled: a stray or missing store shows
    norm = (_mat(s["mean"], dims, 1), _mat(s["std"], dims, 1)) if normalize else (None, None)
    offs = (_mat(wo, 1, N), _mat(ho, 1, N), _mat(flip, 1, N)) if jitter else (None, None, None)
    Matrix.StageImagesJitterU8(dev(s["data"]), dev(s["table"]), dev(s["taps"]), dev(s["cases"][index]), rotated, *norm, dst, *offs, H, W, ph, pw)
    want = js.expect(name, s["crops"][index], normalize, jitter, wo, ho, flip)
    return dst.ToNumpy().reshape(3, ph, pw, N), want.reshape(3, ph, pw, N)


def _same(got, want):
    assert got.shape == want.shape
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
    assert bad.size == 0, (bad.size, bad[:8].tolist(), got.reshape(-1)[bad[:4]].tolist(), want.reshape(-1)[bad[:4]].tolist())


def test_the_scenes_reach_every_arm():
    """From the host definition alone: border pixels, pixels with both fractions non-zero, and enough unrotated cases for a launch."""
    small, oblong = js.scene("small"), js.scene("oblong")
    assert small["both"] > 0 and small["border"] > 0 and oblong["border"] > 0
    assert small["rotated"].sum() == 7 * 6 and (~small["rotated"]).sum() == 6 and js.unrotated_cases("small").size >= 8
    assert {tuple(r[3:5]) for r in small["table"].tolist()} >= {(24, 20), (29, 24), (33, 28)}       # raw, 15 and 45 degrees


@pytest.mark.parametrize("jitter", [True, False], ids=["patch", "whole_crop"])
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("N", [1, 5, 64, 65, 130])
def test_stage_images_jitter_u8_equals_the_host_definition(gpu, N, normalize, jitter):
    _same(*_stage(gpu, "small", np.arange(N), True, normalize, jitter))


@pytest.mark.parametrize("jitter", [True, False], ids=["patch", "whole_crop"])
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "plain"])
def test_a_launch_without_a_rotated_image_takes_the_arm_without_the_blend(gpu, normalize, jitter):
    plain = js.unrotated_cases("small")
    _same(*_stage(gpu, "small", plain, False, normalize, jitter))
    _same(*_stage(gpu, "small", plain, True, normalize, jitter))               # the other arm gives the same pixels for them


def test_the_arm_without_the_blend_reads_a_rotated_image_as_unrotated(gpu):
    """What include/convnet_hip.h says of rotated = 0, and the proof that the argument picks the arm: case 0 (image 1, turned by 15
    degrees) comes out as the centre crop of its resized view, unturned."""
    from convnet_amd import image_iterators as ii
    s = js.scene("small")
    (H, W), (raw_y, raw_x) = s["image"], s["raw"]
    (w, h), row = js.FILES[0], js.JITTER_ROWS[1]
    left, top, sx, sy, angle, RX, RY = js.image_geometry(w, h, row, raw_y, raw_x)
    assert s["cases"][0].tolist() == [1, (raw_x - W) // 2, (raw_y - H) // 2, 0] and s["table"][1, 3:5].tolist() == [RX, RY] and angle == 15
    at = int(s["table"][1, 0]) - (top * w + left) * 3
    view = s["data"][at:at + w * h * 3].reshape(h, w, 3)[top:top + sy, left:left + sx]
    flat = ii.ResizeTo(view, RY, RX)[(raw_y - H) // 2:(raw_y - H) // 2 + H, (raw_x - W) // 2:(raw_x - W) // 2 + W]
    got, turned = _stage(gpu, "small", np.arange(1), False, False, False)
    assert np.array_equal(got[..., 0], flat.transpose(2, 0, 1).astype(np.float32)) and not np.array_equal(got, turned)


def test_a_patch_wider_than_the_tile(gpu):
    assert js.scene("wide")["patch"][1] > 128
    for normalize in (True, False):
        _same(*_stage(gpu, "wide", np.arange(3), True, normalize, True))


def test_a_rotated_window_that_leaves_the_resized_crop(gpu):
    assert js.scene("oblong")["border"] > 0
    _same(*_stage(gpu, "oblong", np.arange(5), True, True, True))
    _same(*_stage(gpu, "oblong", np.arange(5), True, False, False))


def test_ten_cases_share_one_image_and_a_shuffled_case_table(gpu):
    s = js.scene("small")
    assert (s["cases"][:10, 0] == 1).all() and s["rotated"][1] and s["cases"][5:10, 3].all() and not s["cases"][:5, 3].any()
    _same(*_stage(gpu, "small", np.arange(10), True, True, True))
    order = np.random.default_rng(5).permutation(130)[:77]                     # the table's rows swapped about; offsets stay with the batch slot
    _same(*_stage(gpu, "small", order, True, True, True))


def test_shape_errors_return_the_code_and_launch_nothing(gpu):
    import torch
    from convnet_amd._lib import lib
    from hip_adapter import _mat
    s = js.scene("small")
    (H, W), (ph, pw) = s["image"], s["patch"]
    N, dims = 8, 3 * H * W
    keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s["data"], s["table"], s["taps"], s["cases"][:N])]
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in keep]
    vecN = lambda n=N: _mat(np.zeros(n, np.float32), 1, n)                # noqa: E731
    col = lambda d=dims: _mat(np.ones(d, np.float32), d, 1)               # noqa: E731
    width = 3 * ph * pw
    dst = _mat(np.full(N * width, 7.0, np.float32), N, width)
    ok = dict(data=ptr[0], nbytes=s["data"].size, table=ptr[1], images=len(s["table"]), taps=ptr[2], ntaps=len(s["taps"]), cases=ptr[3],
              mean=col(), std=col(), dst=dst, wo=vecN(), ho=vecN(), fl=vecN(), W=W, H=H, pw=pw, ph=ph)

    def call(**kw):
        a = dict(ok, **kw)
        m = lambda x: x.GetMat() if x is not None else None               # noqa: E731
        return lib.stage_images_jitter_u8(a["data"], a["nbytes"], a["table"], a["images"], a["taps"], a["ntaps"], a["cases"], 1, m(a["mean"]),
                                          m(a["std"]), m(a["dst"]), m(a["wo"]), m(a["ho"]), m(a["fl"]), a["W"], a["H"], a["pw"], a["ph"])

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
    x = s["crops"][:N].astype(np.float32).reshape(N, 3, H, W)[:, :, :ph, :pw] - np.float32(1)
    assert np.array_equal(got, x.transpose(1, 2, 3, 0))
    with pytest.raises(Exception, match="jitter image table"):             # the six-column table of stage_images_u8 is not taken
        gpu.StageImagesJitterU8(keep[0], keep[1][:, :6].contiguous(), keep[2], keep[3], True, None, None, dst, None, None, None, H, W, H, W)
