"""Scenes for stage_images_jitter_u8, shared by the emulated and the GPU test of the entry: decoded files, hand-chosen jitter rows, the
11-column image table with its taps and rotation rows (include/convnet_hip.h), a case table, and what the entry must leave — all from
the HOST DEFINITION (convnet_amd/image_iterators.py: CropRect, RotSize, ImageTaps, RotationTables, TransformCrop), which
tests/test_image_jitter_cpu.py pins.  The tables are laid out here, not by the data handler.  A plain module, no fixture of its own."""
import numpy as np

from convnet_amd import image_iterators as ii

BELOW_1 = float(np.nextafter(np.float32(1), np.float32(0)))
# (angle, trans_x, trans_y, scale), chosen by hand: no rotation; a plain one; the worked example's; a tiny angle (fractions next to
# none); 45 degrees from a corner, zoomed; the exact turns; a negative angle from the other corner at three times the zoom
JITTER_ROWS = [(0.0, .5, .5, 1.0), (15.0, .3, .7, 1.0), (-14.9997654, .131537795, .75560534, 1.27067494), (0.01, .6, .2, 1.0),
               (45.0, 0.0, BELOW_1, 1.5), (90.0, .5, .5, 1.0), (180.0, .25, .75, 1.2), (-33.3, BELOW_1, 0.0, 3.0)]
FILES = [(37, 29), (29, 37), (64, 48), (50, 50), (1, 9), (9, 1)]                # (w, h)
# name -> raw y, raw x, crop H, W, patch h, w, the files, the jitter rows, cases
GEOMETRIES = {
    "small": dict(raw=(20, 24), image=(16, 18), patch=(12, 14), files=FILES, rows=JITTER_ROWS, cases=130),
    "wide": dict(raw=(40, 150), image=(36, 140), patch=(30, 130), files=[(200, 60), (90, 45)], rows=[JITTER_ROWS[0], JITTER_ROWS[1]], cases=3),
    "oblong": dict(raw=(20, 60), image=(16, 50), patch=(12, 40), files=[(64, 48), (37, 29)], rows=[JITTER_ROWS[4]], cases=5),
}
_SCENES = {}


def image_geometry(w, h, row, raw_y, raw_x):
    """(left, top, crop w, crop h, angle, RX, RY) of a w x h file under a jitter row.  Two departures, for files and angles the
    reference could not run: a crop that comes out empty is the whole file, and 180 degrees — where RotSize is negative — resizes to
    the raw size."""
    angle, tx, ty, scale = row
    left, top, sx, sy = ii.CropRect(w, h, tx, ty, scale, raw_x, raw_y)
    if sx < 1 or sy < 1:
        left, top, sx, sy = 0, 0, w, h
    RX, RY = (raw_x, raw_y) if np.float32(angle) == 0 or abs(angle) > 135 else ii.RotSize(angle, raw_x, raw_y)
    return left, top, sx, sy, angle, RX, RY


def scene(name):
    """Everything about a geometry, computed once: ``data`` (3 bytes, then the files back to back), ``table`` (images, 11), ``taps``,
    ``cases`` / ``crops`` for the geometry's number of cases (tests take subsets), ``rotated`` per image, mean / std / offsets / flip,
    and over the pixels the cases read: ``border`` (rotated pixels with a neighbour of non-zero weight outside the resized crop) and
    ``both`` (rotated pixels whose fx and fy are both non-zero)."""
    if name in _SCENES:
        return _SCENES[name]
    g = GEOMETRIES[name]
    (raw_y, raw_x), (H, W), (ph, pw) = g["raw"], g["image"], g["patch"]
    rng = np.random.default_rng(len(name) + 31)
    files = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in g["files"]]
    starts = np.cumsum([3] + [im.size for im in files])                  # (three bytes in front: no file starts at an aligned address)
    data = np.concatenate([np.zeros(3, np.uint8)] + [im.reshape(-1) for im in files])
    table, taps, full, source = [], [], [], []
    for f, im in enumerate(files):
        h, w = im.shape[:2]
        for row in g["rows"]:
            left, top, sx, sy, angle, RX, RY = image_geometry(w, h, row, raw_y, raw_x)
            rotated = np.float32(angle) != 0
            first = sum(len(t) for t in taps)
            taps += list(ii.ImageTaps(sx, sy, RX, RY))
            where = None
            if rotated:
                ox, oy = RX // 2 - raw_x // 2, RY // 2 - raw_y // 2
                adelta, bdelta, X0, Y0 = ii.RotationTables(RX, RY, angle)
                taps.append(np.stack([adelta[ox:ox + raw_x], bdelta[ox:ox + raw_x], np.full(raw_x, -7)], axis=1).astype(np.int32))
                taps.append(np.stack([X0[oy:oy + raw_y], Y0[oy:oy + raw_y], np.full(raw_y, -7)], axis=1).astype(np.int32))
                sy_, sx_, fy, fx = (v[oy:oy + raw_y, ox:ox + raw_x] for v in ii.RotationSource((adelta, bdelta, X0, Y0)))
                outside = ((sx_ < 0) | ((sx_ + 1 >= RX) & (fx != 0)) | (sx_ >= RX) | (sy_ < 0) | ((sy_ + 1 >= RY) & (fy != 0)) | (sy_ >= RY))
                where = (outside, (fx != 0) & (fy != 0))
            table.append([starts[f] + (top * w + left) * 3, sx, sy, RX, RY, first, w * 3, int(rotated), first + RX + RY, raw_x, raw_y])
            full.append(ii.TransformCrop(im[top:top + sy, left:left + sx], angle, raw_x, raw_y, (RX, RY)))
            source.append(where)
    N = g["cases"]
    cases, crops = np.zeros((N, 4), np.int32), np.zeros((N, 3 * H * W), np.uint8)
    border = both = 0
    for n in range(N):
        k = 1 if n < 10 else int(rng.integers(0, len(table)))            # one (rotated) image shared by the first ten cases: its positions
        if n < 10:
            left, top, mirrored = ii.Coordinates(raw_x, raw_y, n, H, W)
        else:
            left, top, mirrored = int(rng.integers(0, raw_x - W + 1)), int(rng.integers(0, raw_y - H + 1)), bool(rng.integers(0, 2))
        cases[n] = (k, left, top, mirrored)
        crops[n] = ii.PlanarCrop(full[k], left, top, H, W, mirrored)
        if source[k] is not None:
            border += int(source[k][0][top:top + H, left:left + W].sum())
            both += int(source[k][1][top:top + H, left:left + W].sum())
    dims = 3 * H * W
    s = dict(g, data=data, table=np.asarray(table, np.int64), taps=np.ascontiguousarray(np.concatenate(taps), np.int32), cases=cases,
             crops=crops, rotated=np.asarray(table)[:, 7] != 0, border=border, both=both,
             mean=(rng.random(dims) * 255).astype(np.float32), std=((rng.random(dims) + 0.5) * 60).astype(np.float32),
             wo=np.floor(rng.random(N) * (W - pw + 1)).astype(np.float32) + np.float32(0.25),
             ho=np.floor(rng.random(N) * (H - ph + 1)).astype(np.float32) + np.float32(0.25), flip=rng.random(N).astype(np.float32))
    if N > 1:
        s["wo"][:2], s["ho"][:2], s["flip"][:2] = (0.0, W - pw), (H - ph, 0.0), (0.9, 0.1)      # 0 and the maximum, both ways
    _SCENES[name] = s
    return s


def expect(name, crops, normalize, jitter, wo, ho, flip):
    """What the float pipeline leaves on ``crops`` (cases, 3 H W bytes): cast, (v - mean) / std in float32 with one rounding each, the
    patch at the truncated offsets, flipped above 0.5 — as (3, ph, pw, cases)."""
    s = scene(name)
    (H, W), (ph, pw) = s["image"], s["patch"]
    x = crops.astype(np.float32)
    if normalize:
        x = (x - s["mean"][None, :]) / s["std"][None, :]
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


def unrotated_cases(name):
    """The cases of the scene whose image is not rotated."""
    s = scene(name)
    return np.flatnonzero(~s["rotated"][s["cases"][:, 0]])
