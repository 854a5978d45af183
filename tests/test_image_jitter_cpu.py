"""CPU: jitter_raw_image without a GPU — the random stream against a program built from <random> (tests/jitter_stream_main.cc), the crop
geometry, the rotation's written definition (include/convnet_hip.h: stage_images_jitter_u8), Transform, the data handler's float form
and the images-once disk half's tables on plain host buffers, and the config rules.  Exact unless stated."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_ref
from convnet_amd import hdf5io, pbtxt
from convnet_amd import image_iterators as ii
from convnet_amd.datahandler import DataHandler

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
BELOW_1 = np.nextafter(F(1), F(0))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the random stream ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler to build tests/jitter_stream_main.cc with"
    exe = str(tmp_path_factory.mktemp("stream") / "jitter_stream")
    subprocess.run([cxx, "-O2", "-std=c++11", os.path.join(HERE, "jitter_stream_main.cc"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("max_angle,min_scale", [(15, 1.5), (0, 1), (90, 1), (7.9, 3)])
def test_the_stream_is_the_default_random_engine_bit_for_bit(stream_program, max_angle, min_scale):
    lines = subprocess.run([stream_program, repr(max_angle), repr(min_scale)], capture_output=True, text=True, check=True).stdout.split("\n")
    want_draws = np.array([int(l, 16) for l in lines[:4096]], np.uint32)
    want_rows = np.array([[int(v, 16) for v in l.split()] for l in lines[4096:4096 + 64]], np.uint32)
    assert want_rows.shape == (64, 4)
    draws = ii.JitterStream().Draws(4096)
    assert draws.dtype == np.float32 and np.array_equal(_bits(draws), want_draws)
    assert 0 <= draws.min() and draws.max() < 1
    got = ii.JitterStream().Sample(64, max_angle, min_scale)
    assert all(v.dtype == np.float32 and v.shape == (64,) for v in got)
    assert np.array_equal(np.stack([_bits(v) for v in got], axis=1), want_rows)
    if max_angle == 7.9:                                                       # truncated to 7
        assert np.abs(got[0]).max() <= 7 and np.array_equal(_bits(got[0]), _bits(ii.JitterStream().Sample(64, 7, min_scale)[0]))
    if max_angle == 0:
        assert not got[0].any()
    if min_scale == 1:
        assert (got[3] == 1).all()


def test_the_worked_example():
    s = ii.JitterStream()
    angle, tx, ty, scale = (v[0] for v in s.Sample(4, 15, 1.5))
    assert (angle, tx, ty, scale) == (F(-14.9997654), F(0.131537795), F(0.75560534), F(1.27067494))
    assert ii.CropRect(500, 375, tx, ty, scale, 256, 256) == (26, 60, 295, 295)
    assert ii.RotSize(angle, 256, 256) == (313, 313) and 313 // 2 - 256 // 2 == 28
    t = float(abs(angle)) * 3.14159265 / 180
    assert F(np.sin(t) + np.cos(t)) == F(1.2247419)
    second = s.Sample(4, 15, 1.5)                                              # the stream goes on: the next chunk's entries differ
    assert second[0][0] != angle and second[1][0] != tx


def test_a_draw_that_rounds_to_one_is_the_float_below_one():
    s = ii.JitterStream()
    s.x_ = pow(16807, -1, 2147483647) * 2147483646 % 2147483647                # the state before x = 2^31 - 2, the largest
    u = s.Draws(1)[0]
    assert s.x_ == 2147483646 and u == BELOW_1 and u < 1


# ---- the crop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,tx,ty,scale,size_x,size_y,want", [
    (500, 375, 0.131537795, 0.75560534, 1.27067494, 256, 256, (26, 60, 295, 295)),     # the worked example
    (500, 375, 0.5, 0.5, 1.0, 256, 256, (62, 0, 375, 375)),                            # a wide file; scale exactly 1: no zoom
    (300, 400, 0.5, 0.5, 1.0, 256, 256, (0, 50, 300, 300)),                            # a tall file
    (48, 40, 0.7, 0.3, 1.0, 24, 20, (0, 0, 48, 40)),                                   # already at the raw aspect: nothing to translate
    (48, 40, 0.7, 0.3, 0.5, 24, 20, (0, 0, 48, 40)),                                   # a scale below 1 is ignored
    (48, 40, 0.7, 0.3, 2.0, 24, 20, (16, 6, 24, 20)),
    (37, 29, 0.0, 0.0, 1.5, 24, 20, (0, 0, 22, 19)),                                   # (24 * 29) // 20 = 34 -> 34 / 1.5 = 22.67; 29 / 1.5 = 19.33
    (37, 29, float(BELOW_1), float(BELOW_1), 1.5, 24, 20, (14, 9, 22, 19)),            # the float below 1: one short of the slack
    (500, 375, 0.0, 0.0, 1.0, 128, 256, (0, 0, 187, 375)),                             # non-square raw sizes, both rules
    (500, 375, float(BELOW_1), 0.5, 1.0, 256, 128, (0, 62, 500, 250)),
])
def test_crop_geometry(w, h, tx, ty, scale, size_x, size_y, want):
    got = ii.CropRect(w, h, tx, ty, scale, size_x, size_y)
    assert got == want
    left, top, sx, sy = got
    assert 0 <= left and left + sx <= w and 0 <= top and top + sy <= h


def test_transform_without_an_angle_is_the_resize_of_the_crop():
    image = np.random.default_rng(3).integers(0, 256, (29, 37, 3), dtype=np.uint8)
    for tx, ty, scale in ((0.5, 0.5, 1.0), (0.2, 0.9, 1.7), (0.0, float(BELOW_1), 3.0)):
        left, top, sx, sy = ii.CropRect(37, 29, tx, ty, scale, 24, 20)
        got = ii.Transform(image, 0.0, tx, ty, scale, 24, 20)
        crop = image[top:top + sy, left:left + sx]
        assert got.shape == (20, 24, 3) and np.array_equal(got, ii.ResizeTo(crop, 20, 24))
        assert np.array_equal(got, image_ref.height_pass(image_ref.width_pass(crop, 24), 20))       # the scalar restatement


# ---- the rotation -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 5, 33])
def test_quarter_turns_of_odd_squares_are_exact(size):
    image = np.random.default_rng(size).integers(0, 256, (size, size, 3), dtype=np.uint8)
    assert np.array_equal(ii.Rotate(image, 90), np.rot90(image))
    assert np.array_equal(ii.Rotate(image, -90), np.rot90(image, -1))
    assert np.array_equal(ii.Rotate(image, 180), image[::-1, ::-1])
    assert np.array_equal(ii.Rotate(image, -180), image[::-1, ::-1])


def test_rotation_tables_are_the_written_definition_in_scalars():
    """adelta / bdelta / X0 / Y0 once more, one value at a time with Python floats and round() (half to even), and one pixel by hand."""
    import math
    RX, RY, angle = 11, 7, 33.0
    a, b = math.cos(angle * (math.pi / 180)), math.sin(angle * (math.pi / 180))
    cx, cy = RX // 2, RY // 2
    M = [a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy]
    D = 1 / (M[0] * M[4] - M[1] * M[3])
    i0, i4, i1, i3 = M[4] * D, M[0] * D, -M[1] * D, -M[3] * D
    i2, i5 = -i0 * M[2] - i1 * M[5], -i3 * M[2] - i4 * M[5]
    adelta, bdelta, X0, Y0 = ii.RotationTables(RX, RY, angle)
    assert adelta.tolist() == [round(i0 * x * 1024) for x in range(RX)] and bdelta.tolist() == [round(i3 * x * 1024) for x in range(RX)]
    assert X0.tolist() == [round((i1 * y + i2) * 1024) + 16 for y in range(RY)]
    assert Y0.tolist() == [round((i4 * y + i5) * 1024) + 16 for y in range(RY)]
    image = np.random.default_rng(1).integers(0, 256, (RY, RX, 3), dtype=np.uint8)
    got = ii.Rotate(image, angle)
    R = lambda y, x, k: int(image[y, x, k]) if 0 <= y < RY and 0 <= x < RX else 0          # noqa: E731
    for y in range(RY):
        for x in range(RX):
            X, Y = (int(X0[y]) + int(adelta[x])) >> 5, (int(Y0[y]) + int(bdelta[x])) >> 5
            sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
            for k in range(3):
                want = ((32 - fx) * (32 - fy) * R(sy, sx, k) + fx * (32 - fy) * R(sy, sx + 1, k) + (32 - fx) * fy * R(sy + 1, sx, k)
                        + fx * fy * R(sy + 1, sx + 1, k) + 512) >> 10
                assert got[y, x, k] == want, (y, x, k)
    assert (got[0, 0] == 0).all()                                              # a corner of an oblong image turns in from the border


@pytest.mark.parametrize("angle", [-30, -14.9997654, -1, 0.3, 5, 15, 33, 45])
def test_rotated_ramp_stays_within_the_derived_bound_of_float64(angle):
    """0.5 input rounding + 0.5 output rounding + slope 2.25 x coordinate error (1/64 + 1/2048) = 1.036... < 1.1."""
    h, w = 61, 77
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = np.rint(1.5 * x + 0.75 * y + 3)
    assert ramp.max() < 256
    got = ii.Rotate(np.repeat(ramp.astype(np.uint8)[:, :, None], 3, axis=2), angle)
    assert (got[:, :, 0] == got[:, :, 1]).all() and (got[:, :, 0] == got[:, :, 2]).all()
    t = np.float64(F(angle)) * np.pi / 180
    a, b, cx, cy = np.cos(t), np.sin(t), w // 2, h // 2
    xs, ys = a * (x - cx) - b * (y - cy) + cx, b * (x - cx) + a * (y - cy) + cy      # the source point of (y, x): the inverse rotation
    inside = (xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2)
    assert inside.sum() > 0.5 * h * w
    error = np.abs(got[:, :, 0].astype(np.float64) - (1.5 * xs + 0.75 * ys + 3))[inside]
    print(f"angle {angle}: max error {error.max():.4f} over {inside.sum()} pixels")
    assert error.max() <= 1.1


def test_transform_with_an_angle_is_resize_rotate_and_the_central_window():
    image = np.random.default_rng(4).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    angle, tx, ty, scale = F(-14.9997654), F(0.3), F(0.6), F(1.27)
    left, top, sx, sy = ii.CropRect(64, 48, tx, ty, scale, 24, 20)
    RX, RY = ii.RotSize(angle, 24, 20)
    assert (RX, RY) == (int(F(24) * F(1.2247419)), int(F(20) * F(1.2247419))) == (29, 24)
    big = ii.Rotate(ii.ResizeTo(image[top:top + sy, left:left + sx], RY, RX), angle)
    want = big[RY // 2 - 10:RY // 2 + 10, RX // 2 - 12:RX // 2 + 12]
    assert np.array_equal(ii.Transform(image, angle, tx, ty, scale, 24, 20), want)
    assert ii.RotSize(90.0, 24, 20) == (24, 20) and ii.RotSize(45.0, 24, 20) == (33, 28)


# ---- the data handler on host buffers -----------------------------------------------------------------------------------------------------------
RAW_Y, RAW_X, SIZE_Y, SIZE_X = 20, 24, 16, 18
SIZES = [(37, 29), (29, 37), (64, 48), (50, 50), (41, 33), (30, 52), (45, 45)]
JITTER = "jitter_raw_image: true random_rotate_max_angle: 15 min_scale: 1.5"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("jitter")
    rng = np.random.default_rng(12)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in SIZES]
    paths = [str(d / f"im{i}.ppm") for i in range(len(images))]
    for p, im in zip(paths, images):
        image_ref.write_ppm(p, im)
    with open(str(d / "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    with hdf5io.File(str(d / "labels.h5"), "w") as f:
        f.WriteDataset("y", np.arange(7, dtype=np.float32))
        f.WriteDataset("y10", np.repeat(np.arange(7), 10).astype(np.float32))
    return dict(images=images, paths=paths, list=str(d / "list.txt"), labels=str(d / "labels.h5"))


def _config(files, stream=JITTER, extra="", labels="y"):
    text = (f'data_config {{ file_pattern: "{files["list"]}" layer_name: "input" data_type: IMAGE_RAW raw_image_size_y: {RAW_Y} '
            f'raw_image_size_x: {RAW_X} image_size_y: {SIZE_Y} image_size_x: {SIZE_X} {stream} }}\n')
    if labels:
        text += f'data_config {{ file_pattern: "{files["labels"]}" layer_name: "output" dataset_name: "{labels}" }}\n'
    return pbtxt.parse(text + f"batch_size: 2\n{extra}\n", pbtxt.DatasetConfig)


def _want_row(files, noise, f, position, chunk_size):
    angle, tx, ty, scale = (v[f % chunk_size] for v in noise)
    image = ii.Transform(files["images"][f], angle, tx, ty, scale, RAW_X, RAW_Y)
    assert image.shape == (RAW_Y, RAW_X, 3)
    left, top, mirrored = image_ref.coordinates(RAW_X, RAW_Y, position, SIZE_Y, SIZE_X)
    return image_ref.planar_crop(image, left, top, SIZE_Y, SIZE_X, mirrored)


def test_float_form_rows_are_transform_and_crop_and_every_chunk_draws_anew(files):
    dh = DataHandler(_config(files, extra="chunk_size: 5"), raw_chunks=False)
    stream, chunks = ii.JitterStream(), []
    for want in ([0, 1, 2, 3, 4], [5, 6, 0, 1, 2]):
        noise = stream.Sample(5, 15, 1.5)                                    # ONE draw per DiskAccess, though the second chunk is two pieces
        chunk = np.asarray(dh.DiskAccess()["input"]).copy()
        for i, f in enumerate(want):
            assert np.array_equal(chunk[i], _want_row(files, noise, f, 0, 5).astype(np.float32)), (want, i)
        chunks.append(chunk)
    assert not np.array_equal(chunks[0][0], chunks[1][2])                      # file 0 twice: entry 0 of two draws
    assert np.array_equal(np.asarray(dh.DiskAccess()["output"]).reshape(-1), [3, 4, 5, 6, 0])      # labels are untouched
    dh.close()


def test_float_form_under_randomize_cpu_avg10_and_the_thread_pool(files):
    dh = DataHandler(_config(files, extra="chunk_size: 5 randomize_cpu: true random_access_chunk_size: 2"), raw_chunks=False, seed=4)
    stream = ii.JitterStream()
    for _ in range(2):
        noise = stream.Sample(5, 15, 1.5)
        out = dh.DiskAccess()
        chunk, labels = np.asarray(out["input"]), np.asarray(out["output"]).reshape(-1).astype(int)
        for i, f in enumerate(labels):                                       # the file's row in the list picks the entry, not its place
            assert np.array_equal(chunk[i], _want_row(files, noise, f, 0, 5).astype(np.float32)), i
    dh.close()
    dh = DataHandler(_config(files, JITTER + " avg10_full_image: true", "chunk_size: 20", labels="y10"), raw_chunks=False)
    noise = ii.JitterStream().Sample(20, 15, 1.5)
    chunk = np.asarray(dh.DiskAccess()["input"])
    for row in range(20):                                                    # ten rows, one jitter
        assert np.array_equal(chunk[row], _want_row(files, noise, row // 10, row % 10, 20).astype(np.float32)), row
    assert dh.streams_["input"].reader_.num_reads_ == 2
    dh.close()
    serial = DataHandler(_config(files, extra="chunk_size: 5", labels=None), raw_chunks=False)
    pooled = DataHandler(_config(files, JITTER + " parallel_disk_access: true", "chunk_size: 5", labels=None), raw_chunks=False)
    for _ in range(2):
        assert np.array_equal(np.asarray(pooled.DiskAccess()["input"]), np.asarray(serial.DiskAccess()["input"]))
    serial.close()
    pooled.close()


def _image_from_tables(data, row, taps):
    """The raw-size image an 11-column image-table row describes (include/convnet_hip.h), by numpy from the tables alone."""
    at, w, h, new_w, new_h, first, stride, rotated, rot, win_w, win_h = (int(v) for v in row)
    view = np.lib.stride_tricks.as_strided(data[at:], (h, w, 3), (stride, 3, 1))
    wide = ii.Bilinear(view, taps[first:first + new_w], ii.Taps(h, h))                           # h(y): the width pass, rounded to a byte
    resized = ii.Bilinear(wide, ii.Taps(new_w, new_w), taps[first + new_w:first + new_w + new_h])
    if not rotated:
        assert rot == first + new_w + new_h
        return resized
    cols, rows = taps[rot:rot + win_w].astype(np.int64), taps[rot + win_w:rot + win_w + win_h].astype(np.int64)
    sy, sx, fy, fx = ii.RotationSource((cols[:, 0], cols[:, 1], rows[:, 0], rows[:, 1]))
    padded = np.zeros((new_h + 2, new_w + 2, 3), np.int64)
    padded[1:-1, 1:-1] = resized
    at = lambda y, x: padded[np.clip(y, -1, new_h) + 1, np.clip(x, -1, new_w) + 1]                 # noqa: E731
    fy, fx = fy[:, :, None], fx[:, :, None]
    return (((32 - fx) * (32 - fy) * at(sy, sx) + fx * (32 - fy) * at(sy, sx + 1) + (32 - fx) * fy * at(sy + 1, sx)
             + fx * fy * at(sy + 1, sx + 1) + 512) >> 10).astype(np.uint8)


@pytest.mark.parametrize("stream,angle", [(JITTER, 15), ("jitter_raw_image: true min_scale: 2", 0)], ids=["rotated", "unrotated"])
def test_images_once_tables_describe_the_same_geometry(files, stream, angle):
    dh = DataHandler(_config(files, stream, extra="chunk_size: 5"))
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    half = dh.disk_.halves_["input"]
    assert type(half).__name__ == "_ImagesDisk" and half.image_table_[0].shape == (5, 11)
    jitter = ii.JitterStream()
    for want in ([0, 1, 2, 3, 4], [5, 6, 0, 1, 2]):
        noise = jitter.Sample(5, angle, float(stream.split()[-1]))
        dh.DiskAccess()
        data, table, taps, cases = half.Used(0)
        assert len(table) == 5 and (table[:, 7] != 0).all() == (angle != 0)
        offset = 0
        for k, f in enumerate(want):
            image = files["images"][f]
            assert np.array_equal(data[offset:offset + image.size], image.reshape(-1))       # the whole file, at its original size
            a, tx, ty, scale = (v[f % 5] for v in noise)
            left, top, sx, sy = ii.CropRect(image.shape[1], image.shape[0], tx, ty, scale, RAW_X, RAW_Y)
            assert table[k, :3].tolist() == [offset + (top * image.shape[1] + left) * 3, sx, sy] and table[k, 6] == image.shape[1] * 3
            assert table[k, 3:5].tolist() == (list(ii.RotSize(a, RAW_X, RAW_Y)) if angle else [RAW_X, RAW_Y])
            assert np.array_equal(_image_from_tables(data, table[k], taps), ii.Transform(image, a, tx, ty, scale, RAW_X, RAW_Y)), (want, k)
            assert cases[k].tolist() == [k, *image_ref.coordinates(RAW_X, RAW_Y, 0, SIZE_Y, SIZE_X)[:2], 0]
            offset += image.size
        assert half.bytes_used_[0] == offset and half.taps_used_[0] == int(table[-1, 8]) + (RAW_X + RAW_Y if angle else 0)
    dh.close()


def test_an_unjittered_stream_keeps_its_six_column_table(files):
    dh = DataHandler(_config(files, "", extra="chunk_size: 5"))
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    dh.DiskAccess()
    assert dh.disk_.halves_["input"].image_table_[0].shape == (5, 6) and dh.streams_["input"].reader_.noise_ is None
    dh.close()


# ---- the config rules -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream,words", [
    ("random_rotate_max_angle: 10", ["random_rotate_max_angle 10 without jitter_raw_image", "ignores"]),
    ("min_scale: 1.5", ["min_scale 1.5 without jitter_raw_image", "ignores"]),
    ("jitter_raw_image: true", ["jitter_raw_image with min_scale 0", "every drawn scale would be ignored", "min_scale: 1 gives translation and rotation alone"]),
    ("jitter_raw_image: true min_scale: 0.99 random_rotate_max_angle: 5", ["jitter_raw_image with min_scale 0.99", "every drawn scale would be ignored"]),
    ("jitter_raw_image: true min_scale: 1 random_rotate_max_angle: 91", ["random_rotate_max_angle 91", "beyond 90 degrees"]),
    ('jitter_raw_image: true min_scale: 1 bbox_file: "boxes.txt"', ["bbox_file"]),
])
def test_the_kept_refusals(files, stream, words):
    with pytest.raises(SystemExit) as e:
        DataHandler(_config(files, stream, labels=None))
    message = str(e.value)
    assert message.startswith("Data stream for layer input: ") and all(w in message for w in words), message
    if stream.startswith("jitter_raw_image: true") and "min_scale 0" in message:
        assert message.startswith("Data stream for layer input: jitter_raw_image")


@pytest.mark.parametrize("stream,extra,labels", [
    ("jitter_raw_image: true min_scale: 1", "", "y"),
    ("jitter_raw_image: true min_scale: 1 random_rotate_max_angle: 90", "chunk_size: 4 randomize_gpu: true", "y"),
    (JITTER + " avg10_full_image: true", "chunk_size: 20", "y10"),
    (JITTER + " parallel_disk_access: true", "chunk_size: 4 pipeline_loads: true", "y"),
    (JITTER + " can_translate: true can_flip: true gpu_image_size_y: 12 gpu_image_size_x: 14", "chunk_size: 4 randomize_cpu: true multiplicity: 3", "y"),
])
def test_the_accepted_combinations(files, stream, extra, labels):
    for raw in (True, False):
        dh = DataHandler(_config(files, stream, extra, labels), raw_chunks=raw)
        dh.SetInputLayers(["input"])
        r = dh.streams_["input"].reader_
        assert r.jitter_ and r.min_scale_ >= 1 and dh.streams_["input"].raw_ is raw
        out = dh.DiskAccess()
        assert r.noise_ is not None and len(r.noise_[0]) == dh.chunk_size_ and out["input"] is not None
        dh.close()
