"""CPU: the IMAGE_RAW stream without a GPU — taps and the 8-bit resize against tests/image_ref.py (scalar loops, no shared code) and the
values pinned in include/convnet_hip.h's definition, positions, the row -> (file, position) mapping, the decoders, the file list, every
refusal, and the images-once disk half on plain host buffers.  All comparisons are exact."""
import numpy as np
import pytest

import image_ref
from convnet_amd import hdf5io, pbtxt
from convnet_amd import image_iterators as ii
from convnet_amd.datahandler import DataHandler

SIZES = [(1, 6), (6, 1), (7, 5), (5, 9), (13, 4)]      # w x h
RAW = [(4, 6), (6, 4), (8, 8)]                         # raw y x raw x


def _image(w, h, seed=0):
    return np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the resize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,dsize,want,want_taps", [
    ([0, 100, 200, 50], 6, [0, 50, 117, 183, 125, 50], [(0, 2048, 0), (0, 1024, 1024), (1, 1707, 341), (1, 341, 1707), (2, 1024, 1024), (3, 2048, 0)]),
    ([10, 250], 5, [10, 34, 130, 226, 250], None),
    ([0, 100, 200, 50, 255], 3, [33, 200, 187], None)])
def test_pinned_rows(row, dsize, want, want_taps):
    assert image_ref.resize_row(row, dsize) == want
    taps = ii.Taps(len(row), dsize)
    assert [tuple(t) for t in taps.tolist()] == image_ref.taps(len(row), dsize)
    if want_taps:
        assert [tuple(t) for t in taps.tolist()] == want_taps
    image = np.repeat(np.asarray(row, np.uint8)[None, :, None], 3, axis=2)          # one row, three equal colours
    got = ii.Bilinear(image, taps, ii.Taps(1, 1))
    assert got.shape == (1, dsize, 3) and all(got[0, :, k].tolist() == want for k in range(3))


def test_a_pass_that_keeps_its_size_is_the_identity_on_every_byte():
    values = np.arange(256, dtype=np.uint8)
    assert [tuple(t) for t in ii.Taps(256, 256).tolist()] == [(i, 2048, 0) for i in range(256)]
    assert image_ref.resize_row(values, 256) == values.tolist()
    image = np.repeat(values[None, :, None], 3, axis=2)
    assert np.array_equal(ii.Bilinear(image, ii.Taps(256, 256), ii.Taps(1, 1)), image)
    assert np.array_equal(ii.Bilinear(image.transpose(1, 0, 2), ii.Taps(1, 1), ii.Taps(256, 256)), image.transpose(1, 0, 2))
    assert np.array_equal(image_ref.height_pass(image.transpose(1, 0, 2), 256), image.transpose(1, 0, 2))


def test_the_vectorised_resize_equals_the_scalar_restatement():
    seen = set()
    for w, h in SIZES:
        for raw_y, raw_x in RAW:
            image = _image(w, h)
            want = image_ref.resize(image, raw_y, raw_x)
            got = ii.Resize(image, raw_y, raw_x)
            assert got.shape == want.shape and np.array_equal(got, want), (w, h, raw_y, raw_x)
            new_w, new_h = ii.ResizedSize(w, h, raw_y, raw_x)
            assert (new_w, new_h) == image_ref.resized_size(w, h, raw_y, raw_x) == (got.shape[1], got.shape[0])
            assert (new_w == raw_x and new_h >= raw_y) or (new_h == raw_y and new_w >= raw_x)      # it covers the raw size, one side exactly
            seen.add(("height_rule" if raw_x * h < raw_y * w else "width_rule", "same" if got is image else
                      ("up" if new_w * new_h > w * h else "down")))
            if got is image:
                assert (new_w, new_h) == (w, h)
    assert {("height_rule", "same"), ("height_rule", "up"), ("width_rule", "up")} <= seen
    big = _image(40, 23)                                                            # and down, on both rules
    for raw_y, raw_x in ((5, 4), (4, 20)):
        assert np.array_equal(ii.Resize(big, raw_y, raw_x), image_ref.resize(big, raw_y, raw_x))


def test_image_taps_are_the_two_passes_seen_from_the_destination():
    """What stage_images_u8 is given: a pixel of the resized image from the column tap and the row tap alone."""
    image = _image(7, 5)
    want = image_ref.resize(image, 8, 8)
    new_w, new_h = ii.ResizedSize(7, 5, 8, 8)
    cols, rows = ii.ImageTaps(7, 5, new_w, new_h)
    assert cols.shape == (new_w, 3) and rows.shape == (new_h, 3) and cols.dtype == rows.dtype == np.int32
    p = image.astype(int)
    for y in range(new_h):
        for x in range(new_w):
            (sx, a0, a1), (sy, b0, b1) = cols[x].tolist(), rows[y].tolist()
            def hpass(yy):
                return (((2048 * ((p[yy, sx] * a0 + p[yy, min(sx + 1, 6)] * a1) >> 4)) >> 16) + 2) >> 2
            got = (((b0 * ((2048 * hpass(sy)) >> 4)) >> 16) + ((b1 * ((2048 * hpass(min(sy + 1, 4))) >> 4)) >> 16) + 2) >> 2
            assert got.tolist() == want[y, x].tolist()


# ---- positions, rows ------------------------------------------------------------------------------------------------------------------------
def test_all_ten_positions():
    width, height, sy, sx = 9, 7, 4, 5
    want = [(2, 1), (0, 0), (4, 0), (4, 3), (0, 3)]
    image = _image(width, height)
    for position in range(10):
        left, top, mirrored = ii.Coordinates(width, height, position, sy, sx)
        assert (left, top, mirrored) == (*want[position % 5], position >= 5) == image_ref.coordinates(width, height, position, sy, sx)
        crop = ii.PlanarCrop(image, left, top, sy, sx, mirrored)
        assert crop.dtype == np.uint8 and np.array_equal(crop, image_ref.planar_crop(image, left, top, sy, sx, mirrored))
        planes = crop.reshape(3, sy, sx)
        cols = left + (np.arange(sx)[::-1] if mirrored else np.arange(sx))
        assert np.array_equal(planes, image[top:top + sy][:, cols].transpose(2, 0, 1))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("images")
    images, paths = [], []
    for i, (w, h) in enumerate([(9, 7), (6, 8), (13, 4), (5, 9), (8, 8), (7, 5), (10, 6)]):
        image = _image(w, h, seed=i)
        if i == 3:                                     # a grey file: three equal planes
            image = np.repeat(image[:, :, :1], 3, axis=2)
            image_ref.write_pgm(str(d / f"im{i}.pgm"), image[:, :, 0])
            paths.append(str(d / f"im{i}.pgm"))
        else:
            image_ref.write_ppm(str(d / f"im{i}.ppm"), image)
            paths.append(str(d / f"im{i}.ppm"))
        images.append(image)
    listing = str(d / "list.txt")
    with open(listing, "w") as f:
        f.write(paths[0] + " " + paths[1] + "\n\n" + "\n".join(paths[2:]) + "\n")
    labels = str(d / "labels.h5")
    with hdf5io.File(labels, "w") as f:
        f.WriteDataset("y", np.arange(7, dtype=np.float32))
        f.WriteDataset("y10", np.repeat(np.arange(7), 10).astype(np.float32))
    return {"dir": d, "images": images, "paths": paths, "list": listing, "labels": labels}


RAW_Y, RAW_X, SIZE_Y, SIZE_X = 4, 6, 3, 4


def _config(files, stream="", extra="", labels="y", listing=None):
    text = (f'data_config {{ file_pattern: "{listing or files["list"]}" layer_name: "input" data_type: IMAGE_RAW raw_image_size_y: {RAW_Y} '
            f'raw_image_size_x: {RAW_X} image_size_y: {SIZE_Y} image_size_x: {SIZE_X} {stream} }}\n')
    if labels:
        text += f'data_config {{ file_pattern: "{files["labels"]}" layer_name: "output" dataset_name: "{labels}" }}\n'
    return pbtxt.parse(text + f"batch_size: 2\n{extra}\n", pbtxt.DatasetConfig)


def _want_row(files, f, position):
    return image_ref.row(files["images"][f], RAW_Y, RAW_X, SIZE_Y, SIZE_X, position)


def test_the_file_list_reader(files, tmp_path):
    assert ii.ReadFileList(files["list"]) == files["paths"]
    with pytest.raises(SystemExit, match="Could not open data file : .*nowhere.txt"):
        ii.ReadFileList(str(tmp_path / "nowhere.txt"))


def test_dataset_size_and_row_mapping(files):
    for stream, extra, labels, positions, nfiles in (("", "", "y", 1, 7), ("avg10_full_image: true", "", "y10", 10, 7),
                                                     ("avg10_full_image: true", "max_dataset_size: 3", None, 10, 3),
                                                     ("", "max_dataset_size: 5", None, 1, 5)):
        dh = DataHandler(_config(files, stream, extra, labels), raw_chunks=False)
        r = dh.streams_["input"].reader_
        assert dh.GetDataSetSize() == positions * nfiles == r.GetDataSetSize() and r.GetDims() == 3 * SIZE_Y * SIZE_X
        for row in (0, 1, positions, positions * nfiles - 1):
            assert r.FileAndPosition(row) == (row // positions, row % positions)
        chunk = np.asarray(dh.DiskAccess()["input"])                         # the float form's host chunk: the whole dataset
        assert chunk.dtype == np.float32 and chunk.shape == (positions * nfiles, 3 * SIZE_Y * SIZE_X)
        for row in range(positions * nfiles):
            assert np.array_equal(chunk[row], _want_row(files, row // positions, row % positions).astype(np.float32)), row
        assert r.num_reads_ == nfiles                                        # every file decoded once for its ten rows
        dh.close()


def test_sequential_float_chunks_wrap(files):
    dh = DataHandler(_config(files, extra="chunk_size: 5"), raw_chunks=False)
    for want in ([0, 1, 2, 3, 4], [5, 6, 0, 1, 2], [3, 4, 5, 6, 0]):
        chunk = np.asarray(dh.DiskAccess()["input"])
        for i, f in enumerate(want):
            assert np.array_equal(chunk[i], _want_row(files, f, 0).astype(np.float32))
    dh.close()


# ---- decoding -------------------------------------------------------------------------------------------------------------------------------
def test_the_pnm_parser_against_pil(files):
    from PIL import Image
    for path, image in zip(files["paths"], files["images"]):
        got = ii.ReadImage(path)
        assert got.dtype == np.uint8 and np.array_equal(got, image)
        assert np.array_equal(got, np.asarray(Image.open(path).convert("RGB")))
    assert ii.DecodePNM(b"P3\n1 1\n255\n0 0 0\n") is None and ii.DecodePNM(b"P6\n2 2\n255\n" + bytes(11)) is None      # ASCII; a short raster
    assert ii.DecodePNM(b"P6\n1 1\n65535\n" + bytes(6)) is None


def test_other_formats_decode_as_pil_does(tmp_path):
    from PIL import Image
    rgb = _image(11, 6)
    rgba = np.concatenate([rgb, np.full((6, 11, 1), 77, np.uint8)], axis=2)
    cases = {"a.png": Image.fromarray(rgb), "b.jpg": Image.fromarray(rgb), "c.png": Image.fromarray(rgba),
             "d.png": Image.fromarray(rgb).convert("P", palette=Image.Palette.ADAPTIVE, colors=16), "e.png": Image.fromarray(np.ascontiguousarray(rgb[:, :, 0]))}
    for name, im in cases.items():
        path = str(tmp_path / name)
        im.save(path)
        want = np.asarray(Image.open(path).convert("RGB"))
        got = ii.ReadImage(path)
        assert got.shape == (6, 11, 3) and got.dtype == np.uint8 and np.array_equal(got, want), name
    assert np.array_equal(ii.ReadImage(str(tmp_path / "a.png")), rgb) and np.array_equal(ii.ReadImage(str(tmp_path / "c.png")), rgb)
    assert np.array_equal(ii.ReadImage(str(tmp_path / "e.png")), np.repeat(rgb[:, :, :1], 3, axis=2))
    got = ii.ReadImages([str(tmp_path / n) for n in cases], parallel=True)
    assert all(np.array_equal(a, ii.ReadImage(str(tmp_path / n))) for a, n in zip(got, cases))


def test_an_unreadable_file_stops_the_run_through_the_preload_thread(files, tmp_path):
    bad = str(tmp_path / "broken.ppm")
    with open(bad, "wb") as f:
        f.write(b"not an image")
    with pytest.raises(SystemExit, match="Error reading file .*broken.ppm"):
        ii.ReadImage(bad)
    with pytest.raises(SystemExit, match="Error reading file .*missing.jpg"):
        ii.ReadImage(str(tmp_path / "missing.jpg"))
    listing = str(tmp_path / "list.txt")
    with open(listing, "w") as f:
        f.write(files["paths"][0] + "\n" + bad + "\n")
    for raw in (True, False):
        dh = DataHandler(_config(files, extra="pipeline_loads: true", labels=None, listing=listing), raw_chunks=raw)
        dh.SetInputLayers(["input"])
        dh.StartPreload()
        with pytest.raises(SystemExit, match="Error reading file .*broken.ppm"):
            dh.Sync()
        dh.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("jitter_raw_image: true", "", "jitter_raw_image"), ("random_rotate_max_angle: 10", "", "random_rotate_max_angle"),
    ("min_scale: 0.5", "", "min_scale"), ('bbox_file: "boxes.txt"', "", "bbox_file"), ("num_colors: 1", "", "num_colors 1"),
    ("is_sequence: true seq_length: 2", "", "is_sequence is not supported on an IMAGE_RAW stream"),
    ("image_size_y: 5", "", "image_size 5 x 4 exceeds raw_image_size 4 x 6"), ("image_size_x: 7", "", "image_size 3 x 7 exceeds raw_image_size"),
    ("avg10_full_image: true", "randomize_cpu: true", "avg10_full_image together with randomize_cpu"),
    ("avg10_full_image: true parallel_disk_access: true", "", "avg10_full_image together with parallel_disk_access"),
    ("raw_image_size_y: 0", "", "data_type IMAGE_RAW without a raw_image_size")]


@pytest.mark.parametrize("stream,extra,message", REFUSALS, ids=[r[2].split()[0] + str(i) for i, r in enumerate(REFUSALS)])
def test_refusals_name_the_layer_and_the_field(files, stream, extra, message):
    with pytest.raises(SystemExit) as e:
        DataHandler(_config(files, stream, extra, labels=None))
    assert message in str(e.value) and str(e.value).startswith("Data stream for layer input: "), str(e.value)


def test_refusal_messages_are_all_different_and_the_last_keeps_its_wording(files):
    messages = set()
    for stream, extra, _ in REFUSALS:
        with pytest.raises(SystemExit) as e:
            DataHandler(_config(files, stream, extra, labels=None))
        messages.add(str(e.value))
    assert len(messages) == len(REFUSALS)
    cfg = pbtxt.parse(f'data_config {{ file_pattern: "{files["list"]}" layer_name: "pixels" data_type: IMAGE_RAW image_size: 4 }}', pbtxt.DatasetConfig)
    with pytest.raises(SystemExit, match=r"^Data stream for layer pixels: data_type IMAGE_RAW .* is not supported"):
        DataHandler(cfg)
    with pytest.raises(SystemExit, match="data_type DUMMY"):                     # the other types keep their refusal
        DataHandler(pbtxt.parse('data_config { layer_name: "pixels" data_type: DUMMY }', pbtxt.DatasetConfig))


def test_compute_mean_refuses_an_image_stream_by_name(files):
    from convnet_amd import compute_mean
    with pytest.raises(SystemExit, match="layer input: compute_mean does not take an IMAGE_RAW stream"):
        compute_mean.ComputeMean(_config(files, labels=None), "input", 3)


# ---- the images-once disk half, no GPU call ---------------------------------------------------------------------------------------------------
def _once(files, stream="", extra="", labels=None):
    dh = DataHandler(_config(files, stream, extra, labels))
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    half = dh.disk_.halves_["input"]
    assert type(half).__name__ == "_ImagesDisk" and dh.streams_["input"].raw_
    return dh, half


def _check_chunk(files, dh, half, want_rows, positions=1, buf=0):
    """Offsets, tables and used bytes of the chunk in host buffer ``buf``: cases ``want_rows`` (stream rows), every file once."""
    data = dh.host_[buf]["input"]
    assert data.dtype == np.uint8 and data.ndim == 1
    order = []
    for row in want_rows:
        if row // positions not in order:
            order.append(row // positions)
    assert half.images_used_[buf] == len(order)
    offset = tap = 0
    for k, f in enumerate(order):
        image = files["images"][f]
        h, w = image.shape[:2]
        new_w, new_h = image_ref.resized_size(w, h, RAW_Y, RAW_X)
        assert half.image_table_[buf][k].tolist() == [offset, w, h, new_w, new_h, tap]
        assert np.array_equal(data[offset:offset + image.size], image.reshape(-1))         # interleaved R, G, B rows at the original size
        taps = half.taps_[buf][tap:tap + new_w + new_h]
        assert [tuple(t) for t in taps.tolist()] == image_ref.taps(w, new_w) + image_ref.taps(h, new_h)
        offset, tap = offset + image.size, tap + new_w + new_h
    assert (half.bytes_used_[buf], half.taps_used_[buf]) == (offset, tap)
    for i, row in enumerate(want_rows):
        f, position = divmod(row, positions)
        image = files["images"][f]
        new_w, new_h = image_ref.resized_size(image.shape[1], image.shape[0], RAW_Y, RAW_X)
        left, top, mirrored = image_ref.coordinates(new_w, new_h, position, SIZE_Y, SIZE_X)
        assert half.case_table_[buf][i].tolist() == [order.index(f), left, top, int(mirrored)], (i, row)


def test_images_once_chunks_tables_and_the_wrap(files):
    dh, half = _once(files, extra="chunk_size: 5")
    assert dh.host_[0]["input"].shape == (5 * RAW_Y * RAW_X * 3 * 2,)
    for want in ([0, 1, 2, 3, 4], [5, 6, 0, 1, 2], [3, 4, 5, 6, 0]):
        dh.DiskAccess()
        _check_chunk(files, dh, half, want)
    dh.close()


def test_images_once_shares_a_file_among_its_ten_positions(files):
    dh, half = _once(files, "avg10_full_image: true", "chunk_size: 25")
    dh.DiskAccess()
    _check_chunk(files, dh, half, list(range(25)), positions=10)
    assert half.images_used_[0] == 3 and dh.streams_["input"].reader_.num_reads_ == 3
    dh.DiskAccess()
    _check_chunk(files, dh, half, list(range(25, 50)), positions=10)          # file 2 again: its last five positions
    dh.DiskAccess()
    _check_chunk(files, dh, half, list(range(50, 70)) + list(range(5)), positions=10)
    dh.close()


def test_images_once_under_randomize_cpu(files):
    dh, half = _once(files, extra="chunk_size: 5 randomize_cpu: true random_access_chunk_size: 2")
    for _ in range(3):
        dh.DiskAccess()
        cases = half.case_table_[0][:, 0].tolist()
        table = half.image_table_[0][:half.images_used_[0]]
        found = []
        for k in cases:                                                      # which file each case's image is
            offset, w, h = table[k][:3].tolist()
            found.append([i for i, im in enumerate(files["images"]) if im.shape[:2] == (h, w)
                          and np.array_equal(dh.host_[0]["input"][offset:offset + im.size], im.reshape(-1))][0])
        assert found[1] == (found[0] + 1) % 7 and found[3] == (found[2] + 1) % 7      # runs of 2, the last cut at the chunk's end
        _check_chunk(files, dh, half, found)
    dh.close()


def test_images_once_buffers_grow_at_twice_the_need(files, tmp_path):
    big = _image(40, 30, seed=9)
    image_ref.write_ppm(str(tmp_path / "big.ppm"), big)
    listing = str(tmp_path / "list.txt")
    with open(listing, "w") as f:
        f.write("\n".join([files["paths"][0], str(tmp_path / "big.ppm"), files["paths"][1]]))       # no newline at the end: the last file counts
    dh = DataHandler(_config(files, extra="chunk_size: 2 pipeline_loads: true", labels=None, listing=listing))
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    half = dh.disk_.halves_["input"]
    start = 2 * RAW_Y * RAW_X * 3 * 2
    assert dh.GetDataSetSize() == 3 and [h["input"].size for h in dh.host_] == [start, start]
    dh.StartPreload()
    dh.Sync()
    buf = dh.pending_
    first, need = files["images"][0], files["images"][0].size + big.size
    assert need > start and dh.host_[buf]["input"].size == 2 * need and half.bytes_[buf] is dh.host_[buf]["input"]
    assert dh.host_[1 - buf]["input"].size == start                              # the other buffer is as it was
    assert half.bytes_used_[buf] == need
    assert np.array_equal(dh.host_[buf]["input"][:first.size], first.reshape(-1))
    assert np.array_equal(dh.host_[buf]["input"][first.size:need], big.reshape(-1))
    assert half.image_table_[buf][1].tolist()[:3] == [first.size, 40, 30]
    taps_need = sum(sum(image_ref.resized_size(im.shape[1], im.shape[0], RAW_Y, RAW_X)) for im in (first, big))
    assert half.taps_used_[buf] == taps_need and len(half.taps_[buf]) >= taps_need
    dh.close()


def test_the_thread_pool_fills_the_same_buffer_as_the_serial_path(files):
    assert ii.MAX_DECODE_THREADS == 8
    serial, half_s = _once(files, extra="chunk_size: 5")
    pooled, half_p = _once(files, "parallel_disk_access: true", "chunk_size: 5")
    assert pooled.streams_["input"].reader_.parallel_ and not serial.streams_["input"].reader_.parallel_
    for _ in range(3):
        serial.DiskAccess()
        pooled.DiskAccess()
        used = half_s.bytes_used_[0]
        assert half_p.bytes_used_[0] == used and np.array_equal(pooled.host_[0]["input"][:used], serial.host_[0]["input"][:used])
        for name in ("image_table_", "case_table_"):
            assert np.array_equal(getattr(half_p, name)[0], getattr(half_s, name)[0])
        assert np.array_equal(half_p.taps_[0][:half_p.taps_used_[0]], half_s.taps_[0][:half_s.taps_used_[0]])
    serial.close()
    pooled.close()
    floats_s = DataHandler(_config(files, extra="chunk_size: 5", labels=None), raw_chunks=False)
    floats_p = DataHandler(_config(files, "parallel_disk_access: true", "chunk_size: 5", labels=None), raw_chunks=False)
    assert np.array_equal(np.asarray(floats_p.DiskAccess()["input"]), np.asarray(floats_s.DiskAccess()["input"]))
    floats_s.close()
    floats_p.close()
