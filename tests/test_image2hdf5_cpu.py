"""CPU: convnet_amd.image2hdf5 with --host (numpy resize, no GPU call) against tests/image_ref.py (scalar loops) row for row; the produced
file read back through the data handler's disk half; labels; the refusals with their messages and exit codes; the command line in a
child process; and the byte RowWriter of hdf5io.  Every comparison is exact equality."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import image_ref
from convnet_amd import hdf5io, image2hdf5, pbtxt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIZE, CROP = 8, 6
# w x h: landscape, portrait, exactly the resize size, smaller than it (upscaled), grey, a side of 1 pixel (both ways), downscaled square
SIZES = [(13, 9), (9, 14), (8, 8), (5, 4), (11, 10), (1, 7), (12, 1), (20, 20)]
GREY = 4


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("image2hdf5")
    rng = np.random.default_rng(31)
    images, paths = [], []
    for i, (w, h) in enumerate(SIZES):
        if i == GREY:
            grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
            path = str(d / f"im{i}.pgm")
            image_ref.write_pgm(path, grey)
            image = np.repeat(grey[:, :, None], 3, axis=2)
        else:
            image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            path = str(d / f"im{i}.ppm")
            image_ref.write_ppm(path, image)
        images.append(image)
        paths.append(path)
    listing = str(d / "list.txt")
    with open(listing, "w") as f:
        f.write("\n".join(paths) + "\n")
    labels = str(d / "labels.txt")
    with open(labels, "w") as f:
        f.write(" ".join(str(7 * i - 3) for i in range(len(paths))) + "\n")
    want = np.stack([image_ref.row(im, RESIZE, RESIZE, CROP, CROP, 0) for im in images])      # computed once, shared, never changed
    return {"dir": str(d), "list": listing, "labels": labels, "paths": paths, "images": images, "want": want}


def _read(path, name="data"):
    with hdf5io.File(path) as f:
        r = f.RowReader(name)
        out = np.empty((r.GetDataSetSize(), r.GetDims()), r.GetStoredType())
        if out.dtype == np.uint8:
            r.Get(out, 0, len(out))
        else:
            out = np.empty(out.shape, np.float32)
            r.Get(out, 0, len(out))
        kind = r.GetStoredType()
        r.close()
    return out, kind


def test_host_rows_equal_the_scalar_reference_and_the_dataset_is_bytes(files):
    out = os.path.join(files["dir"], "host.h5")
    log = io.StringIO()
    info = image2hdf5.Image2HDF5(files["list"], out, CROP, RESIZE, chunk=3, host=True, out=log)
    assert info["files"] == len(SIZES) and info["dims"] == 3 * CROP * CROP and info["path"] == "host"
    got, kind = _read(out)
    assert kind == np.uint8 and got.shape == (len(SIZES), 3 * CROP * CROP)
    for i in range(len(SIZES)):
        assert np.array_equal(got[i], files["want"][i]), (i, SIZES[i])
    with hdf5io.File(out) as f:
        assert f.Has("data") and not f.Has("labels")
        assert f.ReadHDF5Shape("data") == (3 * CROP * CROP, len(SIZES))           # the (rows, cols) of the column-major matrix
    n = len(SIZES)
    assert log.getvalue() == "".join(f"\rImage {i + 1} / {n}" for i in range(n)) + "\n"
    # the chunk only groups the writes
    again = os.path.join(files["dir"], "host_one_chunk.h5")
    image2hdf5.Image2HDF5(files["list"], again, CROP, RESIZE, chunk=100, host=True, out=io.StringIO())
    assert np.array_equal(_read(again)[0], got)


def test_a_crop_smaller_than_the_resize_is_the_centre(files):
    out = os.path.join(files["dir"], "centre.h5")
    image2hdf5.Image2HDF5(files["list"], out, 3, RESIZE, host=True, out=io.StringIO())
    got, _ = _read(out)
    for i, im in enumerate(files["images"]):
        assert np.array_equal(got[i], image_ref.row(im, RESIZE, RESIZE, 3, 3, 0)), i


def test_a_byte_stream_over_the_file_gives_the_rows_of_the_image_stream(files):
    """The DataHandler's disk half only: the HDF5 stream over the produced file against the IMAGE_RAW float form over the files."""
    from convnet_amd.datahandler import DataHandler
    out = os.path.join(files["dir"], "stream.h5")
    image2hdf5.Image2HDF5(files["list"], out, CROP, RESIZE, labels=files["labels"], host=True, out=io.StringIO())
    n = len(SIZES)
    stored = pbtxt.parse(f'data_config {{ file_pattern: "{out}" layer_name: "input" dataset_name: "data" image_size: {CROP} num_colors: 3 }}\n'
                         f'data_config {{ file_pattern: "{out}" layer_name: "label" dataset_name: "labels" }}\n'
                         f'batch_size: 2 chunk_size: {n}', pbtxt.DatasetConfig)
    raw = pbtxt.parse(f'data_config {{ file_pattern: "{files["list"]}" layer_name: "input" data_type: IMAGE_RAW raw_image_size: {RESIZE} '
                      f'image_size: {CROP} }}\nbatch_size: 2 chunk_size: {n}', pbtxt.DatasetConfig)
    a, b = DataHandler(stored, raw_chunks=False), DataHandler(raw, raw_chunks=False)
    try:
        assert a.GetDataSetSize() == b.GetDataSetSize() == n
        assert a.streams_["input"].reader_.GetStoredType() == np.uint8
        chunk_a, chunk_b = a.DiskAccess(), b.DiskAccess()
        rows_a, rows_b = np.asarray(chunk_a["input"]), np.asarray(chunk_b["input"])
        assert rows_a.dtype == rows_b.dtype == np.float32 and rows_a.shape == (n, 3 * CROP * CROP)
        assert np.array_equal(rows_a, rows_b) and np.array_equal(rows_a, files["want"].astype(np.float32))
        # --labels round-trips through a label stream
        assert np.array_equal(np.asarray(chunk_a["label"]).reshape(-1), np.asarray([7 * i - 3 for i in range(n)], np.float32))
    finally:
        a.close()
        b.close()
    # the bytes form reads the same rows as stored
    c = DataHandler(stored)
    try:
        c.SetInputLayers(["input"])
        c.AllocateHostMemory(pinned=False)
        assert c.streams_["input"].raw_
        assert np.array_equal(np.asarray(c.DiskAccess()["input"]), files["want"])
    finally:
        c.close()
    labels, kind = _read(out, "labels")
    assert kind == np.int32 and labels.shape == (n, 1)


def test_refusals_their_messages_and_exit_codes(files, capsys):
    out = os.path.join(files["dir"], "refused.h5")
    with pytest.raises(SystemExit) as e:
        image2hdf5.main(["--input", files["list"], "--output", out, "--crop", "9", "--resize", "8", "--host"])
    assert e.value.code == "Crop size cannot be bigger than the resized image."
    with pytest.raises(SystemExit) as e:
        image2hdf5.Image2HDF5(files["list"], out, 9, 8, host=True)
    assert e.value.code == "Crop size cannot be bigger than the resized image."
    capsys.readouterr()
    for argv in (["--output", out, "--host"], ["--input", files["list"], "--host"], []):
        assert image2hdf5.main(argv) == 1
        assert "usage: python -m convnet_amd.image2hdf5" in capsys.readouterr().out
    broken = os.path.join(files["dir"], "broken.ppm")
    with open(broken, "wb") as f:
        f.write(b"P6\n4 4\n255\nshort")
    listing = os.path.join(files["dir"], "with_broken.txt")
    with open(listing, "w") as f:
        f.write(files["paths"][0] + "\n" + broken + "\n")
    with pytest.raises(SystemExit) as e:
        image2hdf5.Image2HDF5(listing, out, CROP, RESIZE, host=True, out=io.StringIO())
    assert e.value.code == f"Error reading file {broken}"
    with pytest.raises(SystemExit) as e:
        image2hdf5.Image2HDF5(files["list"], out, CROP, RESIZE, mean_file=os.path.join(files["dir"], "mean.h5"), host=True)
    assert "compute_mean" in str(e.value.code) and "--mean-file" in str(e.value.code)
    assert not os.path.exists(os.path.join(files["dir"], "mean.h5"))
    with pytest.raises(SystemExit, match="2 boards ask for a model-parallel net, which is not built; name one board."):
        image2hdf5.main(["--input", files["list"], "--output", out, "--board", "01"])
    with pytest.raises(SystemExit, match="Could not open data file : .*nowhere.txt"):
        image2hdf5.Image2HDF5(os.path.join(files["dir"], "nowhere.txt"), out, CROP, RESIZE, host=True)


def test_a_label_count_mismatch_names_both_counts_and_writes_no_file(files):
    out = os.path.join(files["dir"], "never.h5")
    short = os.path.join(files["dir"], "short_labels.txt")
    with open(short, "w") as f:
        f.write("1 2 3\n")
    with pytest.raises(SystemExit) as e:
        image2hdf5.Image2HDF5(files["list"], out, CROP, RESIZE, labels=short, host=True, out=io.StringIO())
    assert "3 labels" in str(e.value.code) and f"{len(SIZES)} listed files" in str(e.value.code)
    assert not os.path.exists(out)


def test_the_command_line_in_a_child_process(files):
    out = os.path.join(files["dir"], "cli.h5")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "convnet_amd.image2hdf5", "-i", files["list"], "-o", out, "-c", str(CROP), "-s", str(RESIZE),
                        "--labels", files["labels"], "--host"], capture_output=True, text=True, cwd=files["dir"], env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # (text mode reads the carriage returns of the progress line as newlines)
    assert f"Image {len(SIZES)} / {len(SIZES)}\n" in r.stdout and r.stdout.rstrip().endswith(out)
    assert np.array_equal(_read(out)[0], files["want"])
    r = subprocess.run([sys.executable, "-m", "convnet_amd.image2hdf5", "-i", files["list"], "-o", out, "-c", "9", "-s", "8", "--host"],
                       capture_output=True, text=True, cwd=files["dir"], env=env, timeout=300)
    assert r.returncode == 1 and "Crop size cannot be bigger than the resized image." in r.stderr


# ---- hdf5io: rows of bytes ------------------------------------------------------------------------------------------------------------------
def test_a_byte_row_writer_round_trips_and_refuses_what_does_not_fit(tmp_path):
    path = str(tmp_path / "rows.h5")
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 256, (7, 5), dtype=np.uint8)
    floats = rng.standard_normal((4, 3)).astype(np.float32)
    with hdf5io.File(path, "w") as f:
        w = f.CreateRows("bytes", 7, 5, np.uint8)
        w.WriteRows(rows[3:], 3)                              # out of order, in pieces
        w.WriteRows(rows[:1], 0)
        w.WriteRows(np.ascontiguousarray(rows[1:3]), 1)
        with pytest.raises(ValueError, match="dataset bytes: WriteRows needs a contiguous uint8 array of whole rows of 5"):
            w.WriteRows(rows.astype(np.float32), 0)
        with pytest.raises(ValueError, match="dataset bytes"):
            w.WriteRows(rows[:, :4], 0)                       # not contiguous
        with pytest.raises(IndexError, match="dataset bytes: rows 5:8 are not inside its 7 rows"):
            w.WriteRows(rows[:3], 5)
        with pytest.raises(IndexError):
            w.WriteRows(rows[:1], -1)
        w.close()
        v = f.CreateRows("floats", 4, 3)                      # the float default, its messages as they were
        v.WriteRows(floats, 0)
        with pytest.raises(ValueError, match="dataset floats: WriteRows needs a contiguous float32 array of whole rows of 3"):
            v.WriteRows(rows[:3, :3].copy(), 0)
        with pytest.raises(IndexError, match="dataset floats: rows 2:6 are not inside its 4 rows"):
            v.WriteRows(floats, 2)
        v.close()
        with pytest.raises(ValueError, match="dataset halves"):
            f.CreateRows("halves", 2, 2, np.float16)
    got, kind = _read(path, "bytes")
    assert kind == np.uint8 and np.array_equal(got, rows)
    got, kind = _read(path, "floats")
    assert kind == np.float32 and np.array_equal(got, floats)
