"""CPU: video2hdf5 --host and the host mirror of RawVideoFileIterator — the frame counts and natural order of convnet_amd/video_iterators,
ResizeTo against a scalar restatement of include/convnet_hip.h's formula in int64, the dataset, boundary file and labels the tool writes,
that file read back as a sequence stream by the DataHandler, every refusal by its message, and the command line in a child process.  Three
videos of random bytes from a seed (tests/video_fixture.py).  Every comparison is exact equality; no GPU call is made."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import image_ref
import video_fixture
from convnet_amd import image_iterators, pbtxt, video2hdf5, video_iterators
from convnet_amd.datahandler import DataHandler
from convnet_amd.image_iterators import Bilinear, PlanarCrop, ResizeTo, Taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 10, 8                                # what the tool stretches every frame to
FRAMES = sum(video_fixture.COUNTS)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return video_fixture.write(tmp_path_factory.mktemp("videos"))


def _want(files, mirrored):
    return np.stack([PlanarCrop(ResizeTo(f, H, W), 0, 0, H, W, mirrored) for f in files["frames"]])


def scalar_resize(image, new_h, new_w):
    """h(y), then result, one byte at a time in int64 — the header's definition written out."""
    h, w = image.shape[:2]
    p = image.astype(np.int64)
    ct, rt = image_ref.taps(w, new_w), image_ref.taps(h, new_h)
    out = np.zeros((new_h, new_w, 3), np.uint8)

    def hrow(y, x, c):
        sx, a0, a1 = ct[x]
        return ((((2048 * ((p[y, sx, c] * a0 + p[y, min(sx + 1, w - 1), c] * a1) >> 4)) >> 16) + 2) >> 2)

    for y in range(new_h):
        sy, b0, b1 = rt[y]
        for x in range(new_w):
            for c in range(3):
                h0, h1 = hrow(sy, x, c), hrow(min(sy + 1, h - 1), x, c)
                out[y, x, c] = ((((b0 * ((2048 * h0) >> 4)) >> 16) + ((b1 * ((2048 * h1) >> 4)) >> 16) + 2) >> 2)
    return out


# ---- the iterator ---------------------------------------------------------------------------------------------------------------------------
def test_count_frames_and_natural_order(files):
    assert video_iterators.ReadVideoList(files["list"]) == files["videos"]
    assert video_iterators.CountFrames(files["videos"]) == video_fixture.COUNTS
    names = [os.path.basename(p) for p in video_iterators.FrameFiles(files["videos"][0])]
    assert names == [f"f_{i}.ppm" for i in range(1, 13)] and sorted(names) != names          # natural, not bytewise; no dot file, no directory
    order = sorted(["f_10.ppm", "f_2.ppm", "f_02.ppm", "a10b2", "a10b10", "a9", "10", "9"], key=video_iterators.NaturalKey)
    assert order == ["9", "10", "a9", "a10b2", "a10b10", "f_02.ppm", "f_2.ppm", "f_10.ppm"]   # (the tie f_02 / f_2 by the whole name)
    single = os.path.join(files["dir"], "single.pgm")
    image_ref.write_pgm(single, files["frames"][0][:, :, 0])
    assert video_iterators.CountFrames([single]) == [1]                                      # a single-frame file is a video of one frame
    assert np.array_equal(video_iterators.ReadFrames(single, 0, 1)[0][:, :, 2], files["frames"][0][:, :, 0])


def test_the_reader_hands_out_every_frame_in_list_and_frame_order(files):
    r = video_iterators.VideoReader(files["videos"])
    assert r.GetDataSetSize() == FRAMES and r.counts_ == video_fixture.COUNTS
    frames = r.Get(0, FRAMES)
    assert len(frames) == FRAMES and all(np.array_equal(a, b) for a, b in zip(frames, files["frames"]))
    span = r.Get(10, 19)                                                                     # across both borders between videos
    assert all(np.array_equal(a, b) for a, b in zip(span, files["frames"][10:19])) and len(span) == 9
    r.Seek(FRAMES - 1)
    assert np.array_equal(r.GetNext(), files["frames"][-1]) and r.Tell() == 0 and np.array_equal(r.GetNext(), files["frames"][0])
    r.SetMaxDataSetSize(14)
    assert r.GetDataSetSize() == 14
    with pytest.raises(IndexError):
        r.Get(13, 15)


# ---- the resize -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(7, 5, 66, 70), (66, 70, 7, 5), (7, 5, 7, 5), (1, 1, 4, 9)], ids=lambda g: "%dx%d-%dx%d" % g)
def test_resize_to_is_the_two_pass_definition(geometry):
    h, w, new_h, new_w = geometry
    image = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = ResizeTo(image, new_h, new_w)
    assert got.shape == (new_h, new_w, 3) and got.dtype == np.uint8
    assert np.array_equal(got, scalar_resize(image, new_h, new_w))
    one_pass = Bilinear(image, Taps(w, new_w), Taps(h, new_h))
    if (h, w) == (new_h, new_w):
        assert np.array_equal(got, image)                                                    # both passes are the identity
    elif h * w > 1:
        assert (got != one_pass).any()                                                       # the byte rounding between the passes shows
    else:
        assert (got == image[0, 0]).all()


# ---- the tool, --host -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [True, False], ids=["mirrored", "no_mirror"])
def test_host_rows_boundary_file_and_labels(files, mirror):
    out, bounds = os.path.join(files["dir"], f"host{int(mirror)}.h5"), os.path.join(files["dir"], f"bounds{int(mirror)}.txt")
    text = io.StringIO()
    info = video2hdf5.Video2HDF5(files["list"], out, W, H, boundary=bounds, labels=files["labels"], mirror=mirror, chunk=7, host=True, out=text)
    assert (info["videos"], info["frames"], info["dims"], info["path"], info["chunks"], info["launches"]) == (3, FRAMES, 3 * H * W, "host", 3, 0)
    assert info["seconds"] > 0 and info["load_wait_seconds"] == 0.0 and f"Frame {FRAMES} / {FRAMES}" in text.getvalue()
    data, labels = video_fixture.read(out)
    assert data.dtype == np.uint8 and np.array_equal(data, _want(files, mirror))
    assert not np.array_equal(data, _want(files, not mirror))
    assert open(bounds).read() == "12\n5\n3\n"
    assert np.array_equal(labels.reshape(-1), np.repeat(video_fixture.LABELS, video_fixture.COUNTS))
    plain = os.path.join(files["dir"], "plain.h5")
    before = set(os.listdir(files["dir"])) | {"plain.h5"}
    video2hdf5.Video2HDF5(files["list"], plain, W, H, mirror=mirror, host=True, out=io.StringIO())      # no flags: no boundary file, no labels
    data2, labels2 = video_fixture.read(plain)
    assert np.array_equal(data2, data) and labels2 is None and set(os.listdir(files["dir"])) == before


def test_the_output_is_a_sequence_stream_of_the_data_handler(files):
    out, bounds, T = os.path.join(files["dir"], "seq.h5"), os.path.join(files["dir"], "seq_bounds.txt"), 3
    video2hdf5.Video2HDF5(files["list"], out, W, H, boundary=bounds, labels=files["labels"], host=True, out=io.StringIO())
    seq = f'is_sequence: true seq_length: {T} boundary_file: "{bounds}"'
    text = (f'data_config {{ file_pattern: "{out}" layer_name: "input" dataset_name: "data" {seq} }}\n'
            f'data_config {{ file_pattern: "{out}" layer_name: "output" dataset_name: "labels" {seq} pick_first: true }}\n'
            "batch_size: 2\nchunk_size: 5\n")
    dh = DataHandler(pbtxt.parse(text, pbtxt.DatasetConfig), raw_chunks=False)
    starts = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 17]                                   # 12, 5 and 3 frames hold 10, 3 and 1 clips of 3
    assert dh.GetDataSetSize() == len(starts) and dh.streams_["input"].reader_.row_mapping_.tolist() == starts
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    want, frame_labels = _want(files, True), np.repeat(video_fixture.LABELS, video_fixture.COUNTS)
    for chunk in (starts[:5], starts[5:10], starts[10:] + starts[:1]):
        host = dh.DiskAccess()
        assert np.array_equal(host["input"], np.stack([want[f:f + T].reshape(-1) for f in chunk]).astype(np.float32))
        assert np.asarray(host["output"]).reshape(-1).tolist() == [frame_labels[f] for f in chunk]
    dh.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_has_its_own_message_and_nothing_is_written(files):
    d = files["dir"]
    out = os.path.join(d, "never.h5")

    def listing(name, *videos):
        path = os.path.join(d, name)
        with open(path, "w") as f:
            f.write("\n".join(videos) + "\n")
        return path

    empty_dir = os.path.join(d, "empty")
    os.makedirs(os.path.join(empty_dir, "sub"))
    movie = os.path.join(d, "movie.mp4")
    with open(movie, "wb") as f:
        f.write(b"\x00\x00\x00\x18ftypmp42" + bytes(64))
    short = os.path.join(d, "short_labels.txt")
    with open(short, "w") as f:
        f.write("1 2\n")
    run = lambda *a, **kw: video2hdf5.Video2HDF5(*a, **dict(dict(host=True, out=io.StringIO()), **kw))   # noqa: E731
    cases = [
        (lambda: run(listing("none.txt"), out), "lists no video"),
        (lambda: run(files["list"], out, width=0), "--width 0 is not a frame width"),
        (lambda: run(files["list"], out, height=-1), "--height -1 is not a frame height"),
        (lambda: run(files["list"], out, chunk=0), "--chunk 0 is not a number of frames"),
        (lambda: run(files["list"], out, labels=short), "2 labels for 3 listed files"),
        (lambda: run(files["list"], out, board="01", host=False), "2 boards ask for a model-parallel net, which is not built; name one board."),
        (lambda: run(files["list"], out, mean_file=os.path.join(d, "mean.h5")), "--mean-file is computed on the GPU path"),
        (lambda: run(listing("gone.txt", os.path.join(d, "gone")), out), f"Video {os.path.join(d, 'gone')} does not exist."),
        (lambda: run(listing("hollow.txt", empty_dir), out), f"Video directory {empty_dir} holds no frame file."),
        (lambda: run(listing("movie.txt", movie), out), "compressed video needs a decoder this package does not have; extract the frames"),
        (lambda: run(os.path.join(d, "nowhere.txt"), out), "Could not open data file : "),
    ]
    messages = []
    for call, word in cases:
        with pytest.raises(SystemExit) as e:
            call()
        assert word in str(e.value.code), (word, e.value.code)
        messages.append(str(e.value.code))
    assert movie in messages[-2] and len(set(messages)) == len(messages)
    assert not os.path.exists(out) and not os.path.exists(os.path.join(d, "mean.h5"))


def test_a_frame_that_fails_to_decode_stops_the_run_with_its_number(files):
    import shutil
    d = os.path.join(files["dir"], "broken_clip")
    shutil.copytree(files["videos"][0], d)
    broken = os.path.join(d, "f_3.ppm")
    with open(broken, "wb") as f:
        f.write(b"P6\n4 4\n255\nshort")
    listing = os.path.join(files["dir"], "broken.txt")
    with open(listing, "w") as f:
        f.write(d + "\n")
    with pytest.raises(SystemExit) as e:
        video2hdf5.Video2HDF5(listing, os.path.join(files["dir"], "broken.h5"), W, H, host=True, out=io.StringIO())
    assert e.value.code == f"Error reading file {broken} (frame 2)"


# ---- the command line -----------------------------------------------------------------------------------------------------------------------
def test_the_command_line_in_a_child_process(files, capsys):
    out, bounds = os.path.join(files["dir"], "cli.h5"), os.path.join(files["dir"], "cli_bounds.txt")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "convnet_amd.video2hdf5", "-i", files["list"], "-o", out, "--width", str(W), "--height", str(H),
           "--boundary", bounds, "--labels", files["labels"], "--host"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=files["dir"], env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"Frame {FRAMES} / {FRAMES}\n" in r.stdout and "mirrored as the reference's tool writes them" in r.stdout
    assert r.stdout.rstrip().endswith(out) and open(bounds).read() == "12\n5\n3\n"
    assert np.array_equal(video_fixture.read(out)[0], _want(files, True))
    r = subprocess.run(cmd + ["--no-mirror"], capture_output=True, text=True, cwd=files["dir"], env=env, timeout=300)
    assert r.returncode == 0 and "not mirrored" in r.stdout and np.array_equal(video_fixture.read(out)[0], _want(files, False))
    r = subprocess.run(cmd + ["--width", "0"], capture_output=True, text=True, cwd=files["dir"], env=env, timeout=300)
    assert r.returncode == 1 and "--width 0 is not a frame width." in r.stderr
    assert video2hdf5.main(["--output", out, "--host"]) == 1
    assert "usage: python -m convnet_amd.video2hdf5" in capsys.readouterr().out
