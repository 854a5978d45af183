"""GPU: convnet_amd.video2hdf5 end to end on the three videos of tests/video_fixture.py — the GPU path (a decode thread, one upload per
chunk, resize_frames_u8 per run of equal geometry, pinned downloads, the writer thread) against --host (numpy on the host), byte for byte
with the labels; --mean-file against compute_mean on the produced file, dataset for dataset and bit for bit; video_small trained from the
output and its boundary file through the DataHandler; the command line in a child process."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import video_fixture  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 10, 8
FRAMES = sum(video_fixture.COUNTS)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from convnet_amd import video2hdf5
    f = video_fixture.write(tmp_path_factory.mktemp("video2hdf5_gpu"))
    for mirror in (True, False):                                      # the comparison legs, once
        path = os.path.join(f["dir"], f"host{int(mirror)}.h5")
        video2hdf5.Video2HDF5(f["list"], path, W, H, labels=f["labels"], mirror=mirror, host=True, out=io.StringIO())
        f["want", mirror] = video_fixture.read(path)
    return f


def _floats(path):
    from convnet_amd import hdf5io
    from convnet_amd.compute_mean import DATASETS
    with hdf5io.File(path) as f:
        return {name: f.ReadHDF5CPU(int(np.prod(f.ReadHDF5Shape(name))), name) for name in DATASETS if f.Has(name)}


@pytest.mark.parametrize("mirror", [True, False], ids=["mirrored", "no_mirror"])
@pytest.mark.parametrize("chunk", [4, 256], ids=["chunks_span_videos", "one_chunk"])
def test_the_gpu_path_writes_the_bytes_of_the_host_path(gpu, files, chunk, mirror):
    from convnet_amd import video2hdf5
    out, log = os.path.join(files["dir"], f"gpu{chunk}_{int(mirror)}.h5"), io.StringIO()
    info = video2hdf5.Video2HDF5(files["list"], out, W, H, labels=files["labels"], mirror=mirror, chunk=chunk, out=log)
    assert info["path"] == "kernel" and info["frames"] == FRAMES and info["videos"] == 3 and info["dims"] == 3 * H * W
    # chunks of 4 over 12 + 5 + 3 frames: A A A B (B C): six runs of one geometry; one chunk: three
    assert (info["chunks"], info["launches"]) == ((5, 6) if chunk == 4 else (1, 3))
    data, labels = video_fixture.read(out)
    want, want_labels = files["want", mirror]
    assert data.dtype == np.uint8 and data.shape == (FRAMES, 3 * H * W)
    assert np.array_equal(data, want), np.argwhere(data != want)[:8].tolist()
    assert np.array_equal(labels, want_labels) and labels.shape == (FRAMES, 1)
    assert log.getvalue().endswith(f"\rFrame {FRAMES} / {FRAMES}\n")


def test_the_mean_file_is_what_compute_mean_makes_of_the_dataset(gpu, files):
    from convnet_amd import compute_mean, pbtxt, video2hdf5
    out, mean = os.path.join(files["dir"], "with_mean.h5"), os.path.join(files["dir"], "mean.h5")
    video2hdf5.Video2HDF5(files["list"], out, W, H, chunk=7, mean_file=mean, out=io.StringIO())
    assert np.array_equal(video_fixture.read(out)[0], files["want", True][0])
    cfg = pbtxt.parse(f'data_config {{ file_pattern: "{out}" layer_name: "input" dataset_name: "data" image_size_y: {H} image_size_x: {W} '
                      'num_colors: 3 }\nbatch_size: 3 chunk_size: 5', pbtxt.DatasetConfig)
    stats = compute_mean.ComputeMean(cfg, "input", 3)
    assert stats["info"]["dataset_size"] == FRAMES
    again = os.path.join(files["dir"], "mean_again.h5")
    compute_mean.WriteMeanFile(again, stats)
    a, b = _floats(mean), _floats(again)
    assert sorted(a) == sorted(b) and {"mean", "std", "pixel_mean", "pixel_std", "pixel_cov"} <= set(a)
    for name in a:
        assert a[name].shape == b[name].shape and np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


def test_video_small_trains_from_the_output_and_its_boundary_file(gpu, files):
    from convnet_amd import models, pbtxt, video2hdf5
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import DataHandler
    S, T, BS = 16, 10, 2
    out, bounds = os.path.join(files["dir"], "train.h5"), os.path.join(files["dir"], "train_bounds.txt")
    video2hdf5.Video2HDF5(files["list"], out, S, S, boundary=bounds, labels=files["labels"], chunk=8, out=io.StringIO())
    seq = f'is_sequence: true seq_length: {T} boundary_file: "{bounds}"'
    text = (f'data_config {{\n  file_pattern: "{out}"\n  layer_name: "input"\n  dataset_name: "data"\n  image_size: {S}\n'
            f'  gpu_image_size_y: {S}\n  gpu_image_size_x: {S}\n  num_colors: 3\n  {seq}\n}}\n'
            f'data_config {{\n  file_pattern: "{out}"\n  layer_name: "output"\n  dataset_name: "labels"\n  {seq}\n  pick_first: true\n}}\n'
            f'batch_size: {BS}\n')
    dh = DataHandler(pbtxt.parse(text, pbtxt.DatasetConfig), seed=3)
    assert dh.GetDataSetSize() == 3                                   # the 12 frames hold 3 clips of 10; the other two videos none
    net = ConvNet(models.video_small(image_size=S, frames=T), fused=False)
    net.SetBatchsize(BS)
    net.SetupDataset(dh)
    net.AllocateMemory(False)
    for _ in range(3):
        net.TrainOneBatch()
        loss = float(net.output_layers_[0].GetLoss())
        print("loss", loss)
        assert np.isfinite(loss)
    assert net.current_iter_ == 3 and np.isfinite(net.parameters_.ToNumpy()).all()
    dh.close()


def test_the_command_line_in_a_child_process(gpu, files):
    out = os.path.join(files["dir"], "cli.h5")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "convnet_amd.video2hdf5", "--input", files["list"], "--output", out, "--width", str(W),
                        "--height", str(H), "--board", "0", "--chunk", "6", "--no-mirror"], capture_output=True, text=True,
                       cwd=files["dir"], env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Using board 0" in r.stdout and "resize_frames_u8" in r.stdout and "not mirrored" in r.stdout and r.stdout.rstrip().endswith(out)
    assert np.array_equal(video_fixture.read(out)[0], files["want", False][0])
