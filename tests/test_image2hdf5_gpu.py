"""GPU: convnet_amd.image2hdf5 end to end on PPM / PGM files written at run time — the GPU path (images-once chunks, crop_images_u8, pinned
downloads, the writer thread) against --host (numpy on the host), byte for byte; --mean-file against compute_mean on the produced file,
dataset for dataset and bit for bit; --labels; the command line in a child process."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import image_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIZE, CROP = 12, 10
# w x h of 11 files: landscape, portrait, the resize size itself, upscaled, grey, one pixel wide / high, larger ones
SIZES = [(17, 13), (12, 19), (12, 12), (7, 5), (14, 15), (1, 6), (9, 1), (40, 31), (23, 60), (12, 30), (31, 12)]
GREY = 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from convnet_amd import image2hdf5
    d = tmp_path_factory.mktemp("image2hdf5_gpu")
    rng = np.random.default_rng(77)
    paths = []
    for i, (w, h) in enumerate(SIZES):
        if i == GREY:
            paths.append(str(d / f"im{i}.pgm"))
            image_ref.write_pgm(paths[-1], rng.integers(0, 256, (h, w), dtype=np.uint8))
        else:
            paths.append(str(d / f"im{i}.ppm"))
            image_ref.write_ppm(paths[-1], rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    f = {"dir": str(d), "list": str(d / "list.txt"), "labels": str(d / "labels.txt"), "host": str(d / "host.h5")}
    with open(f["list"], "w") as out:
        out.write("\n".join(paths) + "\n")
    with open(f["labels"], "w") as out:
        out.write("\n".join(str(3 * i + 1) for i in range(len(paths))))
    image2hdf5.Image2HDF5(f["list"], f["host"], CROP, RESIZE, host=True, out=io.StringIO())       # the comparison leg, once
    f["want"] = _dataset(f["host"], "data", np.uint8)
    return f


def _dataset(path, name, dtype):
    from convnet_amd import hdf5io
    with hdf5io.File(path) as f:
        r = f.RowReader(name)
        assert r.GetStoredType() == dtype
        out = np.empty((r.GetDataSetSize(), r.GetDims()), np.uint8 if dtype == np.uint8 else np.float32)
        r.Get(out, 0, len(out))
        r.close()
    return out


def _decoded(files, i):
    from convnet_amd import image_iterators
    with open(files["list"]) as f:
        return image_iterators.ReadImage(f.read().split()[i])


def _floats(path):
    from convnet_amd import hdf5io
    from convnet_amd.compute_mean import DATASETS
    with hdf5io.File(path) as f:
        return {name: f.ReadHDF5CPU(int(np.prod(f.ReadHDF5Shape(name))), name) for name in DATASETS if f.Has(name)}


@pytest.mark.parametrize("chunk", [4, 64], ids=["three_chunks_the_last_wraps", "one_chunk_larger_than_the_list"])
def test_the_gpu_path_writes_the_bytes_of_the_host_path(gpu, files, chunk):
    from convnet_amd import image2hdf5
    out, log = os.path.join(files["dir"], f"gpu{chunk}.h5"), io.StringIO()
    info = image2hdf5.Image2HDF5(files["list"], out, CROP, RESIZE, chunk=chunk, out=log)
    n = len(SIZES)
    assert info["path"] == "kernel" and info["files"] == n and info["chunks"] == (3 if chunk == 4 else 1)
    got = _dataset(out, "data", np.uint8)
    assert got.shape == (n, 3 * CROP * CROP)
    assert np.array_equal(got, files["want"]), np.argwhere(got != files["want"])[:8].tolist()
    assert log.getvalue().endswith(f"\rImage {n} / {n}\n")
    assert np.array_equal(got[0], image_ref.row(_decoded(files, 0), RESIZE, RESIZE, CROP, CROP, 0))       # (and of the scalar loops)


def test_the_mean_file_is_what_compute_mean_makes_of_the_dataset(gpu, files):
    from convnet_amd import compute_mean, image2hdf5, pbtxt
    out, mean = os.path.join(files["dir"], "with_mean.h5"), os.path.join(files["dir"], "mean.h5")
    image2hdf5.Image2HDF5(files["list"], out, CROP, RESIZE, chunk=4, labels=files["labels"], mean_file=mean, out=io.StringIO())
    assert np.array_equal(_dataset(out, "data", np.uint8), files["want"])
    # --labels
    labels = _dataset(out, "labels", np.int32)
    assert labels.shape == (len(SIZES), 1) and labels.reshape(-1).tolist() == [3 * i + 1 for i in range(len(SIZES))]
    cfg = pbtxt.parse(f'data_config {{ file_pattern: "{out}" layer_name: "input" dataset_name: "data" image_size: {CROP} num_colors: 3 }}\n'
                      'batch_size: 3 chunk_size: 5', pbtxt.DatasetConfig)
    stats = compute_mean.ComputeMean(cfg, "input", 3)
    assert stats["info"]["path"] == "kernel" and stats["info"]["dataset_size"] == len(SIZES)
    again = os.path.join(files["dir"], "mean_again.h5")
    compute_mean.WriteMeanFile(again, stats)
    a, b = _floats(mean), _floats(again)
    assert sorted(a) == sorted(b) and {"mean", "std", "pixel_mean", "pixel_std", "pixel_cov"} <= set(a)
    for name in a:
        assert a[name].shape == b[name].shape and np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


def test_the_command_line_in_a_child_process(gpu, files):
    out = os.path.join(files["dir"], "cli.h5")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "convnet_amd.image2hdf5", "--input", files["list"], "--output", out, "--crop", str(CROP),
                        "--resize", str(RESIZE), "--board", "0", "--chunk", "5"], capture_output=True, text=True, cwd=files["dir"], env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Using board 0" in r.stdout and "crop_images_u8" in r.stdout and r.stdout.rstrip().endswith(out)
    assert np.array_equal(_dataset(out, "data", np.uint8), files["want"])
