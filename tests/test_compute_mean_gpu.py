"""GPU: convnet_amd.compute_mean end to end on HDF5 files written at run time — 37 rows of 3 x 6 x 6, chunk_size 16, batch 8: three
chunks, a short last one, a tail below a batch.  The byte path (chunk_moments_u8, integer finish) within 1 float32 ulp of the float64
restatement (tests/moments_ref.py), also where the float sequence loses everything; the float sequence within a measured tolerance;
the file it writes feeds DataHandler; the command line writes the same bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import moments_ref  # noqa: E402

ROWS, C, H, W, CHUNK, BS = 37, 3, 6, 6, 16, 8
DIMS = C * H * W
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The float sequence against float64, each dataset on its own scale (moments_ref.scale_relative_error).  Obtained on the CPU with the
# float32 numpy restatement of the sequence (moments_ref.stats_float32_sequence) on this file's "plain" fixture, per dataset:
#   mean 7.7e-8, pixel_mean 8.9e-8, std 5.2e-7, pixel_std 8.8e-8, pixel_cov 3.6e-7, S 2.5e-7, U 5.12e-6
# (U is the worst: the correlation matrix of random bytes is nearly the identity, its eigenvalues 1.029 / 1.000 / 0.970 lie 0.03
# apart, and an eigenvector moves by the matrix's error over that gap.)  The bound is the worst of them x 4; the factor covers the
# GEMM's and SumRows' summation order, which is not numpy's.
MEASURED_WORST = 5.12e-6
FLOAT_TOL = 4 * MEASURED_WORST


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(5)
    return Matrix


def _rows(kind):
    rng = np.random.default_rng(21)
    if kind == "adversarial":
        return rng.integers(254, 256, (ROWS, DIMS), dtype=np.uint8)           # bright, low variance: every value 254 or 255
    return rng.integers(0, 256, (ROWS, DIMS), dtype=np.uint8)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from convnet_amd import hdf5io
    d = tmp_path_factory.mktemp("compute_mean")
    f = {"dir": str(d), "h5": str(d / "data.h5")}
    f["plain"], f["adversarial"] = _rows("plain"), _rows("adversarial")
    with hdf5io.File(f["h5"], "w") as h:
        h.WriteDataset("plain", f["plain"])
        h.WriteDataset("adversarial", f["adversarial"])
        h.WriteDataset("plain_float", f["plain"].astype(np.float32))
        h.WriteDataset("labels", np.arange(ROWS, dtype=np.int32))
    f["ref"] = {k: moments_ref.stats_float64(f[k], C) for k in ("plain", "adversarial")}      # computed once, shared, never changed
    return f


def config_text(files, dataset="plain", stream=""):
    return (f'data_config {{\n  file_pattern: "{files["h5"]}"\n  layer_name: "input"\n  dataset_name: "{dataset}"\n  image_size: {H}\n'
            f'  num_colors: {C}\n  {stream}\n}}\n'
            f'data_config {{\n  file_pattern: "{files["h5"]}"\n  layer_name: "output"\n  dataset_name: "labels"\n}}\n'
            f'batch_size: {BS}\nchunk_size: {CHUNK}\n')


def config(files, dataset="plain", stream=""):
    from convnet_amd import pbtxt
    return pbtxt.parse(config_text(files, dataset, stream), pbtxt.DatasetConfig)


def check_ulps(stats, ref):
    from convnet_amd.compute_mean import DATASETS
    for name in DATASETS:
        assert stats[name].dtype == np.float32 and stats[name].shape == np.shape(ref[name]), name
        assert moments_ref.within_ulps(stats[name], ref[name], 1), (name, stats[name], ref[name])


def test_byte_path_is_within_one_ulp_of_float64_over_all_rows(gpu, files):
    from convnet_amd.compute_mean import ComputeMean
    # a training config as it stands: normalisation and jitter asked for, the mean file not there yet
    stats = ComputeMean(config(files, stream=f'normalize: true mean_file: "{files["dir"]}/not_yet.h5" can_flip: true'), "input", C)
    assert stats["info"] == {"path": "kernel", "dataset_size": ROWS, "dims": DIMS, "image_size": (H, W), "chunks": 3}
    check_ulps(stats, files["ref"]["plain"])
    # all 37 rows: the statistics of the 32 rows whole batches cover (the reference's) are further away than an ulp
    assert not moments_ref.within_ulps(stats["mean"], moments_ref.stats_float64(files["plain"][:32], C)["mean"], 1)


def test_byte_path_holds_where_float32_moments_cancel(gpu, files):
    from convnet_amd.compute_mean import ComputeMean
    ref = files["ref"]["adversarial"]
    assert ref["std"].min() > 0.3                        # no zero-variance dim
    # the float32 sequence, E[x^2] - mean^2 at x^2 ~ 64 770 (ulp 0.0078) for a variance of 0.25, is wrong far beyond the bound
    f32 = moments_ref.stats_float32_sequence(files["adversarial"], C, BS)
    assert not moments_ref.within_ulps(f32["std"], ref["std"], 1) and not moments_ref.within_ulps(f32["pixel_cov"], ref["pixel_cov"], 1)
    assert moments_ref.scale_relative_error(f32["std"], ref["std"]) > 1e-3
    stats = ComputeMean(config(files, "adversarial"), "input", C)
    assert stats["info"]["path"] == "kernel"
    check_ulps(stats, ref)


def test_float_sequence_tolerance_is_the_measured_one(files):
    """No device: the constant beside FLOAT_TOL is what the float32 restatement gives on this fixture."""
    from convnet_amd.compute_mean import DATASETS
    f32, ref = moments_ref.stats_float32_sequence(files["plain"], C, BS), files["ref"]["plain"]
    worst = {name: moments_ref.scale_relative_error(f32[name], ref[name]) for name in DATASETS}
    print("float32 restatement, scale-relative error per dataset:", worst)
    # (numpy's own summation order may differ between builds: the constant is of this size, not this value to the last digit)
    assert MEASURED_WORST / 4 <= max(worst.values()) <= FLOAT_TOL


@pytest.mark.parametrize("dataset,raw", [("plain", False), ("plain_float", True)], ids=["forced", "float-stored"])
def test_float_sequence_agrees_with_float64(gpu, files, dataset, raw):
    """raw_chunks=False on the byte file, and a float-stored copy of it, which takes the float path without being asked."""
    from convnet_amd.compute_mean import DATASETS, ComputeMean
    stats = ComputeMean(config(files, dataset), "input", C, raw_chunks=raw)
    assert stats["info"]["path"] == "float" and stats["info"]["chunks"] == 3
    for name in DATASETS:
        err = moments_ref.scale_relative_error(stats[name], files["ref"]["plain"][name])
        print(name, err)
        assert err <= FLOAT_TOL, (name, err)


def test_five_colours_take_the_float_path(gpu, files):
    """36 x 3 values read as 4 colours of 27 pixels take the kernel; as 6 colours of 18 pixels, the matrix path.  The tolerance of the
    6-colour statistics is obtained as FLOAT_TOL is: 4 x the float32 restatement's own worst error on the same reading of the rows."""
    from convnet_amd.compute_mean import ComputeMean
    four, six = ComputeMean(config(files), "input", 4), ComputeMean(config(files), "input", 6)
    assert four["info"]["path"] == "kernel" and six["info"]["path"] == "float"
    check_ulps(four, moments_ref.stats_float64(files["plain"], 4))
    ref, f32 = moments_ref.stats_float64(files["plain"], 6), moments_ref.stats_float32_sequence(files["plain"], 6, BS)
    assert six["pixel_cov"].shape == (6, 6)
    names = ("mean", "std", "pixel_mean", "pixel_std", "pixel_cov")
    tol = 4 * max(moments_ref.scale_relative_error(f32[name], ref[name]) for name in names)
    for name in names:
        assert moments_ref.scale_relative_error(six[name], ref[name]) <= tol, (name, tol)


class _InputLayer:
    """What DataHandler.GetBatch asks of a layer."""

    def __init__(self, Matrix, cases):
        self.state_ = Matrix()
        self.state_.AllocateGPUMemory(cases, DIMS)

    def GetName(self):
        return "input"

    def IsInput(self):
        return True

    def GetState(self):
        return self.state_


def test_the_file_feeds_the_data_handler(gpu, files):
    from convnet_amd.compute_mean import ComputeMean, WriteMeanFile
    from convnet_amd.datahandler import DataHandler
    mean_file = os.path.join(files["dir"], "mean_e2e.h5")
    WriteMeanFile(mean_file, ComputeMean(config(files), "input", C))
    # colour noise from S and U
    layer = _InputLayer(gpu, BS)
    dh = DataHandler(config(files, stream=f'pixelwise_normalize: true pca_noise_stddev: 0.1 mean_file: "{mean_file}"'))
    dh.GetBatch([layer])
    noisy = layer.GetState().ToNumpy()
    assert np.isfinite(noisy).all() and np.abs(noisy).max() < 4.0       # (x - m) / s of a byte is within 1.8; the noise adds about 0.1
    st = dh.streams_["input"]
    assert (st.eig_values_.GetRows(), st.eig_values_.GetCols()) == (1, C) and (st.eig_vectors_.GetRows(), st.eig_vectors_.GetCols()) == (C, C)
    dh.close()
    # normalize: true, no noise, the whole dataset as one batch out of one chunk
    cfg = config(files, stream=f'normalize: true mean_file: "{mean_file}"')
    cfg.batch_size, cfg.chunk_size = ROWS, 0
    layer = _InputLayer(gpu, ROWS)
    dh = DataHandler(cfg)
    dh.GetBatch([layer])
    dh.close()
    x = layer.GetState().ToNumpy().T.astype(np.float64)                 # (cases, dims): float32 of exactly normalised bytes
    assert x.shape == (ROWS, DIMS)
    assert files["ref"]["plain"]["std"].min() > 0                        # the fixture's random bytes leave no zero-variance dim
    assert np.abs(x.mean(0)).max() < 1e-5
    assert np.abs(x.std(0) - 1).max() < 1e-4


def test_command_line_writes_the_same_bytes(gpu, files):
    """A fresh child process.  The datasets are compared byte for byte (an HDF5 file also holds the time it was written at)."""
    from convnet_amd import hdf5io
    from convnet_amd.compute_mean import DATASETS, ComputeMean, WriteMeanFile
    d = files["dir"]
    data, layer, a, b = (os.path.join(d, n) for n in ("train_data.pbtxt", "layer.pbtxt", "mean_cli.h5", "mean_call.h5"))
    with open(data, "w") as f:
        f.write(config_text(files, stream='normalize: true mean_file: "' + a + '"'))
    with open(layer, "w") as f:
        f.write(f'name: "input"\nnum_channels: {C}\nis_input: true\n')
    WriteMeanFile(b, ComputeMean(data, "input", C))
    out = subprocess.run([sys.executable, "-m", "convnet_amd.compute_mean", "--board", "0", "--data", data, "--layer", layer, "--output", a],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"Data set size {ROWS}" in out.stdout and f"Image size {H}x{W}" in out.stdout and "chunk_moments_u8" in out.stdout
    with hdf5io.File(a) as fa, hdf5io.File(b) as fb:
        for name in DATASETS:
            shape = fa.ReadHDF5Shape(name)
            assert shape == fb.ReadHDF5Shape(name), name
            assert fa.ReadHDF5CPU(shape[0] * shape[1], name).tobytes() == fb.ReadHDF5CPU(shape[0] * shape[1], name).tobytes(), name


def test_a_net_trains_from_the_file_the_command_line_wrote(gpu, tmp_path):
    """The whole route: a training config that names a mean file which does not exist yet (normalize, crop + flip, both shuffles) goes to
    the command line as it stands; the net of tests/test_datahandler_gpu.py then trains and validates from the file it wrote."""
    import test_datahandler_gpu as dhg
    from convnet_amd import compute_mean, hdf5io
    from convnet_amd.convnet import ConvNet
    rng = np.random.default_rng(31)
    f = {"h5": str(tmp_path / "data.h5"), "mean": str(tmp_path / "mean.h5")}
    images = rng.integers(0, 256, (dhg.CASES, dhg.DIMS), dtype=np.uint8)
    with hdf5io.File(f["h5"], "w") as h:
        h.WriteDataset("images", images)
        h.WriteDataset("labels", (np.arange(dhg.CASES) % 10).astype(np.float32))
    model, train, val = dhg._write_run(f, tmp_path)
    assert not os.path.exists(f["mean"])
    assert compute_mean.main(["--board", "0", "--data", train, "--layer-name", "input", "--num-colors", str(dhg.COLORS), "--output", f["mean"]]) == 0
    with hdf5io.File(f["mean"]) as h:
        assert moments_ref.within_ulps(h.ReadHDF5CPU(dhg.DIMS, "mean"), images.astype(np.float64).mean(0), 1)
    net = ConvNet(model, fused=True)
    net.SetupDataset(train, val)
    net.AllocateMemory(False)
    history = net.Train(log=lambda s: None)
    assert net.current_iter_ == 4 and [h[0] for h in history["train"]] == [2, 4] and [h[0] for h in history["val"]] == [2, 4]
    assert np.isfinite(net.parameters_.ToNumpy()).all()
    net.train_dataset_.close()
    net.val_dataset_.close()
