"""CPU: the host side of convnet_amd.compute_mean that needs no device — the oracle against hand-computed values, the config copy a
statistics pass runs on, the refusals, the integer finish, the file's names and shapes, and S / U."""
import os

import numpy as np
import pytest

import moments_ref
from convnet_amd import compute_mean, hdf5io, pbtxt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# 2 cases, C = 2, 1 x 2 pixels: a row is [c0p0, c0p1, c1p0, c1p1]
TINY = np.array([[1, 2, 3, 4], [5, 6, 7, 9]], np.uint8)


def test_int_moments_by_hand():
    acc = moments_ref.int_moments(TINY, 2)
    assert acc[:4].tolist() == [6, 8, 10, 13]                       # sums
    assert acc[4:8].tolist() == [26, 40, 58, 97]                    # sums of squares
    # colour 0 values (1, 2, 5, 6), colour 1 values (3, 4, 7, 9) at the same (case, pixel)
    assert acc[8:].tolist() == [66, 1 * 3 + 2 * 4 + 5 * 7 + 6 * 9, 100, 155]
    assert np.array_equal(moments_ref.int_moments(TINY[1:], 2, acc=moments_ref.int_moments(TINY[:1], 2)), acc)


def test_float64_statistics_by_hand():
    st = moments_ref.stats_float64(TINY, 2)
    assert np.allclose(st["mean"], [3, 4, 5, 6.5], rtol=0, atol=1e-15)
    assert np.allclose(st["std"], [2, 2, 2, 2.5], rtol=0, atol=1e-15)
    assert np.allclose(st["pixel_mean"], [3.5, 5.75], rtol=0, atol=1e-15)
    # colour 0: E[x^2] = 66 / 4, var = 16.5 - 12.25; colour 1: 155 / 4 - 5.75^2; covariance 100 / 4 - 3.5 * 5.75
    v0, v1, c01 = 4.25, 38.75 - 33.0625, 25 - 20.125
    assert np.allclose(st["pixel_std"], np.sqrt([v0, v1]), rtol=1e-15)
    assert np.allclose(st["pixel_cov"], [[1, c01 / np.sqrt(v0 * v1)], [c01 / np.sqrt(v0 * v1), 1]], rtol=1e-14)


def test_integer_finish_matches_float64_and_keeps_a_constant_dim_at_zero():
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 256, (37, 3 * 6 * 6), dtype=np.uint8)
    rows[:, 5] = 200                                                # a zero-variance dim: std 0, as in the reference
    got = compute_mean.FinishMoments(moments_ref.int_moments(rows, 3).astype(np.uint64), 37, rows.shape[1], 3)
    ref = moments_ref.stats_float64(rows, 3)
    for name in compute_mean.DATASETS:
        assert got[name].dtype == np.float32 and moments_ref.within_ulps(got[name], ref[name]), name
    assert got["std"][5] == 0.0 and got["mean"][5] == 200.0


def test_integer_finish_does_not_overflow_64_bits():
    """Two billion all-255 cases: N * sum(x^2) = 255^2 * N^2 ~ 2.6e23 is far beyond 2^64.  Variance 0 exactly, no S / U."""
    N, P, C = 2_000_000_000, 4, 3
    dims = C * P
    acc = np.array([255 * N] * dims + [255 * 255 * N] * dims + [255 * 255 * N * P] * (C * C), np.uint64)
    got = compute_mean.FinishMoments(acc, N, dims, C)
    assert (got["mean"] == 255).all() and (got["std"] == 0).all() and (got["pixel_std"] == 0).all()
    assert np.isnan(got["pixel_cov"]).all() and "S" not in got and "U" not in got


def _config(tmp_path, stream="", extra=""):
    path = str(tmp_path / "data.h5")
    rows = np.random.default_rng(1).integers(0, 256, (10, 12), dtype=np.uint8)
    with hdf5io.File(path, "w") as f:
        f.WriteDataset("images", rows)
        f.WriteDataset("labels", np.arange(10, dtype=np.int32))
    text = (f'data_config {{\n  file_pattern: "{path}"\n  layer_name: "input"\n  dataset_name: "images"\n  image_size: 2\n  {stream}\n}}\n'
            f'data_config {{\n  file_pattern: "{path}"\n  layer_name: "output"\n  dataset_name: "labels"\n}}\nbatch_size: 4\n{extra}\n')
    return pbtxt.parse(text, pbtxt.DatasetConfig)


def test_a_training_config_builds_before_its_mean_file_exists(tmp_path):
    from convnet_amd.datahandler import DataHandler
    missing = str(tmp_path / "not_yet.h5")
    cfg = _config(tmp_path, f'normalize: true mean_file: "{missing}" can_flip: true can_translate: true gpu_image_size_y: 1 '
                            'gpu_image_size_x: 1 pca_noise_stddev: 0.1 pixelwise_normalize: true normalize_local: true',
                  "randomize_cpu: true randomize_gpu: true chunk_size: 4")
    copy = compute_mean.StoredRowsConfig(cfg, "input")
    assert len(copy.data_config) == 1 and copy.batch_size == 4 and copy.chunk_size == 4 and copy.pipeline_loads
    assert not copy.randomize_cpu and not copy.randomize_gpu
    dsc = copy.data_config[0]
    for field in ("normalize", "pixelwise_normalize", "normalize_local", "pca_noise_stddev", "mean_file", "can_translate", "can_flip",
                  "gpu_image_size_y", "gpu_image_size_x"):
        assert not getattr(dsc, "has_" + field)(), field
    assert dsc.image_size == 2 and dsc.dataset_name == "images"
    # the caller's config is as it was
    assert cfg.data_config[0].normalize and cfg.data_config[0].mean_file == missing and cfg.randomize_gpu and len(cfg.data_config) == 2
    dh = DataHandler(copy)                      # builds: nothing asks for the mean file, no jitter
    st = dh.streams_["input"]
    assert not st.normalize_ and not st.jitter_.Jitters() and dh.GetDataSetSize() == 10
    dh.close()


def test_refusals(tmp_path):
    cfg = _config(tmp_path, "is_sequence: true seq_length: 2")
    with pytest.raises(SystemExit, match=r"layer input.*sequence stream.*base frame stream"):
        compute_mean.StoredRowsConfig(cfg, "input")
    with pytest.raises(SystemExit, match="Layer name hidden not found"):
        compute_mean.StoredRowsConfig(cfg, "hidden")
    raw = _config(tmp_path, "data_type: IMAGE_RAW")
    from convnet_amd.datahandler import DataHandler
    with pytest.raises(SystemExit, match="IMAGE_RAW.*not supported"):       # the data handler's own refusal, untouched
        DataHandler(compute_mean.StoredRowsConfig(raw, "input"))


def test_eigen_noise_reconstructs_the_correlation_matrix():
    rows = np.random.default_rng(2).integers(0, 256, (50, 3 * 5 * 5), dtype=np.uint8)
    rows[:, 25:50] = rows[:, :25] // 2 + rows[:, 25:50] // 2        # correlated colours: well separated eigenvalues
    stats = compute_mean.FinishMoments(moments_ref.int_moments(rows, 3).astype(np.uint64), 50, 75, 3)
    S, U, cov = (stats[k].astype(np.float64) for k in ("S", "U", "pixel_cov"))
    assert np.all(np.diff(S) <= 0) and np.all(S >= 0)
    assert np.allclose(U.T @ np.diag(S ** 2) @ U, cov, rtol=0, atol=1e-6)
    assert np.allclose(U @ U.T, np.eye(3), rtol=0, atol=1e-6)
    assert abs(np.sum(S ** 2) - 3) < 1e-6                           # a correlation matrix: the trace is C
    S1, U1 = compute_mean.EigenNoise(np.ones((1, 1)))
    assert S1.tolist() == [1.0] and U1.tolist() == [[1.0]]


def test_mean_file_round_trips_names_and_shapes(tmp_path):
    rows = np.random.default_rng(3).integers(0, 256, (20, 3 * 4 * 4), dtype=np.uint8)
    stats = compute_mean.FinishMoments(moments_ref.int_moments(rows, 3).astype(np.uint64), 20, 48, 3)
    path = str(tmp_path / "mean.h5")
    compute_mean.WriteMeanFile(path, stats)
    with hdf5io.File(path) as f:
        # (rows, cols) of the matrix a dataset reads as: the reference's (1, n) datasets are (n, 1) matrices, read flat by LoadMeans
        assert {n: f.ReadHDF5Shape(n) for n in compute_mean.DATASETS} == {
            "mean": (48, 1), "std": (48, 1), "pixel_mean": (3, 1), "pixel_std": (3, 1), "pixel_cov": (3, 3), "S": (1, 3), "U": (3, 3)}
        for name in ("mean", "std"):
            assert np.array_equal(f.ReadHDF5CPU(48, name), stats[name])
        for name in ("pixel_mean", "pixel_std", "S"):
            assert np.array_equal(f.ReadHDF5CPU(3, name), stats[name])
        assert np.array_equal(f.ReadHDF5CPU(9, "pixel_cov").reshape(3, 3), stats["pixel_cov"])
        # the matrix U, column-major in memory: its ROWS are the eigenvectors, as AddPCANoise's Dot(noise, U) needs
        assert np.array_equal(f.ReadHDF5CPU(9, "U").reshape(3, 3).T, stats["U"])
    no_noise = {k: v for k, v in stats.items() if k not in ("S", "U")}
    compute_mean.WriteMeanFile(path, no_noise)
    with hdf5io.File(path) as f:
        assert not f.Has("S") and not f.Has("U") and f.Has("pixel_cov")


def test_the_reference_pixel_mean_file_still_loads():
    with hdf5io.File(os.path.join(GOLDEN, "pixel_mean.h5")) as f:
        assert f.ReadHDF5Shape("S") == (1, 3) and f.ReadHDF5Shape("U") == (3, 3) and f.ReadHDF5Shape("pixel_mean") == (1, 3)
        U = f.ReadHDF5CPU(9, "U").reshape(3, 3).T.astype(np.float64)
        assert np.allclose(U @ U.T, np.eye(3), atol=1e-5)
        assert abs(abs(U[0]).sum() / np.sqrt(3) - 1) < 0.01        # row 0, the largest S: the grey axis, about (1, 1, 1) / sqrt(3)


def test_command_line_without_arguments_prints_help(capsys):
    assert compute_mean.main([]) == 1
    assert "--layer-name" in capsys.readouterr().out
