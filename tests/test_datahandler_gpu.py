"""GPU: DataHandler over HDF5 files — both chunk forms against the CPU oracle and against each other, the loader's reuse /
multiplicity / normalisation rules, ConvNet.SetupDataset(train, val) with a pipelined Train(), and the train_convnet entry point.
Tiny net (35 x 35 input), 8-case batches, 3 x 41 x 41 byte images."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402

CASES, COLORS, S, CROP, BS = 40, 3, 41, 35, 8
DIMS = COLORS * S * S


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """One dataset file (byte images, the case id as an int label, a class label as a float), a mean / std file and a per-channel one."""
    from convnet_amd import hdf5io
    d = tmp_path_factory.mktemp("dataset")
    rng = np.random.default_rng(3)
    f = dict(h5=str(d / "data.h5"), mean=str(d / "mean.h5"), pixel=str(d / "pixel_mean.h5"), dir=str(d))
    f["images"] = rng.integers(0, 256, (CASES, DIMS), dtype=np.uint8)
    f["mean_v"] = (rng.random(DIMS) * 255).astype(np.float32)
    f["std_v"] = ((rng.random(DIMS) + 0.5) * 60).astype(np.float32)
    f["pixel_mean_v"], f["pixel_std_v"] = np.array([120.5, 113.25, 99.0], np.float32), np.array([61.0, 58.5, 64.75], np.float32)
    with hdf5io.File(f["h5"], "w") as h:
        h.WriteDataset("images", f["images"])
        h.WriteDataset("ids", np.arange(CASES, dtype=np.int32))
        h.WriteDataset("labels", (np.arange(CASES) % 10).astype(np.float32))
    with hdf5io.File(f["mean"], "w") as h:               # a (dims, 1) column-major matrix is a (1, dims) dataset
        h.WriteHDF5CPU(f["mean_v"], 1, DIMS, "mean")
        h.WriteHDF5CPU(f["std_v"], 1, DIMS, "std")
    with hdf5io.File(f["pixel"], "w") as h:
        h.WriteHDF5CPU(f["pixel_mean_v"], 1, 3, "pixel_mean")
        h.WriteHDF5CPU(f["pixel_std_v"], 1, 3, "pixel_std")
    return f


def config_text(files, stream="", labels="ids", extra=""):
    return (f'data_config {{\n  file_pattern: "{files["h5"]}"\n  layer_name: "input"\n  dataset_name: "images"\n  image_size: {S}\n'
            f'  gpu_image_size_y: {CROP}\n  gpu_image_size_x: {CROP}\n  num_colors: {COLORS}\n  {stream}\n}}\n'
            f'data_config {{\n  file_pattern: "{files["h5"]}"\n  layer_name: "output"\n  dataset_name: "{labels}"\n}}\nbatch_size: {BS}\n{extra}\n')


def handler(files, stream="", labels="ids", extra="", **kw):
    from convnet_amd import pbtxt
    from convnet_amd.datahandler import DataHandler
    return DataHandler(pbtxt.parse(config_text(files, stream, labels, extra), pbtxt.DatasetConfig), **kw)


def make_net(dh):
    from convnet_amd.convnet import ConvNet
    from test_net_gpu import small_alexnet
    net = ConvNet(small_alexnet(), fused=True)          # (seeds the device RNG from the model: every net here starts from the same state)
    net.SetBatchsize(BS)
    net.SetupDataset(dh)
    net.AllocateMemory(False)
    return net


def staged(net):
    return (net.input_layers_[0].GetState().ToNumpy().reshape(COLORS, CROP, CROP, BS).copy(),
            net.output_layers_[0].GetData().ToNumpy().reshape(-1).copy())


def normalised(files, mean, std):
    x = files["images"].astype(np.float32)
    return oracle.port.div_by_col_vec(oracle.port.add_col_mult(x, mean, -1.0), std)


def expect(x, case, wo, ho, fl):
    return oracle.port.extract_patches(np.ascontiguousarray(x[case]), np.ascontiguousarray(wo, np.float32), np.ascontiguousarray(ho, np.float32),
                                       np.ascontiguousarray(fl, np.float32), S, S, CROP, CROP)


@pytest.mark.parametrize("raw", [False, True], ids=["float", "bytes"])
def test_datahandler_stages_batches_like_the_reference_pipeline(gpu, files, raw):
    """21 cases, labels = case ids, mean / std normalised, random crop + flip, randomize_gpu: every staged image is re-derived on the
    CPU from the ORIGINAL file, the label it arrived with and the offsets the device sampled; seven batches cross several shuffles (the
    chunk of 21 holds two batches, its tail of 5 is dropped, and every restart of the chunk shuffles it)."""
    dh = handler(files, f'can_translate: true can_flip: true normalize: true mean_file: "{files["mean"]}"',
                 extra="randomize_gpu: true max_dataset_size: 21", raw_chunks=raw, seed=4)
    net = make_net(dh)
    st = dh.streams_["input"]
    assert dh.GetDataSetSize() == 21 and dh.fits_on_gpu_
    x = normalised(files, files["mean_v"], files["std_v"])
    seen = []
    for step in range(7):
        net.GetBatch(dh)                                  # (the first one decides the chunk form: "input" is an input layer)
        assert st.raw_ is raw
        got, label = staged(net)
        case = label.astype(int)
        wo, ho, fl = (m.ToNumpy().reshape(-1) for m in (st.width_offset_, st.height_offset_, st.flip_bit_))
        assert (wo >= 0).all() and (wo < S - CROP + 1).all() and (ho >= 0).all() and (ho < S - CROP + 1).all()
        assert np.array_equal(got, expect(x, case, wo, ho, fl)), step
        seen.append(case.tolist())
    for a, b in ((0, 1), (2, 3), (4, 5)):                 # a pass over the chunk never repeats a case
        assert len(set(seen[a] + seen[b])) == 2 * BS
    assert all(0 <= c < 21 for s in seen for c in s)
    assert sorted(seen[0] + seen[1]) != seen[0] + seen[1] and seen[0] + seen[1] != seen[2] + seen[3]     # shuffled, and again
    assert st.reader_.num_reads_ == 1                     # the chunk is the dataset: read once
    dh.close()


def _run_form(files, raw, extra):
    dh = handler(files, f'can_translate: true can_flip: true normalize: true mean_file: "{files["mean"]}"', labels="labels", extra=extra,
                 raw_chunks=raw, seed=9)
    net = make_net(dh)
    batches = []
    for _ in range(12):
        net.GetBatch(dh)
        batches.append(staged(net))
    assert dh.streams_["input"].raw_ is raw and not dh.streams_["output"].raw_
    for _ in range(3):
        net.TrainOneBatch()
    flat = net.parameters_.ToNumpy().reshape(-1)
    params = np.concatenate([flat[off:off + n] for off, n in net.edge_slices_.values()])    # (the padding between slices is never written)
    dh.close()
    return batches, params


@pytest.mark.parametrize("pipeline", [False, True], ids=["serial", "pipelined"])
def test_bytes_form_equals_float_form(gpu, files, pipeline):
    """Same file, same seeds, chunk_size 16 of 40 (chunk switches, dropped tails, the wrap at the end of the file), randomize_cpu in runs of
    4 and randomize_gpu: input state and labels bit-identical for 12 batches, parameters bit-identical after 3 training steps."""
    before = threading.active_count()
    extra = "chunk_size: 16 randomize_cpu: true random_access_chunk_size: 4 randomize_gpu: true" + (" pipeline_loads: true" if pipeline else "")
    (fb, fp), (bb, bp) = _run_form(files, False, extra), _run_form(files, True, extra)
    for k, ((fx, fl), (bx, bl)) in enumerate(zip(fb, bb)):
        assert np.array_equal(fl, bl), k
        assert np.array_equal(fx.view(np.uint32), bx.view(np.uint32)), k
    assert np.array_equal(fp.view(np.uint32), bp.view(np.uint32)) and np.isfinite(fp).all()
    assert len({tuple(l.tolist()) for _, l in fb}) > 6    # (the batches do differ from one another)
    assert threading.active_count() == before


def test_max_reuse_count_reads_the_file_once_per_three_passes(gpu, files):
    dh = handler(files, extra="chunk_size: 16 max_dataset_size: 32 max_reuse_count: 2")
    net = make_net(dh)
    reader = dh.streams_["input"].reader_
    labels = []
    for step in range(13):
        net.GetBatch(dh)
        labels.append(staged(net)[1].astype(int).tolist())
        assert reader.num_reads_ == 1 + step // 6, step   # a chunk is two batches: three passes of it per read
    first, second = list(range(0, 8)), list(range(8, 16))
    assert labels[:6] == [first, second] * 3 and labels[6:12] == [list(range(16, 24)), list(range(24, 32))] * 3 and labels[12] == first
    dh.close()


def test_multiplicity_walks_the_centre_corner_flip_table(gpu, files):
    """multiplicity: 10 without can_translate / can_flip: ten views of the same 8 cases — centre, (0, 0), (max, 0), (max, max), (0, max),
    unflipped and then flipped — before the next 8 cases."""
    dh = handler(files, extra="multiplicity: 10")
    net = make_net(dh)
    x, mx = files["images"].astype(np.float32), S - CROP
    table = [(mx // 2, mx // 2), (0, 0), (mx, 0), (mx, mx), (0, mx)]      # (width offset, height offset)
    for view in range(10):
        net.GetBatch(dh)
        got, label = staged(net)
        assert label.tolist() == list(range(8)), view
        w, h = table[view % 5]
        assert np.array_equal(got, expect(x, label.astype(int), np.full(BS, w), np.full(BS, h), np.full(BS, view // 5))), view
    net.GetBatch(dh)
    got, label = staged(net)
    assert label.tolist() == list(range(8, 16)) and dh.streams_["input"].raw_
    assert np.array_equal(got, expect(x, label.astype(int), np.full(BS, mx // 2), np.full(BS, mx // 2), np.zeros(BS)))
    dh.close()


@pytest.mark.parametrize("raw", [False, True], ids=["float", "bytes"])
def test_pixelwise_normalize_broadcasts_the_channel_values_over_the_pixels(gpu, files, raw):
    dh = handler(files, f'pixelwise_normalize: true mean_file: "{files["pixel"]}"', raw_chunks=raw)
    net = make_net(dh)
    net.GetBatch(dh)
    got, label = staged(net)
    x = normalised(files, np.repeat(files["pixel_mean_v"], S * S), np.repeat(files["pixel_std_v"], S * S))
    c = (S - CROP) // 2
    assert np.array_equal(got, expect(x, label.astype(int), np.full(BS, c), np.full(BS, c), np.zeros(BS)))
    dh.close()


def test_normalize_local_falls_back_to_the_float_form(gpu, files):
    """normalize_local centres every colour plane of every case before mean / std: a pass over the whole chunk, so the stream keeps the
    float form.  Equal to the oracle port bit for bit: a plane's sum of 1 681 byte values stays below 2^24, so it is exact in fp32 in
    any order, and the mean is one division of it."""
    dh = handler(files, f'normalize_local: true normalize: true mean_file: "{files["mean"]}"')
    net = make_net(dh)
    net.GetBatch(dh)
    assert not dh.streams_["input"].raw_ and handler(files).streams_["input"].reader_.GetStoredType() == np.uint8
    got, label = staged(net)
    x = oracle.port.normalize_columns(files["images"].astype(np.float32).reshape(CASES * COLORS, S * S)).reshape(CASES, DIMS)
    x = oracle.port.div_by_col_vec(oracle.port.add_col_mult(np.ascontiguousarray(x), files["mean_v"], -1.0), files["std_v"])
    c = (S - CROP) // 2
    assert np.array_equal(got, expect(x, label.astype(int), np.full(BS, c), np.full(BS, c), np.zeros(BS)))
    dh.close()


def _write_run(files, tmp_path, max_iter=4):
    from convnet_amd import pbtxt
    from test_net_gpu import small_alexnet
    m = pbtxt.parse(small_alexnet())
    m.max_iter, m.print_after, m.validate_after, m.save_after, m.checkpoint_dir = max_iter, 2, 2, 2, str(tmp_path / "ckpt")
    paths = [str(tmp_path / n) for n in ("net.pbtxt", "train_data.pbtxt", "val_data.pbtxt")]
    pbtxt.write(paths[0], m)
    stream = f'can_translate: true can_flip: true normalize: true mean_file: "{files["mean"]}"'
    with open(paths[1], "w") as f:
        f.write(config_text(files, stream, "labels", "chunk_size: 16 randomize_cpu: true random_access_chunk_size: 4 randomize_gpu: true pipeline_loads: true"))
    with open(paths[2], "w") as f:
        f.write(config_text(files, f'normalize: true mean_file: "{files["mean"]}"', "labels", "max_dataset_size: 24"))
    return paths


def _logs(ckpt):
    names = sorted(os.listdir(ckpt))
    train = [n for n in names if n.endswith("_train.log")]
    valid = [n for n in names if n.endswith("_valid.log")]
    assert len(train) == 1 and len(valid) == 1 and any(n.endswith(".h5") for n in names), names
    read = lambda n: [l.split() for l in open(os.path.join(ckpt, n)).read().splitlines()]      # noqa: E731
    return read(train[0]), read(valid[0])


def test_setup_dataset_from_pbtxt_files_and_train(gpu, files, tmp_path):
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import DataHandler
    before = threading.active_count()
    model, train, val = _write_run(files, tmp_path)
    net = ConvNet(model, fused=True)
    with pytest.raises(SystemExit, match="Error: No training set provided."):
        net.SetupDataset("", val)
    net = ConvNet(model, fused=True)
    net.SetupDataset(train, val)
    assert net.batch_size_ == BS and isinstance(net.train_dataset_, DataHandler) and isinstance(net.val_dataset_, DataHandler)
    assert net.train_dataset_config_.chunk_size == 16 and net.valid_dataset_config_.max_dataset_size == 24
    assert net.train_dataset_.streams_["input"].raw_ and net.train_dataset_.GetDataSetSize() == 40 and net.val_dataset_.GetDataSetSize() == 24
    net.AllocateMemory(False)
    in_flight, sync = [], net.train_dataset_.Sync
    net.train_dataset_.Sync = lambda: (in_flight.append(net.train_dataset_.preload_thread_ is not None), sync())[1]
    history = net.Train(log=lambda s: None)               # validates and saves twice, each behind a Sync()
    assert net.current_iter_ == 4 and [h[0] for h in history["train"]] == [2, 4] and [h[0] for h in history["val"]] == [2, 4]
    assert np.isfinite(net.parameters_.ToNumpy()).all()
    assert len(in_flight) >= 4 and any(in_flight)         # ... and at least one of them with a preload in flight
    train_log, valid_log = _logs(str(tmp_path / "ckpt"))
    assert [l[0] for l in train_log] == ["2", "4"] and all(len(l) == 3 for l in train_log)      # iter time accuracy
    assert [l[0] for l in valid_log] == ["2", "4"] and all(len(l) == 2 for l in valid_log)      # iter accuracy
    assert float(valid_log[1][1]) == pytest.approx(history["val"][1][1], rel=1e-5)
    net.train_dataset_.close()
    net.val_dataset_.close()
    assert threading.active_count() == before
    # a stream whose cropped size is not the layer's stops before anything is allocated
    with open(train, "w") as f:
        f.write(config_text(files, "", "labels").replace(f"gpu_image_size_x: {CROP}", f"gpu_image_size_x: {CROP - 1}"))
    with pytest.raises(SystemExit, match=r"layer input.*stages 3570 values.*holds 3675"):
        ConvNet(model, fused=True).SetupDataset(train)


def test_train_convnet_entry_point_runs_in_a_fresh_process(files, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model, train, val = _write_run(files, tmp_path)
    cmd = [sys.executable, "-m", "convnet_amd.train_convnet", "--board", "0", "--model", model, "--train", train, "--val", val]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "Using board 0" in out.stdout
    train_log, valid_log = _logs(str(tmp_path / "ckpt"))
    assert [l[0] for l in train_log] == ["2", "4"] and all(len(l) == 3 and 0.0 <= float(l[2]) <= 1.0 for l in train_log)
    assert [l[0] for l in valid_log] == ["2", "4"]
    out = subprocess.run(cmd[:4] + ["01"] + cmd[5:], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode != 0 and "model-parallel" in out.stderr
