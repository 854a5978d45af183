"""GPU: ConvNet.ExtractFeatures(FeatureExtractorConfig) over DataWriter and feature_rows, on the tiny net and the runtime-built byte
dataset of tests/test_datahandler_gpu.py (small_alexnet, 3 x 41 x 41 images cropped to 35 x 35, batches of 8): a hidden layer (f7, 40
dims), a convolutional one (c5) and the output.

Bounds: a value averaged over P views and G cases is compared with the float64 mean of its P * G terms within
(P + G + 2) * 2^-24 * sum|x| / (P * G) — tests/test_feature_rows_gpu.py derives it; everything else is bit for bit."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from test_datahandler_gpu import BS, _write_run, config_text, files, gpu, handler, make_net  # noqa: F401  (files, gpu: fixtures)

pytestmark = pytest.mark.gpu

LAYERS = ("f7", "c5", "output")
U = 2.0 ** -24


def feature_config(files, output, extra="", P=1, G=1, layers=LAYERS):
    from convnet_amd import pbtxt
    feats = "".join(f'feature {{ layer: "{l}" average_batches: {P} average_online: {G} }}\n' for l in layers)
    text = f'output_file: "{output}"\n{feats}input {{\n{config_text(files, "", "labels", extra)}}}\n'
    return pbtxt.parse(text, pbtxt.FeatureExtractorConfig)


def fresh_net():
    from convnet_amd.convnet import ConvNet
    from test_net_gpu import small_alexnet
    return ConvNet(small_alexnet(), fused=True)      # (seeds the device RNG from the model: every fresh net allocates the same weights)


def read_file(path, layers=LAYERS):
    from convnet_amd import hdf5io
    out = {}
    with hdf5io.File(path) as f:
        for name in layers:
            dims, rows = f.ReadHDF5Shape(name)       # a (rows, dims) dataset reads as a (dims, rows) column-major matrix
            out[name] = f.ReadHDF5CPU(dims * rows, name).reshape(rows, dims)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def test_plain_extraction_equals_the_three_argument_form(gpu, files, tmp_path):
    """21 cases in batches of 8: a left-over batch of 5."""
    before = threading.active_count()
    extra = "max_dataset_size: 21"
    dh = handler(files, labels="labels", extra=extra)
    net = make_net(dh)
    old = str(tmp_path / "old.h5")
    net.ExtractFeatures(dh, list(LAYERS), old)
    dh.close()
    want = read_file(old)
    assert want["f7"].shape == (21, 40) and want["output"].shape == (21, 10) and np.abs(want["c5"]).max() > 0
    for pipelined in (True, False):
        path = str(tmp_path / f"new_{pipelined}.h5")
        rows = fresh_net().ExtractFeatures(feature_config(files, path, extra), pipelined=pipelined)
        assert rows == {name: 21 for name in LAYERS}
        got = read_file(path)
        for name in LAYERS:
            assert got[name].shape == want[name].shape and np.array_equal(bits(got[name]), bits(want[name])), (pipelined, name)
    assert threading.active_count() == before


def test_ten_view_averaging(gpu, files, tmp_path):
    """multiplicity: 10, average_batches: 10, no translate / flip: the centre / corner / flip table, averaged per case."""
    from convnet_amd.matrix import Matrix
    extra = "max_dataset_size: 21 multiplicity: 10"
    avg, views = str(tmp_path / "avg.h5"), str(tmp_path / "views.h5")
    assert fresh_net().ExtractFeatures(feature_config(files, avg, extra, P=10)) == {name: 21 for name in LAYERS}
    assert fresh_net().ExtractFeatures(feature_config(files, views, extra)) == {name: 210 for name in LAYERS}
    got, per_view = read_file(avg), read_file(views)
    # the device's own unfused sequence: buf.Set(0); buf.Add(state) x 10; buf.Divide(10) (src/datawriter.cc:138-148)
    dh = handler(files, labels="labels", extra=extra)
    net = make_net(dh)
    layers = [net.GetLayerByName(n) for n in LAYERS]
    bufs = [Matrix() for _ in layers]
    for b, l in zip(bufs, layers):
        b.AllocateGPUMemory(l.GetState().GetRows(), l.GetState().GetCols())
    want = {name: [] for name in LAYERS}
    for numcases in (8, 8, 5):
        for b in bufs:
            b.Set(0.0)
        for _ in range(10):
            for l in net.layers_:
                l.ResetAddOrOverwrite()
            net.GetBatch(dh)
            net.Fprop(False)
            for b, l in zip(bufs, layers):
                b.Add(l.GetState())
        for b, name in zip(bufs, LAYERS):
            b.Divide(10)
            want[name].append(b.ToNumpy().T[:numcases].copy())
    dh.close()
    for name in LAYERS:
        w = np.concatenate(want[name], axis=0)
        assert got[name].shape == (21, w.shape[1]) and np.array_equal(bits(got[name]), bits(w)), name
        # the P = 1 file: per batch, view after view of its numcases cases
        v, at, mean, scale = per_view[name].astype(np.float64), 0, [], []
        for numcases in (8, 8, 5):
            block = v[at:at + 10 * numcases].reshape(10, numcases, -1)
            mean.append(block.mean(axis=0))
            scale.append(np.abs(block).sum(axis=0) / 10)
            at += 10 * numcases
        mean, scale = np.concatenate(mean), np.concatenate(scale)
        err = np.abs(got[name] - mean)
        assert np.all(err <= (10 + 1 + 2) * U * scale), (name, float((err / np.maximum(scale, 1e-300)).max() / U))
        assert np.abs(per_view[name][:8] - per_view[name][8:16]).max() > 0          # (the views do differ)


def test_online_averaging_of_three_consecutive_cases(gpu, files, tmp_path):
    """24 cases, average_online: 3: 8 rows; the groups straddle the batches of 8."""
    extra = "max_dataset_size: 24"
    grouped, plain = str(tmp_path / "g3.h5"), str(tmp_path / "g1.h5")
    assert fresh_net().ExtractFeatures(feature_config(files, grouped, extra, G=3)) == {name: 8 for name in LAYERS}
    fresh_net().ExtractFeatures(feature_config(files, plain, extra))
    got, each = read_file(grouped), read_file(plain)
    for name in LAYERS:
        x = each[name].astype(np.float64).reshape(8, 3, -1)
        err, scale = np.abs(got[name] - x.mean(axis=1)), np.abs(x).sum(axis=1) / 3
        assert got[name].shape == (8, x.shape[2])
        assert np.all(err <= (1 + 3 + 2) * U * scale), (name, float((err / np.maximum(scale, 1e-300)).max() / U))


def test_refusals_come_before_anything_is_written(gpu, files, tmp_path):
    out = str(tmp_path / "never.h5")
    for kw, msg in ((dict(layers=("f7", "f9")), r"Feature f9: the model has no layer of that name"),
                    (dict(P=4, extra="multiplicity: 10"), r"Feature f7: average_batches 4 does not divide the input's multiplicity 10"),
                    (dict(G=5, extra="max_dataset_size: 24"), r"Feature f7: 24 rows .* not a multiple of average_online 5"),
                    (dict(layers=()), r"names no feature")):
        with pytest.raises(SystemExit, match=msg):
            fresh_net().ExtractFeatures(feature_config(files, out, **kw))
        assert not os.path.exists(out)


def test_pretrained_initialization_loads_weights_and_bias(gpu, files, tmp_path):
    from convnet_amd import hdf5io, pbtxt
    from convnet_amd.convnet import ConvNet
    from convnet_amd.edge import EdgeWithWeight
    from test_net_gpu import small_alexnet
    dh = handler(files, labels="labels")
    first = make_net(dh)
    for _ in range(2):
        first.TrainOneBatch()                              # (weights and biases away from their initial values)
    dh.close()
    ckpt = str(tmp_path / "first.h5")
    with hdf5io.File(ckpt, "w") as f:                      # f7 -> output is stored under another name only
        for e in first.edges_:
            if e.GetName() != "f7:output":
                e.SaveParameters(f)
        last = first.GetEdgeByName("f7:output")
        last.GetWeight().WriteHDF5(f, "classifier:weight")
        last.GetBias().WriteHDF5(f, "classifier:bias")

    def model(rename):
        m = pbtxt.parse(small_alexnet())
        for e in m.edge:
            if e.edge_type in ("FC", "CONVOLUTIONAL"):
                e.initialization, e.pretrained_model = "PRETRAINED", ckpt
                if (e.source, e.dest) == ("f7", "output"):
                    e.pretrained_edge_name = rename
        return pbtxt.parse(pbtxt.dump(m))                  # (through the text format, as a user's file would come)

    second = ConvNet(model("classifier"), fused=True)
    second.SetBatchsize(BS)
    second.AllocateMemory(True)
    a, b = first.parameters_.ToNumpy().reshape(-1), second.parameters_.ToNumpy().reshape(-1)
    checked = 0
    for e in first.edges_:
        if isinstance(e, EdgeWithWeight):
            off, n = first.edge_slices_[e]
            off2, n2 = second.edge_slices_[second.GetEdgeByName(e.GetName())]
            assert n == n2 and np.array_equal(bits(a[off:off + n]), bits(b[off2:off2 + n2])), e.GetName()
            assert np.abs(e.GetBias().ToNumpy()).max() > 0
            checked += 1
    assert checked == 8
    wrong = ConvNet(model("no_such_edge"), fused=True)
    wrong.SetBatchsize(BS)
    with pytest.raises(SystemExit, match=r"Edge f7:output: initialization PRETRAINED: no dataset no_such_edge:weight in .*first\.h5"):
        wrong.AllocateMemory(True)
    gone = pbtxt.parse(small_alexnet())
    gone.edge[0].initialization, gone.edge[0].pretrained_model = "PRETRAINED", str(tmp_path / "missing.h5")
    with pytest.raises(SystemExit, match=r"Edge input:c1: initialization PRETRAINED: cannot open HDF5 file .*missing\.h5"):
        net = ConvNet(gone, fused=True)
        net.SetBatchsize(BS)
        net.AllocateMemory(True)


def test_extract_representation_entry_point_runs_in_a_fresh_process(gpu, files, tmp_path):
    from convnet_amd import pbtxt
    from convnet_amd.convnet import ConvNet
    model, train, val = _write_run(files, tmp_path, max_iter=2)
    net = ConvNet(model, fused=True)
    net.SetupDataset(train, val)
    net.AllocateMemory(False)
    net.Train(log=lambda s: None)                          # two steps, one checkpoint and the stamped model beside it
    net.train_dataset_.close()
    net.val_dataset_.close()
    ckpt = str(tmp_path / "ckpt")
    stamped = [os.path.join(ckpt, n) for n in os.listdir(ckpt) if n.endswith(".pbtxt")]
    assert len(stamped) == 1 and pbtxt.read(stamped[0]).timestamp
    outs = [str(tmp_path / n) for n in ("cli.h5", "inproc.h5")]
    configs = []
    for out in outs:
        configs.append(out + ".pbtxt")
        pbtxt.write(configs[-1], feature_config(files, out, "max_dataset_size: 21"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "convnet_amd.extract_representation", "--board", "0", "--model", stamped[0], "--feature-config", configs[0]]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "Using board 0" in run.stdout and "Wrote 21 rows of f7" in run.stdout
    again = ConvNet(stamped[0], fused=True)
    again.ExtractFeatures(configs[1], on_allocated=again.Load)
    cli, inproc = read_file(outs[0]), read_file(outs[1])
    trained = net.parameters_.ToNumpy().reshape(-1)
    for e, (off, n) in net.edge_slices_.items():           # the checkpoint, not a fresh initialisation, is what ran
        off2, _ = again.edge_slices_[again.GetEdgeByName(e.GetName())]
        assert np.array_equal(bits(trained[off:off + n]), bits(again.parameters_.ToNumpy().reshape(-1)[off2:off2 + n])), e.GetName()
    for name in LAYERS:
        assert cli[name].shape[0] == 21 and np.array_equal(bits(cli[name]), bits(inproc[name])), name
    bad = subprocess.run(cmd[:4] + ["01"] + cmd[5:], capture_output=True, text=True, timeout=300, cwd=root)
    assert bad.returncode != 0 and "model-parallel" in bad.stderr


@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "synchronous"])
def test_a_failing_write_surfaces_on_the_main_thread(gpu, files, tmp_path, pipelined):
    """One stream's dataset is closed early: the writer thread's H5 call fails; the next Write (or close) raises it here, the thread is
    joined and the file closed."""
    from convnet_amd.datawriter import DataWriter
    before = threading.active_count()
    extra = "max_dataset_size: 24"
    dh = handler(files, labels="labels", extra=extra)
    net = make_net(dh)
    layers = [net.GetLayerByName(n) for n in LAYERS]
    w = DataWriter(feature_config(files, str(tmp_path / "broken.h5"), extra), net.layers_, 24, 1, BS, pipelined=pipelined)
    assert threading.active_count() == before + (1 if pipelined else 0)
    w.streams_["c5"].dataset_.close()
    with pytest.raises(OSError, match=r"dataset c5 of .*broken\.h5 is closed"):
        for _ in range(3):
            for l in net.layers_:
                l.ResetAddOrOverwrite()
            net.GetBatch(dh)
            net.Fprop(False)
            w.Write(layers, BS)
        w.close()
    w.close()                                              # (nothing left to raise, nothing left running)
    assert threading.active_count() == before and w.file_.id < 0
    dh.close()
