"""GPU: DataHandler over an HDF5 file of frames read as clips (is_sequence) — the frames-once byte form against the float form bit for
bit, against numpy-indexed frames on its own, and video_small trained, validated, checkpointed and run from the command line on the file.
40 byte frames 3 x 20 x 20 in sequences of 17, 2 (skipped) and 21, clips of 16 cropped to 16 x 16, batches of 4."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES, COLORS, S, CROP, T, BS = 40, 3, 20, 16, 16, 4
FS = COLORS * S * S
BOUNDS = [17, 2, 21]
CLIPS = [0, 1, 19, 20, 21, 22, 23, 24]
SETTINGS = ["", "randomize_gpu: true", "randomize_cpu: true random_access_chunk_size: 4", "pipeline_loads: true",
            "randomize_cpu: true random_access_chunk_size: 4 randomize_gpu: true pipeline_loads: true"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from convnet_amd import hdf5io
    d = tmp_path_factory.mktemp("clips")
    rng = np.random.default_rng(7)
    f = dict(h5=str(d / "frames.h5"), mean=str(d / "mean.h5"), bounds=str(d / "bounds.txt"), dir=str(d))
    f["frames"] = rng.integers(0, 256, (FRAMES, FS), dtype=np.uint8)
    f["mean_v"] = (rng.random(FS) * 255).astype(np.float32)
    f["std_v"] = ((rng.random(FS) + 0.5) * 60).astype(np.float32)
    with hdf5io.File(f["h5"], "w") as h:
        h.WriteDataset("frames", f["frames"])
        h.WriteDataset("ids", np.arange(FRAMES, dtype=np.int32))
        h.WriteDataset("labels", (np.arange(FRAMES) % 10).astype(np.float32))
    with hdf5io.File(f["mean"], "w") as h:
        h.WriteHDF5CPU(f["mean_v"], 1, FS, "mean")
        h.WriteHDF5CPU(f["std_v"], 1, FS, "std")
    with open(f["bounds"], "w") as h:
        h.write("\n".join(map(str, BOUNDS)) + "\n")
    return f


def config_text(files, stream="", labels="labels", extra="", crop=CROP):
    seq = f'is_sequence: true seq_length: {T} boundary_file: "{files["bounds"]}"'
    return (f'data_config {{\n  file_pattern: "{files["h5"]}"\n  layer_name: "input"\n  dataset_name: "frames"\n  image_size: {S}\n'
            f'  gpu_image_size_y: {crop}\n  gpu_image_size_x: {crop}\n  num_colors: {COLORS}\n  {seq}\n  {stream}\n}}\n'
            f'data_config {{\n  file_pattern: "{files["h5"]}"\n  layer_name: "output"\n  dataset_name: "{labels}"\n  {seq}\n  pick_first: true\n}}\n'
            f'batch_size: {BS}\n{extra}\n')


def jitter(files):
    return f'can_translate: true can_flip: true normalize: true mean_file: "{files["mean"]}"'


def handler(files, stream="", labels="labels", extra="", crop=CROP, **kw):
    from convnet_amd import pbtxt
    from convnet_amd.datahandler import DataHandler
    return DataHandler(pbtxt.parse(config_text(files, stream, labels, extra, crop), pbtxt.DatasetConfig), **kw)


def make_net(dh):
    from convnet_amd import models
    from convnet_amd.convnet import ConvNet
    net = ConvNet(models.video_small(image_size=CROP, frames=T), fused=True)
    net.SetBatchsize(BS)
    net.SetupDataset(dh)
    net.AllocateMemory(False)
    return net


def staged(net):
    return (net.input_layers_[0].GetState().ToNumpy().reshape(T * COLORS, CROP, CROP, BS).copy(),
            net.output_layers_[0].GetData().ToNumpy().reshape(-1).copy())


def _params(net):
    flat = net.parameters_.ToNumpy().reshape(-1)
    return np.concatenate([flat[off:off + n] for off, n in net.edge_slices_.values()])    # (the padding between slices is never written)


def _run_form(files, raw, extra):
    dh = handler(files, jitter(files), extra="chunk_size: 6 " + extra, raw_chunks=raw, seed=9)
    net = make_net(dh)
    st = dh.streams_["input"]
    batches = []
    for _ in range(8):                                    # a chunk of 6 clips holds one batch: eight chunk loads, several wraps
        net.GetBatch(dh)
        batches.append(staged(net))
    assert st.raw_ is raw and st.frames_once_ is raw and not dh.streams_["output"].raw_
    assert st.reader_.num_reads_ >= 8
    if raw:                                               # every frame of a run once: fewer than the 6 x 16 of materialised clips
        assert dh.raw_data_["input"].numel() == dh.FrameBufferSize("input") * FS < 6 * T * FS
    for _ in range(3):
        net.TrainOneBatch()
    params = _params(net)
    dh.close()
    return batches, params


@pytest.mark.parametrize("extra", SETTINGS, ids=["sequential", "randomize_gpu", "randomize_cpu", "sequential_pipelined", "all_pipelined"])
def test_frames_once_form_equals_float_form(gpu, files, extra):
    """Same file, same seeds: input state and labels bit-identical for 8 batches (each from a chunk of its own), video_small's parameters
    bit-identical after 3 training steps."""
    before = threading.active_count()
    (fb, fp), (bb, bp) = _run_form(files, False, extra), _run_form(files, True, extra)
    for k, ((fx, fl), (bx, bl)) in enumerate(zip(fb, bb)):
        assert np.array_equal(fl, bl), k
        assert np.array_equal(fx.view(np.uint32), bx.view(np.uint32)), k
    assert np.array_equal(fp.view(np.uint32), bp.view(np.uint32)) and np.isfinite(fp).all()
    assert len({tuple(l.tolist()) for _, l in fb}) > 2    # (the batches do differ from one another)
    assert threading.active_count() == before


class _Layer:
    """What GetBatch needs of a data layer."""

    def __init__(self, Matrix, name, is_input, dims):
        self.name_, self.is_input_, self.m_ = name, is_input, Matrix()
        self.m_.AllocateGPUMemory(BS, dims)

    def GetName(self):
        return self.name_

    def IsInput(self):
        return self.is_input_

    def GetState(self):
        return self.m_

    GetData = GetState


@pytest.mark.parametrize("extra", ["", "randomize_cpu: true random_access_chunk_size: 4 randomize_gpu: true"], ids=["sequential", "shuffled"])
def test_staged_clips_are_the_files_frames_in_layer_order(gpu, files, extra):
    """No jitter, no mean: every staged clip is frames[first : first + 16] in the layer's (C*T, Y, X, N) order — plane t * C + c is colour
    c of frame first + t — with the label (the id of the clip's first frame) it arrived with.  The float form is not involved."""
    dh = handler(files, labels="ids", extra="chunk_size: 6 " + extra, crop=S, seed=2)
    layers = [_Layer(gpu, "input", True, T * FS), _Layer(gpu, "output", False, 1)]
    dh.SetInputLayers(["input"])
    seen = []
    for _ in range(6):
        dh.GetBatch(layers)
        got = layers[0].m_.ToNumpy().reshape(T * COLORS, S, S, BS)
        first = layers[1].m_.ToNumpy().reshape(-1).astype(int)
        assert dh.streams_["input"].frames_once_ and all(f in CLIPS for f in first)
        for n, f in enumerate(first):
            assert np.array_equal(got[..., n], files["frames"][f:f + T].astype(np.float32).reshape(T * COLORS, S, S)), (n, f)
        seen.append(first.tolist())
    if not extra:
        assert seen[:3] == [[0, 1, 19, 20], [23, 24, 0, 1], [21, 22, 23, 24]]     # chunks of 6 clip rows, tails of 2 dropped, the wrap
    dh.close()


def _write_run(files, tmp_path, max_iter=4):
    from convnet_amd import models, pbtxt
    m = pbtxt.parse(models.video_small(image_size=CROP, frames=T))
    m.max_iter, m.print_after, m.validate_after, m.save_after, m.checkpoint_dir = max_iter, 2, 2, 2, str(tmp_path / "ckpt")
    paths = [str(tmp_path / n) for n in ("video.pbtxt", "clips.pbtxt", "clips_val.pbtxt")]
    pbtxt.write(paths[0], m)
    with open(paths[1], "w") as f:
        f.write(config_text(files, jitter(files), extra="chunk_size: 6 randomize_cpu: true random_access_chunk_size: 4 randomize_gpu: true pipeline_loads: true"))
    with open(paths[2], "w") as f:
        f.write(config_text(files, f'normalize: true mean_file: "{files["mean"]}"'))
    return paths


def test_train_validate_extract_checkpoint_and_resume_on_the_frame_file(gpu, files, tmp_path):
    from convnet_amd import hdf5io
    from convnet_amd.convnet import ConvNet
    before = threading.active_count()
    model, train, val = _write_run(files, tmp_path)
    net = ConvNet(model, fused=True)
    net.SetupDataset(train, val)
    assert net.batch_size_ == BS and net.train_dataset_.GetDataSetSize() == 8 and net.val_dataset_.GetDataSetSize() == 8
    assert net.train_dataset_.streams_["input"].frames_once_ and net.val_dataset_.streams_["input"].frames_once_
    net.AllocateMemory(False)
    history = net.Train(log=lambda s: None)
    assert net.current_iter_ == 4 and [h[0] for h in history["train"]] == [2, 4] and [h[0] for h in history["val"]] == [2, 4]
    acc = net.Validate()
    assert len(acc) == 1 and 0.0 <= acc[0] <= 1.0
    feats = str(tmp_path / "features.h5")
    net.ExtractFeatures(net.val_dataset_, ["output"], feats)
    with hdf5io.File(feats) as f:
        rows, cols = f.ReadHDF5Shape("output")
        out = f.ReadHDF5CPU(rows * cols, "output")
    assert rows * cols == 8 * 10 and np.isfinite(out).all()
    ckpt = str(tmp_path / "resume.h5")
    net.Save(ckpt)
    other = ConvNet(model, fused=True)
    other.SetupDataset(train, val)
    other.AllocateMemory(False)
    other.Load(ckpt)
    assert other.current_iter_ == 4
    for ea, eb in zip(net.edges_, other.edges_):
        if ea.GetParameterMemoryRequirement():
            assert np.array_equal(ea.GetWeight().ToNumpy(), eb.GetWeight().ToNumpy()), ea.GetName()
            assert np.array_equal(ea.GetBias().ToNumpy(), eb.GetBias().ToNumpy()), ea.GetName()
    other.Train(max_iter=6, log=lambda s: None)
    assert other.current_iter_ == 6 and np.isfinite(other.parameters_.ToNumpy()).all()
    for n in (net, other):
        n.train_dataset_.close()
        n.val_dataset_.close()
    assert threading.active_count() == before
    # a stream whose clip length is not the layer's stops before anything is allocated
    with open(train, "w") as f:
        f.write(config_text(files, jitter(files)).replace(f"seq_length: {T}", f"seq_length: {T - 1}"))
    with pytest.raises(SystemExit, match=r"layer input.*stages 11520 values.*holds 12288"):
        ConvNet(model, fused=True).SetupDataset(train)


def test_train_convnet_entry_point_trains_video_small_from_the_frame_file(files, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model, train, val = _write_run(files, tmp_path)
    cmd = [sys.executable, "-m", "convnet_amd.train_convnet", "--board", "0", "--model", model, "--train", train, "--val", val]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    names = sorted(os.listdir(str(tmp_path / "ckpt")))
    train_log = [n for n in names if n.endswith("_train.log")]
    valid_log = [n for n in names if n.endswith("_valid.log")]
    assert len(train_log) == 1 and len(valid_log) == 1 and any(n.endswith(".h5") for n in names), names
    read = lambda n: [l.split() for l in open(os.path.join(str(tmp_path / "ckpt"), n)).read().splitlines()]      # noqa: E731
    assert [l[0] for l in read(train_log[0])] == ["2", "4"] and [l[0] for l in read(valid_log[0])] == ["2", "4"]
