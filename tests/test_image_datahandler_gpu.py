"""GPU: DataHandler over IMAGE_RAW streams — PPM files written at run time.  The images-once form (decoded files on the GPU, one
stage_images_u8 per batch) against the float form (resized and cropped on the host, the reference's): bit for bit, batch by batch, then
through training steps, feature extraction and the two command-line programs of the reference's imagenet example.
40 images of about 60 x 50 pixels, raw_image_size 41, image_size 38, gpu_image_size 35 (tests/test_net_gpu.py's tiny net), batches of 8."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import image_ref  # noqa: E402

FILES, RAW, S, CROP, BS = 40, 41, 38, 35, 8
DIMS = 3 * S * S
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    d = tmp_path_factory.mktemp("images")
    rng = np.random.default_rng(8)
    f = dict(list=str(d / "list.txt"), h5=str(d / "labels.h5"), mean=str(d / "mean.h5"), pixel=str(d / "pixel_mean.h5"), images=[], paths=[])
    for i in range(FILES):
        w, h = int(rng.integers(45, 71)), int(rng.integers(42, 67))
        if i == 5:
            w, h = RAW, RAW                                # one file needs no resample
        if i == 6:
            w, h = 30, 33                                  # one is enlarged
        f["images"].append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        f["paths"].append(str(d / f"im{i:02d}.ppm"))
        image_ref.write_ppm(f["paths"][-1], f["images"][-1])
    with open(f["list"], "w") as h:
        h.write("\n".join(f["paths"]) + "\n")
    with hdf5io.File(f["h5"], "w") as h:
        h.WriteDataset("ids", np.arange(FILES, dtype=np.int32))
        h.WriteDataset("labels", (np.arange(FILES) % 10).astype(np.float32))
        h.WriteDataset("ids10", np.arange(10 * FILES, dtype=np.int32))
    with hdf5io.File(f["mean"], "w") as h:
        h.WriteHDF5CPU((rng.random(DIMS) * 255).astype(np.float32), 1, DIMS, "mean")
        h.WriteHDF5CPU(((rng.random(DIMS) + 0.5) * 60).astype(np.float32), 1, DIMS, "std")
    with hdf5io.File(f["pixel"], "w") as h:
        h.WriteHDF5CPU(np.array([120.5, 113.25, 99.0], np.float32), 1, 3, "pixel_mean")
        h.WriteHDF5CPU(np.array([61.0, 58.5, 64.75], np.float32), 1, 3, "pixel_std")
    return f


def config_text(files, stream="", labels="ids", extra="", crop=True):
    gpu_size = f"gpu_image_size_y: {CROP} gpu_image_size_x: {CROP}" if crop else ""
    text = (f'data_config {{\n  file_pattern: "{files["list"]}"\n  layer_name: "input"\n  data_type: IMAGE_RAW\n  raw_image_size: {RAW}\n'
            f'  image_size: {S}\n  {gpu_size}\n  {stream}\n}}\n')
    if labels:
        text += f'data_config {{\n  file_pattern: "{files["h5"]}"\n  layer_name: "output"\n  dataset_name: "{labels}"\n}}\n'
    return text + f"batch_size: {BS}\n{extra}\n"


def handler(files, stream="", labels="ids", extra="", crop=True, **kw):
    from convnet_amd import pbtxt
    from convnet_amd.datahandler import DataHandler
    return DataHandler(pbtxt.parse(config_text(files, stream, labels, extra, crop), pbtxt.DatasetConfig), **kw)


class _Layer:
    """What GetBatch asks of a data layer."""

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


def _batches(Matrix, files, raw, count, **kw):
    """``count`` batches (input state, labels) out of one form, from the same host and device seeds."""
    Matrix.InitRandom(42)
    dh = handler(files, raw_chunks=raw, seed=9, **kw)
    dh.SetInputLayers(["input"])
    layers = [_Layer(Matrix, name, name == "input", st.StagedDims()) for name, st in dh.streams_.items()]
    out = []
    for _ in range(count):
        dh.GetBatch(layers)
        out.append(tuple(l.m_.ToNumpy().copy() for l in layers))
    st = dh.streams_["input"]
    assert st.raw_ is raw and type(st.form_).__name__ == ("_ImagesOnceForm" if raw else "_FloatForm")
    dh.close()
    return out


JITTER = "can_translate: true can_flip: true"
CASES = {
    "chunk_switches_and_the_wrap": dict(extra="chunk_size: 16"),
    "pipelined": dict(stream=JITTER, extra="chunk_size: 16 pipeline_loads: true"),
    "randomize_gpu": dict(stream=JITTER, extra="chunk_size: 16 randomize_gpu: true"),
    "randomize_cpu": dict(stream=JITTER, extra="chunk_size: 16 randomize_cpu: true random_access_chunk_size: 4 randomize_gpu: true"),
    "avg10_full_image": dict(stream="avg10_full_image: true", labels="ids10", extra="chunk_size: 24", crop=False),
    "multiplicity_10": dict(extra="chunk_size: 16 multiplicity: 10"),
    "pixelwise_normalize": dict(stream=JITTER + ' pixelwise_normalize: true mean_file: "{pixel}"', extra="chunk_size: 16"),
    "normalize": dict(stream=JITTER + ' normalize: true mean_file: "{mean}"', extra="chunk_size: 16 randomize_gpu: true"),
    "parallel_disk_access": dict(stream=JITTER + " parallel_disk_access: true", extra="chunk_size: 16"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_images_once_form_equals_the_float_form(gpu, files, case):
    before = threading.active_count()
    kw = dict(CASES[case])
    kw["stream"] = kw.get("stream", "").format(**files)
    count = 22 if case == "multiplicity_10" else 12
    floats, once = _batches(gpu, files, False, count, **kw), _batches(gpu, files, True, count, **kw)
    for k, ((fx, fl), (bx, bl)) in enumerate(zip(floats, once)):
        assert np.array_equal(fl, bl), k
        assert fx.shape == bx.shape and np.array_equal(fx.view(np.uint32), bx.view(np.uint32)), k
    assert len({tuple(l.reshape(-1).tolist()) for _, l in floats}) >= (3 if case == "multiplicity_10" else 5)      # the batches differ
    assert threading.active_count() == before
    if case == "chunk_switches_and_the_wrap":            # no jitter: the centre patch of position 0 of files 0 ..., re-derived from the file
        c = (S - CROP) // 2
        for k in (0, 5):                                 # (batch 5 is the wrap: files 40 ... -> 0 ...)
            x, labels = floats[k]
            x = x.reshape(3, CROP, CROP, BS)
            for n, f in enumerate(labels.reshape(-1).astype(int)):
                row = image_ref.row(files["images"][f], RAW, RAW, S, S, 0).reshape(3, S, S)
                assert np.array_equal(x[..., n], row[:, c:c + CROP, c:c + CROP].astype(np.float32)), (k, n)
        assert floats[5][1].reshape(-1).tolist() == list(range(8))
    if case == "avg10_full_image":                       # rows 0 ... 9 are the ten positions of file 0
        x = once[0][0].reshape(3, S, S, BS)
        for position in range(BS):
            assert np.array_equal(x[..., position], image_ref.row(files["images"][0], RAW, RAW, S, S, position).reshape(3, S, S).astype(np.float32))


def test_three_training_steps_leave_the_same_parameters(gpu, files):
    from convnet_amd.convnet import ConvNet
    from test_net_gpu import small_alexnet
    params = []
    for raw in (False, True):
        dh = handler(files, JITTER + f' normalize: true mean_file: "{files["mean"]}"', labels="labels",
                     extra="chunk_size: 16 randomize_gpu: true pipeline_loads: true", raw_chunks=raw, seed=3)
        net = ConvNet(small_alexnet(), fused=True)       # (seeds the device RNG from the model)
        net.SetBatchsize(BS)
        net.SetupDataset(dh)
        net.AllocateMemory(False)
        for _ in range(3):
            net.TrainOneBatch()
        assert dh.streams_["input"].raw_ is raw
        flat = net.parameters_.ToNumpy().reshape(-1)
        params.append(np.concatenate([flat[off:off + n] for off, n in net.edge_slices_.values()]))
        dh.close()
    assert np.isfinite(params[0]).all() and np.array_equal(params[0].view(np.uint32), params[1].view(np.uint32))


def _read(path, name):
    from convnet_amd import hdf5io
    with hdf5io.File(path) as f:
        dims, rows = f.ReadHDF5Shape(name)
        return f.ReadHDF5CPU(dims * rows, name).reshape(rows, dims)


def test_extract_features_over_a_list_of_six_images(gpu, files, tmp_path):
    from convnet_amd import pbtxt
    from convnet_amd.convnet import ConvNet
    from test_net_gpu import small_alexnet
    layers = ("f7", "output")
    extra = "max_dataset_size: 6 multiplicity: 10"         # six files, ten views each, averaged; batches of 4: a left-over batch of 2
    want_path, got_path = str(tmp_path / "float.h5"), str(tmp_path / "once.h5")
    feats = "".join(f'feature {{ layer: "{l}" average_batches: 10 }}\n' for l in layers)
    text = f'output_file: "{got_path}"\n{feats}input {{\n{config_text(files, "", None, extra)}}}\n'.replace(f"batch_size: {BS}", "batch_size: 4")
    config = pbtxt.parse(text, pbtxt.FeatureExtractorConfig)
    net = ConvNet(small_alexnet(), fused=True)
    assert net.ExtractFeatures(config) == {name: 6 for name in layers}
    # the float form, in process: the same config with another output file, on a handler that keeps float chunks
    from convnet_amd import datahandler
    config.output_file = want_path
    plain, built = datahandler.DataHandler, []

    def float_handler(cfg, **kw):
        built.append(plain(cfg, raw_chunks=False, **kw))
        return built[-1]
    datahandler.DataHandler = float_handler
    try:
        assert ConvNet(small_alexnet(), fused=True).ExtractFeatures(config) == {name: 6 for name in layers}
    finally:
        datahandler.DataHandler = plain
    assert len(built) == 1 and not built[0].streams_["input"].raw_
    for name in layers:
        want, got = _read(want_path, name), _read(got_path, name)
        assert want.shape == got.shape and want.shape[0] == 6 and np.array_equal(want.view(np.uint32), got.view(np.uint32)), name
    assert np.abs(_read(got_path, "f7")).max() > 0


def test_the_imagenet_example_commands_run_in_fresh_processes(gpu, tmp_path):
    """extract_representation --model --feature-config on a list of image files, then show_results on its output: a net with hand-set
    weights (class k sums colour plane k of the 4 x 4 crop) names the dominant colour of every file."""
    from convnet_amd import hdf5io, models, pbtxt
    from convnet_amd.convnet import ConvNet
    rng = np.random.default_rng(2)
    names, paths, want = ["red", "green", "blue"], [], []
    for i, (w, h) in enumerate([(9, 7), (6, 8), (13, 6), (6, 6), (7, 12), (10, 9)]):
        image = rng.integers(0, 100, (h, w, 3), dtype=np.uint8)
        image[:, :, i % 3] = rng.integers(150, 256, (h, w))
        paths.append(str(tmp_path / f"c{i}.ppm"))
        image_ref.write_ppm(paths[-1], image)
        sums = image_ref.row(image, 6, 6, 4, 4, 0).reshape(3, -1).astype(np.int64).sum(axis=1)
        want.append(names[int(np.argmax(sums))])
    assert want == ["red", "green", "blue"] * 2
    listing, classes, out = str(tmp_path / "list.txt"), str(tmp_path / "class_names.txt"), str(tmp_path / "output.h5")
    with open(listing, "w") as f:
        f.write("\n".join(paths) + "\n")
    with open(classes, "w") as f:
        f.write("\n".join(names) + "\n")
    text = models._header("colours") + models._layer("input", 3, size=4) + models._layer("output", 3, "SOFTMAX") + models._fc("input", "output")
    net = ConvNet(text, fused=True)
    net.SetBatchsize(3)
    net.AllocateMemory(True)
    edge = net.GetEdgeByName("input:output")
    weight = np.zeros((48, 3), np.float32)               # numpy (inputs, outputs): the column-major (outputs, inputs) matrix
    for k in range(3):
        weight[16 * k:16 * (k + 1), k] = 0.01
    edge.GetWeight().FromNumpy(weight)
    edge.GetBias().Set(0.0)
    ckpt = str(tmp_path / "colours.h5")
    with hdf5io.File(ckpt, "w") as f:                    # (as SaveParameters names them)
        edge.GetWeight().WriteHDF5(f, "input:output:weight")
        edge.GetBias().WriteHDF5(f, "input:output:bias")
    model = pbtxt.parse(text)
    model.edge[0].initialization, model.edge[0].pretrained_model = "PRETRAINED", ckpt
    model_path, config_path = str(tmp_path / "colours.pbtxt"), str(tmp_path / "feature_config.pbtxt")
    pbtxt.write(model_path, model)
    with open(config_path, "w") as f:
        f.write(f'output_file: "{out}"\nfeature {{ layer: "output" }}\ninput {{\n  data_config {{\n    file_pattern: "{listing}"\n'
                '    layer_name: "input"\n    data_type: IMAGE_RAW\n    raw_image_size: 6\n    image_size: 4\n  }\n  batch_size: 3\n}\n')
    cmd = [sys.executable, "-m", "convnet_amd.extract_representation", "--board", "0", "--model", model_path, "--feature-config", config_path]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "Wrote 6 rows of output" in run.stdout
    show = subprocess.run([sys.executable, "-m", "convnet_amd.show_results", out, "--class-names", classes, "--top", "2"],
                          capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert show.returncode == 0, show.stderr[-3000:]
    lines = show.stdout.splitlines()
    assert lines[0] == repr(os.path.splitext(out)) and len(lines) == 1 + 6 * 3
    for i in range(6):
        rule, first, second = lines[1 + 3 * i:4 + 3 * i]
        assert rule == "----------------" and first.split()[0] == want[i] and second.split()[0] != want[i]
        assert float(first.split()[1]) > 0.5 > float(second.split()[1])
