"""GPU: DataHandler over IMAGE_RAW streams with jitter_raw_image — the images-once form (decoded files on the GPU, one
stage_images_jitter_u8 per batch) against the float form (Transform on the host, the reference's path): bit for bit, batch by batch over
chunk switches, then through training steps and the train_convnet entry point.  The files, the config and the batch loop are
tests/test_image_datahandler_gpu.py's: 40 PPM files of about 60 x 50 pixels, raw_image_size 41, image_size 38, gpu_image_size 35."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_image_datahandler_gpu import BS, CROP, RAW, S, ROOT, _batches, config_text, files, gpu, handler  # noqa: E402,F401

RAW_JITTER = "jitter_raw_image: true random_rotate_max_angle: 15 min_scale: 1.5"
GPU_JITTER = " can_translate: true can_flip: true"
CASES = {
    "chunk_switches_and_the_wrap": dict(stream=RAW_JITTER, extra="chunk_size: 16"),
    "translation_alone": dict(stream="jitter_raw_image: true min_scale: 1" + GPU_JITTER, extra="chunk_size: 16 pipeline_loads: true"),
    "randomize_gpu": dict(stream=RAW_JITTER + GPU_JITTER, extra="chunk_size: 16 randomize_gpu: true"),
    "randomize_cpu": dict(stream=RAW_JITTER + GPU_JITTER, extra="chunk_size: 16 randomize_cpu: true random_access_chunk_size: 4 randomize_gpu: true"),
    "avg10_full_image": dict(stream=RAW_JITTER + " avg10_full_image: true", labels="ids10", extra="chunk_size: 24", crop=False),
    "multiplicity_10": dict(stream=RAW_JITTER, extra="chunk_size: 16 multiplicity: 10"),
    "normalize": dict(stream=RAW_JITTER + GPU_JITTER + ' normalize: true mean_file: "{mean}"', extra="chunk_size: 16 randomize_gpu: true"),
    "parallel_disk_access": dict(stream=RAW_JITTER + GPU_JITTER + " parallel_disk_access: true", extra="chunk_size: 16 pipeline_loads: true"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_images_once_form_equals_the_float_form_under_jitter_raw_image(gpu, files, case):
    before = threading.active_count()
    kw = dict(CASES[case])
    kw["stream"] = kw["stream"].format(**files)
    count = 22 if case == "multiplicity_10" else 12         # 96 rows: six chunks of 16 (four of 24), each with a draw of its own
    floats, once = _batches(gpu, files, False, count, **kw), _batches(gpu, files, True, count, **kw)
    for k, ((fx, fl), (bx, bl)) in enumerate(zip(floats, once)):
        assert np.array_equal(fl, bl), k
        assert fx.shape == bx.shape and np.array_equal(fx.view(np.uint32), bx.view(np.uint32)), k
    assert threading.active_count() == before
    if case == "chunk_switches_and_the_wrap":            # re-derived from the files: Transform by the stream's entries, the centre patch
        from convnet_amd import image_iterators as ii
        stream, c = ii.JitterStream(), (S - CROP) // 2
        noise = [stream.Sample(16, 15, 1.5) for _ in range(3)]
        for k in (0, 5):                                 # batch 5 is the third chunk's second: files 40 ... wrap to 0 ...
            x, labels = floats[k]
            x = x.reshape(3, CROP, CROP, BS)
            for n, f in enumerate(labels.reshape(-1).astype(int)):
                angle, tx, ty, scale = (v[f % 16] for v in noise[k // 2])
                image = ii.Transform(files["images"][f], angle, tx, ty, scale, RAW, RAW)
                left, top, _ = ii.Coordinates(RAW, RAW, 0, S, S)
                row = ii.PlanarCrop(image, left, top, S, S, False).reshape(3, S, S)
                assert np.array_equal(x[..., n], row[:, c:c + CROP, c:c + CROP].astype(np.float32)), (k, n)
        assert floats[5][1].reshape(-1).tolist() == list(range(8))
        assert not np.array_equal(floats[0][0], floats[5][0])                    # files 0 ... 7 twice, under two draws
    if case == "avg10_full_image":                       # rows 0 ... 9: ten positions of file 0 under ONE jitter
        x = once[0][0].reshape(3, S, S, BS)
        assert np.array_equal(x[..., 5], x[..., 0][:, :, ::-1])                   # position 5 is position 0 mirrored


def test_three_training_steps_leave_the_same_parameters(gpu, files):
    from convnet_amd.convnet import ConvNet
    from test_net_gpu import small_alexnet
    params = []
    for raw in (False, True):
        dh = handler(files, RAW_JITTER + GPU_JITTER + f' normalize: true mean_file: "{files["mean"]}"', labels="labels",
                     extra="chunk_size: 16 randomize_gpu: true pipeline_loads: true", raw_chunks=raw, seed=3)
        net = ConvNet(small_alexnet(), fused=True)
        net.SetBatchsize(BS)
        net.SetupDataset(dh)
        net.AllocateMemory(False)
        for _ in range(3):
            net.TrainOneBatch()
        st = dh.streams_["input"]
        assert st.raw_ is raw and st.reader_.jitter_ and (not raw or st.form_.rotated_)
        flat = net.parameters_.ToNumpy().reshape(-1)
        params.append(np.concatenate([flat[off:off + n] for off, n in net.edge_slices_.values()]))
        dh.close()
    assert np.isfinite(params[0]).all() and np.array_equal(params[0].view(np.uint32), params[1].view(np.uint32))


def test_train_convnet_runs_from_a_pbtxt_that_sets_the_three_fields(files, tmp_path):
    from convnet_amd import pbtxt
    from test_net_gpu import small_alexnet
    m = pbtxt.parse(small_alexnet())
    m.max_iter, m.print_after, m.validate_after, m.save_after, m.checkpoint_dir = 4, 2, 2, 2, str(tmp_path / "ckpt")
    model, train, val = (str(tmp_path / n) for n in ("net.pbtxt", "train_data.pbtxt", "val_data.pbtxt"))
    pbtxt.write(model, m)
    norm = f' normalize: true mean_file: "{files["mean"]}"'
    with open(train, "w") as f:
        f.write(config_text(files, RAW_JITTER + GPU_JITTER + norm, "labels", "chunk_size: 16 randomize_gpu: true pipeline_loads: true"))
    with open(val, "w") as f:
        f.write(config_text(files, norm, "labels", "max_dataset_size: 24"))
    cmd = [sys.executable, "-m", "convnet_amd.train_convnet", "--board", "0", "--model", model, "--train", train, "--val", val]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    names = sorted(os.listdir(str(tmp_path / "ckpt")))
    logs = [n for n in names if n.endswith("_train.log")]
    assert len(logs) == 1 and any(n.endswith(".h5") for n in names), names
    lines = [l.split() for l in open(os.path.join(str(tmp_path / "ckpt"), logs[0])).read().splitlines()]
    assert [l[0] for l in lines] == ["2", "4"] and all(0.0 <= float(l[2]) <= 1.0 for l in lines)
