"""GPU: whole nets with UPSAMPLE and RGBTOYUV edges (models.conv_autoencoder at image size 16, models.skip_sum_small) through the python
host, unfused and fused, on both matrix paths, against the reference's unmodified host on its CPU Matrix (oracle/_ref/libref_host_cpu.so
through tests/ref_host.py) — the whole-net pattern, helpers and bounds of tests/test_slices_net_gpu.py: rel_err < 1e-4 against the
reference, < 1e-5 fused against unfused.  Batch 8.

The reference's RGBToYUVEdge sizes its destination 1 x 1 (tests/test_resample_cpu.py), so the nets compared with the reference host are
the autoencoder and skip_sum_small WITHOUT its colour edge; the colour edge's forward state is held against float64, and the whole
skip_sum_small fused against unfused.  The reference host linked to THIS library aborts on these nets (oracle/seam/seam_stubs.c keeps abort
stubs for UpSampleGemm / DownSampleGemm), so there is no drop-in run here.

Grad checks: the backward pass of UPSAMPLE is the mean where the adjoint is the sum (NOTES.md), so every edge below one fails the
reference's own checker, by a factor 4 per factor-2 edge above it.  The test asserts the premise on the smooth variants of the nets — a
passing criterion of the reference's CPU run, with its rounding allowance, below half the 1 % limit; a failing one above twice the limit
at every epsilon and, at the first, with the allowance taken off — and then demands the same verdicts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_host
import resample_ref
from golden_cases import rel_err
from test_logistic_net_gpu import PATHS, assert_slices_close, on_path, one_pass
from test_slices_net_gpu import build, cpu_host, gpu  # noqa: F401  (module fixtures)

pytestmark = pytest.mark.gpu

SEED, STEPS, TOL, BATCH = 9, 3, 1e-4, 8


def _text(which, **kw):
    from convnet_amd import models
    if which == "autoencoder":
        return models.conv_autoencoder(image_size=16, **kw)
    return models.skip_sum_small(colour=False, **kw)


NETS = ("autoencoder", "skip_sum")


@pytest.fixture(scope="module")
def reference(cpu_host, tmp_path_factory):
    """The reference host's runs, once per net and only when a test asks: initial parameters, the gradient at them, the 3-step run."""
    cache = {}

    def get(which):
        if which not in cache:
            text = _text(which)
            m, d = ref_host.write_configs(tmp_path_factory.mktemp(which), text, BATCH, 2, SEED, which)
            p0 = cpu_host.init_params(m, d)
            g0 = cpu_host.gradient(m, d, p0)
            p3, metric, loss = cpu_host.train(m, d, STEPS, p0)
            cache[which] = dict(text=text, m=m, d=d, p0=p0, g0=g0, p3=p3, metric=metric, loss=np.asarray(loss, np.float64))
        return cache[which]
    return get


def _finite_and_live(net, flat, what):
    for e, (off, n) in net.edge_slices_.items():
        assert np.all(np.isfinite(flat[off:off + n])) and np.any(flat[off:off + n]), (what, e.GetName())


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", NETS)
def test_gradient_equals_the_reference_host(gpu, reference, which, path, fused):
    ref = reference(which)
    with on_path(path):
        net = build(ref["text"], BATCH, fused, ref["p0"], seed=SEED)
        r = one_pass(net)
    _finite_and_live(net, ref["g0"], "reference gradient")
    assert_slices_close(net, r["grads"], ref["g0"], TOL, f"gradient {which} {path} fused={fused}")


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", NETS)
def test_three_training_steps_equal_the_reference_host(gpu, reference, which, path, fused):
    ref = reference(which)
    with on_path(path):
        net = build(ref["text"], BATCH, fused, ref["p0"], seed=SEED)
        on_device = net.metric_on_device_
        assert on_device == (fused and which == "skip_sum"), "a SQUARED_ERROR output reports through the reference's call"
        if on_device:
            net.ReadCorrectCount()
        metric, loss = 0.0, []
        for _ in range(STEPS):
            err = net.TrainOneBatch()
            assert (err is None) == on_device
            if err is not None:
                metric += sum(err)
            loss.append(sum(l.GetLoss() for l in net.output_layers_))
        if on_device:
            metric = net.ReadCorrectCount()
        p3 = net.parameters_.ToNumpy().reshape(-1)
    print(which, path, fused, "loss", loss, ref["loss"].tolist(), "metric", metric, ref["metric"])
    _finite_and_live(net, ref["p3"], "reference parameters")
    assert_slices_close(net, p3, ref["p3"], TOL, f"parameters after {STEPS} steps {which} {path} fused={fused}")
    assert not np.array_equal(p3, ref["p0"])
    assert np.all(ref["loss"] > 0) and rel_err(loss, ref["loss"]) < TOL, (loss, ref["loss"])
    assert rel_err([metric], [ref["metric"]]) < TOL, (metric, ref["metric"])


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", ["autoencoder", "skip_sum", "skip_sum_colour"])
def test_fused_equals_unfused(gpu, reference, which, path):
    """The destinations of the new edges take the unfused activation path inside a fused net; every state, derivative and gradient of the
    two hosts agrees within 1e-5.  skip_sum_colour: the whole model, its RGBTOYUV edge included."""
    from convnet_amd import models
    from convnet_amd.edge import RGBToYUVEdge, UpSampleEdge
    text = models.skip_sum_small() if which == "skip_sum_colour" else reference(which)["text"]
    with on_path(path):
        a = build(text, BATCH, False, seed=SEED)
        b = build(text, BATCH, True, a.parameters_.ToNumpy().reshape(-1), seed=SEED)
        ra, rb = one_pass(a), one_pass(b)
    for l in a.layers_:
        n = l.GetName()
        assert rel_err(ra["states"][n], rb["states"][n]) < 1e-5, ("state fused vs unfused", n)
        if n in ra["derivs"] and not l.IsInput():
            assert rel_err(ra["derivs"][n], rb["derivs"][n]) < 1e-5, ("deriv fused vs unfused", n)
    assert rel_err(ra["grads"], rb["grads"]) < 1e-5
    _finite_and_live(a, ra["grads"], "gradient")
    new = [e for e in b.edges_ if isinstance(e, (UpSampleEdge, RGBToYUVEdge))]
    assert len(new) == {"autoencoder": 2, "skip_sum": 1, "skip_sum_colour": 2}[which]
    assert all(b.plan_[e.GetDest()].fuse_relu is None for e in new) and any(p.fuse_relu is not None for p in b.plan_.values())


def test_the_colour_edge_forward_state_is_within_the_bound_of_float64(gpu):
    from convnet_amd import models
    net = build(models.skip_sum_small(), BATCH, True, seed=SEED)
    r = one_pass(net)
    x = r["states"]["input"].reshape(3, 16, 16, BATCH)
    exact, mag = resample_ref.rgb_to_yuv64(x)
    err = np.abs(r["states"]["yuv"].reshape(3, 16, 16, BATCH).astype(np.float64) - exact)
    print("worst error / bound", float((err / (3 * 2.0 ** -24 * mag)).max()))
    assert np.all(err <= 3 * 2.0 ** -24 * mag) and np.any(x)
    assert np.any(r["states"]["sum"] > 0) and np.all(np.isfinite(r["grads"]))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", NETS)
def test_grad_checker_verdicts_equal_the_reference_checker(gpu, cpu_host, tmp_path, which, path):
    from convnet_amd.grad_check import GradChecker
    text, eps0 = _text(which, grad_check=True, relu=False), 0.03
    if which == "autoencoder":
        # an all-linear net under a squared error: the loss is quadratic in every parameter, so a central difference is exact at any
        # step and only its rounding, ulp(loss) / (2 eps batch), matters — and the loss summed over 8 x 768 outputs is ~5000.  Steps
        # ten times the models' defaults bring the passing edge's rounding allowance under the premise's margin
        for small, big in (("0.03", "0.3"), ("0.01", "0.1"), ("0.003", "0.03"), ("0.001", "0.01")):
            text = text.replace(f"grad_check_epsilon: {small}\n", f"grad_check_epsilon: {big}\n")     # (largest first: no value is hit twice)
        eps0 = 0.3
    m, d = ref_host.write_configs(tmp_path, text, BATCH, 1, SEED, "gc")
    p0 = cpu_host.init_params(m, d)
    out = os.path.join(str(tmp_path), "gc_cpu.h5")
    flags = cpu_host.grad_check_fixed(m, d, p0, out)
    names = {"autoencoder": ["input:enc1", "pool1:enc2", "pool2:dec1", "up1:dec2", "up2:output"],
             "skip_sum": ["input:stem", "pool:coarse", "stem:sum", "pool2:output"]}[which]
    res = ref_host.read_grad_check(out, names)
    assert len(flags) == len(names)
    _, _, loss = cpu_host.train(m, d, 1, p0)
    quantum = float(np.spacing(np.float32(loss[0]))) / (2 * eps0 * BATCH)
    for name, (fw, fb) in zip(names, flags):
        for kind, passed in (("weights", fw), ("bias", fb)):
            a, n = res[name][kind]
            crit = ref_host.grad_check_criterion(a, n)
            if passed:
                u = float(np.mean(4 * quantum / np.abs(a)))
                print(name, kind, "reference verdict", passed, "criterion", crit, "rounding allowance", u)
                assert len(crit) == 1 and crit[0] + u < 0.005, ("the reference's verdict is not clear of the 1 % limit", name, kind, crit, u)
            else:
                # at the first epsilon, where the difference quotient's quantum is smallest, the criterion with 4 quanta taken off every
                # difference and 2 added to every scale; at the smaller epsilons the reference's own value (a pass there would need the
                # rounding noise to reproduce the analytic value within 1 % on every entry)
                low = float(np.mean(np.maximum(np.abs(a - n[0]) - 4 * quantum, 0) / (np.abs(a + n[0]) / 2 + 2 * quantum)))
                print(name, kind, "reference verdict", passed, "criterion", crit, "its lower bound at the first epsilon", low)
                assert len(crit) == len(n) and min(crit) > 0.02 and low > 0.02, ("the reference's verdict is not clear of the 1 % limit",
                                                                                   name, kind, crit, low)
    # the edges below an UPSAMPLE fail, the ones above it (or beside it) pass
    failing = {"autoencoder": ["input:enc1", "pool1:enc2", "pool2:dec1", "up1:dec2"], "skip_sum": ["input:stem", "pool:coarse"]}[which]
    assert [n for n, (fw, fb) in zip(names, flags) if not fw and not fb] == failing
    assert all(fw and fb for n, (fw, fb) in zip(names, flags) if n not in failing)
    with on_path(path):
        net = build(text, BATCH, False, p0, cls=GradChecker, num_batches=1, seed=SEED)
        port = net.Run(fixed_batch=True)
    assert sorted(port) == sorted(names)
    for name, (fw, fb) in zip(names, flags):
        for kind, passed in (("weights", fw), ("bias", fb)):
            p_pass, p_a, _ = port[name][kind]
            a_cpu, _ = res[name][kind]
            print(name, kind, "reference", passed, "port", p_pass)
            assert rel_err(p_a, a_cpu) < TOL, ("analytic gradient", name, kind)
            assert bool(p_pass) == passed, ("verdict", name, kind, p_pass, passed)


@pytest.mark.parametrize("which", NETS)
def test_a_net_resumes_from_its_checkpoint(gpu, reference, tmp_path, which):
    ref = reference(which)
    a = build(ref["text"], BATCH, True, ref["p0"], seed=SEED)
    a.TrainOneBatch()
    path = os.path.join(str(tmp_path), "net.h5")
    a.Save(path)
    b = build(ref["text"], BATCH, True, seed=SEED)
    b.Load(path)
    assert b.current_iter_ == 1
    pa, pb = a.parameters_.ToNumpy().reshape(-1), b.parameters_.ToNumpy().reshape(-1)
    for e, (off, n) in a.edge_slices_.items():       # (the 128-float padding between the edges' slices is never written: skip it)
        assert np.array_equal(pa[off:off + n], pb[off:off + n]), ("loaded", e.GetName())
    b.train_dataset_.Seek(BATCH)
    a.TrainOneBatch()
    b.TrainOneBatch()
    pa2, pb2 = a.parameters_.ToNumpy().reshape(-1), b.parameters_.ToNumpy().reshape(-1)
    for e, (off, n) in a.edge_slices_.items():
        assert np.array_equal(pa2[off:off + n], pb2[off:off + n]), ("next step", e.GetName())
        assert not np.array_equal(pa2[off:off + n], pa[off:off + n])


# ---- train_convnet from an HDF5 file whose target stream feeds the output layer ---------------------------------------------------------
CASES, S, CROP = 24, 18, 16


def _write_run(tmp_path):
    from convnet_amd import hdf5io, models, pbtxt
    rng = np.random.default_rng(2)
    h5, mean = str(tmp_path / "data.h5"), str(tmp_path / "pixel_mean.h5")
    with hdf5io.File(h5, "w") as h:
        h.WriteDataset("images", rng.integers(0, 256, (CASES, 3 * S * S), dtype=np.uint8))
        h.WriteDataset("targets", rng.standard_normal((CASES, 3 * CROP * CROP)).astype(np.float32))
    with hdf5io.File(mean, "w") as h:               # bytes to zero mean, unit variance: the net's learning rate is set for such inputs
        h.WriteHDF5CPU(np.full(3, 127.5, np.float32), 1, 3, "pixel_mean")
        h.WriteHDF5CPU(np.full(3, 73.9, np.float32), 1, 3, "pixel_std")
    m = pbtxt.parse(models.conv_autoencoder(image_size=CROP))
    m.max_iter, m.print_after, m.validate_after, m.save_after, m.checkpoint_dir = 4, 2, 2, 2, str(tmp_path / "ckpt")
    paths = [str(tmp_path / n) for n in ("net.pbtxt", "train_data.pbtxt", "val_data.pbtxt")]
    pbtxt.write(paths[0], m)
    for p, extra in ((paths[1], "chunk_size: 16"), (paths[2], "max_dataset_size: 16")):
        with open(p, "w") as f:
            f.write(f'data_config {{\n  file_pattern: "{h5}"\n  layer_name: "input"\n  dataset_name: "images"\n  image_size: {S}\n'
                    f'  gpu_image_size_y: {CROP}\n  gpu_image_size_x: {CROP}\n  num_colors: 3\n  pixelwise_normalize: true\n'
                    f'  mean_file: "{mean}"\n}}\n'
                    f'data_config {{\n  file_pattern: "{h5}"\n  layer_name: "output"\n  dataset_name: "targets"\n}}\nbatch_size: {BATCH}\n{extra}\n')
    return paths


def test_train_convnet_trains_the_autoencoder_from_an_hdf5_file(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model, train, val = _write_run(tmp_path)
    cmd = [sys.executable, "-m", "convnet_amd.train_convnet", "--board", "0", "--model", model, "--train", train, "--val", val]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    names = sorted(os.listdir(str(tmp_path / "ckpt")))
    train_log = [n for n in names if n.endswith("_train.log")]
    assert len(train_log) == 1 and any(n.endswith(".h5") for n in names), names
    rows = [l.split() for l in open(os.path.join(str(tmp_path / "ckpt"), train_log[0])).read().splitlines()]
    assert [r[0] for r in rows] == ["2", "4"] and all(np.isfinite(float(r[-1])) and float(r[-1]) > 0 for r in rows), rows
