"""GPU: whole nets with layer slices (tests/slice_nets.py: grouped convolutions and channel concatenation) through the python host,
unfused and fused, on both matrix paths, against the reference's unmodified host on its CPU Matrix (oracle/_ref/libref_host_cpu.so
through tests/ref_host.py) — the whole-net pattern of tests/test_logistic_net_gpu.py: same pbtxt, the reference's own initial parameters,
the very batches its data shim generates.

 * net A (batch 5): slice b of h2 starts 2025 floats into the layer, a view whose base is 4-byte aligned only, on the destination side of a
   conv and on the input side of nothing but the whole-layer pool; net B (h1 = a:3, b:7): h1.b starts 1215 floats in, so a misaligned view
   is also the SOURCE of a conv, the target of its input gradient and the input of its weight gradient;
 * net C (batch 64, slice widths multiples of 16): one group's forward, input-gradient and weight-gradient GEMMs run on the wide kernels
   (asserted from the library's kernel timers);
 * every net with ReLU + MAXPOOL and with LINEAR + AVERAGE_POOL;
 * models.inception_small: 1x1, 3x3 and 5x5 branches into one layer, and with a pooled branch whose max-pool mask pair runs on a view.

Bounds: golden_cases.rel_err < 1e-4 against the reference, < 1e-5 fused against unfused — the project's existing ones.
The grad-check test follows tests/test_logistic_net_gpu.py (its docstring has the reasoning on the verdicts): the premise — every criterion
of the reference's own CPU run below half the 1 % limit — is asserted first, then equal verdicts are demanded."""
import ctypes
import os

import numpy as np
import pytest

import ref_host
import slice_nets as nets
from golden_cases import rel_err
from test_logistic_net_gpu import PATHS, HashData, assert_slices_close, on_path, one_pass

pytestmark = pytest.mark.gpu

SEED, STEPS, TOL = 9, 3, 1e-4
TIE = 64 * 2.0 ** -23     # 64 ulp: two fp32 sums of the 1152 products of a net C unit in different orders differ by a few ulp
KINDS = {"relu_maxpool": nets.RELU, "linear_avgpool": nets.LINEAR}
# (generator, batch, data seed).  Net C's data seed is one whose compared passes hold the premise of pool_tie_margin below
NETS = {"A": (nets.net_a, 5, SEED), "B": (nets.net_b, 5, SEED), "C": (nets.wide_net, nets.WIDE["batch"], 10),
        "inception": (nets.inception, 8, SEED), "inception_pooled": (lambda kinds: nets.inception(kinds, pooled_branch=True), 8, SEED)}


def pool_tie_margin(net, which, kinds):
    """The premise of a comparison of net C with max pooling, asserted before it (tests/slice_nets.py, WIDE): no window that carries a
    derivative has its two largest inputs within TIE of each other — there the gradient is discontinuous and two correct fp32
    implementations may differ by a whole filter row of a weight gradient.  Returns the smallest relative gap between the two largest
    inputs over those windows (None where the premise does not apply: smooth nets, and nets A / B with their few windows)."""
    if which != "C" or kinds != "relu_maxpool":
        return None
    n = nets.WIDE["size"] ** 2
    h2 = net.GetLayerByName("h2").GetState().ToNumpy().reshape(-1, n, nets.WIDE["batch"])
    dp = net.GetLayerByName("pool").GetDeriv().ToNumpy().reshape(-1, nets.WIDE["batch"])
    top2 = np.partition(h2, n - 2, axis=1)[:, n - 2:, :]
    live = (dp != 0) & (top2[:, 1, :] > 0)
    assert live.any()
    return float(((top2[:, 1, :] - top2[:, 0, :])[live] / top2[:, 1, :][live]).min())


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


@pytest.fixture(scope="module")
def cpu_host():
    # on a GPU box a missing oracle is a failure, not a skip (as in tests/test_grad_check_strict.py)
    assert os.path.exists(ref_host.CPU_SO), "oracle/_ref/libref_host_cpu.so missing: run __graft_entry__.build() where the reference tree exists"
    return ref_host.RefHost(ref_host.CPU_SO)


def build(text, batch, fused, params=None, cls=None, num_batches=2, seed=None):
    from convnet_amd.convnet import ConvNet
    net = (cls or ConvNet)(text, fused=fused)
    net.SetBatchsize(batch)
    net.AllocateLayerMemory()                      # the data layers' shapes, which the batches follow
    net.SetupDataset(HashData(net, batch, num_batches, SEED if seed is None else seed))
    net.AllocateMemory(False)
    if params is not None:
        assert net.parameters_.GetNumEls() == params.size
        net.parameters_.FromNumpy(params.reshape(1, -1))
    return net


@pytest.fixture(scope="module")
def reference(cpu_host, tmp_path_factory):
    """The reference host's runs, once per (net, kinds) and only when a test asks: initial parameters, the gradient at them, the 3-step
    training run."""
    cache = {}

    def get(which, kinds):
        key = (which, kinds)
        if key not in cache:
            gen, batch, seed = NETS[which]
            text = gen(KINDS[kinds])
            m, d = ref_host.write_configs(tmp_path_factory.mktemp(f"{which}_{kinds}"), text, batch, 2, seed, which)
            p0 = cpu_host.init_params(m, d)
            g0 = cpu_host.gradient(m, d, p0)
            p3, metric, loss = cpu_host.train(m, d, STEPS, p0)
            assert np.any(g0) and np.all(np.isfinite(g0)) and np.all(np.isfinite(p3))
            cache[key] = dict(text=text, batch=batch, seed=seed, m=m, d=d, p0=p0, g0=g0, p3=p3, metric=metric, loss=np.asarray(loss, np.float64))
        return cache[key]
    return get


CASES = [(w, k) for w in NETS for k in KINDS]


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which,kinds", CASES)
def test_gradient_equals_the_reference_host(gpu, reference, which, kinds, path, fused):
    ref = reference(which, kinds)
    with on_path(path):
        net = build(ref["text"], ref["batch"], fused, ref["p0"], seed=ref["seed"])
        r = one_pass(net)
        margin = pool_tie_margin(net, which, kinds)
    print("pool tie margin", margin)
    assert margin is None or margin > TIE, ("the batch sits on a pooling tie: the comparison is void, choose another data seed", margin)
    assert_slices_close(net, r["grads"], ref["g0"], TOL, f"gradient {which} {kinds} {path} fused={fused}")
    if kinds == "linear_avgpool":     # a smooth net: every parameter of every edge, on every slice, takes part
        for e, (off, n) in net.edge_slices_.items():
            assert np.all(ref["g0"][off:off + n] != 0), ("an entry without gradient", e.GetName())
    if which in "AB":
        # the views the net ran on: 4-byte aligned only (module docstring)
        h1, h2 = net.GetLayerByName("h1"), net.GetLayerByName("h2")
        off = lambda l, s: (l.GetState(s).mat_.data_device - l.GetState().mat_.data_device) // 4  # noqa: E731
        assert (off(h1, "b"), off(h2, "b")) == ((1620, 2025) if which == "A" else (1215, 2025))
        assert h2.GetState("b").mat_.data_device % 16 != 0 and h2.GetDeriv("b").mat_.data_device % 16 != 0
        assert (h1.GetState("b").mat_.data_device % 16 != 0) == (which == "B")


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which,kinds", CASES)
def test_three_training_steps_equal_the_reference_host(gpu, reference, which, kinds, path, fused):
    ref = reference(which, kinds)
    with on_path(path):
        net = build(ref["text"], ref["batch"], fused, ref["p0"], seed=ref["seed"])
        if fused:
            net.ReadCorrectCount()
        metric, loss = 0.0, []
        for _ in range(STEPS):
            err = net.TrainOneBatch()
            margin = pool_tie_margin(net, which, kinds)
            print("pool tie margin", margin)
            assert margin is None or margin > TIE, ("the batch sits on a pooling tie: the comparison is void, choose another data seed", margin)
            assert (err is None) == fused, "the fused host keeps the metric on the device"
            if err is not None:
                metric += sum(err)
            loss.append(sum(l.GetLoss() for l in net.output_layers_))
        if fused:
            metric = net.ReadCorrectCount()
        p3 = net.parameters_.ToNumpy().reshape(-1)
    print(which, kinds, path, fused, "loss", loss, ref["loss"].tolist(), "metric", metric, ref["metric"])
    assert_slices_close(net, p3, ref["p3"], TOL, f"parameters after {STEPS} steps {which} {kinds} {path} fused={fused}")
    assert not np.array_equal(p3, ref["p0"])
    assert np.all(ref["loss"] > 0) and rel_err(loss, ref["loss"]) < TOL, (loss, ref["loss"])
    assert rel_err([metric], [ref["metric"]]) < TOL, (metric, ref["metric"])


def _timer_names(fn):
    """fn() with the library's kernel timers on: the rows of its report ({kernel, op, ...})."""
    from convnet_amd import _lib
    _lib.profile_report()
    _lib.profile_enable(True)
    try:
        fn()
        return _lib.profile_report()
    finally:
        _lib.profile_enable(False)


def test_one_group_of_net_c_runs_on_the_wide_kernels(gpu, cpu_host, tmp_path):
    """The launch trace's mechanism (tests/gemm_launch_trace.py: the kernel timers) around one training pass of net C on the bf16-split
    path: the wide patch kernel took a forward and an input-gradient launch, the wide weight-gradient kernel a weight-gradient launch.
    Only the group h1.b -> h2.b (128 -> 192) meets their conditions (tests/slice_nets.py WIDE)."""
    text = nets.wide_net()
    m, d = ref_host.write_configs(tmp_path, text, nets.WIDE["batch"], 2, NETS["C"][2], "C")
    p0 = cpu_host.init_params(m, d)
    with on_path("split"):
        net = build(text, nets.WIDE["batch"], True, p0, seed=NETS["C"][2])
        one_pass(net)          # (the first pass sizes the scratch arenas)
        rows = _timer_names(lambda: one_pass(net))
    seen = sorted({(r["kernel"], r["op"]) for r in rows})
    print("\n".join(f"{k}  {op}" for k, op in seen))
    ops_of = lambda prefix: {op for k, op in seen if k.startswith(prefix)}  # noqa: E731
    assert {"conv_fprop", "conv_dgrad"} <= ops_of("gpw_kernel"), seen
    assert ops_of("wgw_kernel") == {"conv_wgrad"}, seen


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", ["A", "C", "inception"])
def test_fused_equals_unfused_with_dropout_on_the_sliced_relu_layers(gpu, reference, which, path):
    from convnet_amd.layer import ReLULayer
    gen, batch, seed = NETS[which]
    text = gen(nets.RELU, dropprob=0.25) if which != "C" else nets.wide_net(dropprob=0.25)
    p0 = reference(which, "relu_maxpool")["p0"]
    with on_path(path):
        a, b = build(text, batch, False, p0, seed=seed), build(text, batch, True, p0, seed=seed)
        for i, seed in enumerate((101, 202)):
            ra, rb = one_pass(a, seed), one_pass(b, seed)
            dropped = 0
            for l in a.layers_:
                n = l.GetName()
                if l.dropprob_ > 0:
                    assert type(l) is ReLULayer and l.HasSlices() and not l.store_dropout_noise_
                    # a ReLU unit is 0 where it was dropped or where it did not fire: the two hosts must agree on both
                    ma, mb = ra["states"][n] == 0, rb["states"][n] == 0
                    assert np.array_equal(ma, mb), ("dropout masks differ", n, i)
                    assert 0.25 < ma.mean() < 0.95
                    kept = ~ma
                    assert np.all(ra["derivs"][n][ma] == 0) and np.all(rb["derivs"][n][mb] == 0) and kept.any()
                    dropped += 1
                assert rel_err(ra["states"][n], rb["states"][n]) < 1e-5, ("state fused vs unfused", n, i)
                if n in ra["derivs"]:
                    assert rel_err(ra["derivs"][n], rb["derivs"][n]) < 1e-5, ("deriv fused vs unfused", n, i)
            assert dropped == (1 if which == "inception" else 2)
            assert rel_err(ra["grads"], rb["grads"]) < 1e-5, ("gradients fused vs unfused", i)
            a.UpdateWeights()
            b.UpdateWeights()
            assert rel_err(a.parameters_.ToNumpy(), b.parameters_.ToNumpy()) < 1e-6
            b.parameters_.Set(a.parameters_)
            for ea, eb in zip(a.edges_, b.edges_):
                if hasattr(ea, "weight_optimizer_"):
                    eb.weight_optimizer_.gradient_history_.Set(ea.weight_optimizer_.gradient_history_)
                    eb.bias_optimizer_.gradient_history_.Set(ea.bias_optimizer_.gradient_history_)
    # the fused net did plan the epilogues this test is about
    sliced = [l for l in b.layers_ if l.HasSlices()]
    assert sliced and all(b.plan_[l].fuse_relu is True for l in sliced)
    if which != "inception":
        assert b.plan_[b.GetLayerByName("h1")].down_scale == pytest.approx(1 / 0.75)


def test_the_pooled_branch_runs_the_mask_pair_on_a_view(gpu, reference):
    """inception_small with a max-pooled branch into the concat layer: the fused host records and uses the window masks on the slice."""
    ref = reference("inception_pooled", "relu_maxpool")
    net = build(ref["text"], ref["batch"], True, ref["p0"], seed=ref["seed"])
    e = net.GetEdgeByName("stem:mix_pool")
    assert e.MaskEligible() and e.GetDestSliceName() == "pool"
    view = net.GetLayerByName("mix").GetState("pool")
    assert view.mat_.data_device != net.GetLayerByName("mix").GetState().mat_.data_device and list(view.shape_.shape) == [8, 6, 6, 8]
    rows = _timer_names(lambda: one_pass(net))
    kernels = {r["kernel"] for r in rows}
    print(sorted(kernels))
    assert {"pool_fwd_mask_kernel<max>", "pool_undo_mask_kernel<max>"} <= kernels
    assert e.mask_for_ is not None and e.mask_for_[1] == view.mat_.data_device and not e.mask_refused_
    assert_slices_close(net, net.grad_parameters_.ToNumpy().reshape(-1), ref["g0"], TOL, "gradient inception_pooled fused")


@pytest.mark.parametrize("path", list(PATHS))
def test_grad_checker_verdicts_equal_the_reference_checker(gpu, cpu_host, tmp_path, path):
    from convnet_amd.grad_check import GradChecker
    batch = 5
    text = nets.net_a(nets.LINEAR, grad_check=True)
    m, d = ref_host.write_configs(tmp_path, text, batch, 1, SEED, "gc")
    p0 = cpu_host.init_params(m, d)
    out = os.path.join(str(tmp_path), "gc_cpu.h5")
    flags = cpu_host.grad_check_fixed(m, d, p0, out)
    names = ["input:h1_a", "input:h1_b", "h1_a:h2_a", "h1_b:h2_b", "pool:output"]      # the datasets carry Edge::GetName()
    res = ref_host.read_grad_check(out, names)
    assert len(flags) == len(names)
    _, _, loss = cpu_host.train(m, d, 1, p0)
    quantum = float(np.spacing(np.float32(loss[0]))) / (2 * 0.03 * batch)
    for name in names:
        for kind, (a, n) in res[name].items():
            crit = ref_host.grad_check_criterion(a, n)
            u = float(np.mean(4 * quantum / np.abs(a)))
            print(name, kind, "reference criterion", crit, "rounding allowance", u)
            assert len(crit) == 1 and crit[0] + u < 0.005, ("the reference's verdict is not clear of the 1 % limit", name, kind, crit, u)
    with on_path(path):
        net = build(text, batch, False, p0, cls=GradChecker, num_batches=1)
        port = net.Run(fixed_batch=True)
    assert sorted(port) == sorted(names)
    for name, (fw, fb) in zip(names, flags):
        for kind, passed in (("weights", fw), ("bias", fb)):
            p_pass, p_a, _ = port[name][kind]
            a_cpu, n_cpu = res[name][kind]
            print(name, kind, "reference", passed, ref_host.grad_check_criterion(a_cpu, n_cpu), "port", p_pass)
            assert rel_err(p_a, a_cpu) < TOL, ("analytic gradient", name, kind)
            assert bool(p_pass) == passed, ("verdict", name, kind, p_pass, passed)
    assert all(v for pair in flags for v in pair)


def test_reference_host_on_this_library_runs_net_a_through_its_own_slices(gpu, reference, tmp_path):
    """The drop-in demonstration: the reference's unmodified host (its own Layer::SetupSlices / GetSlice calls) on this library through
    the C ABI, against its CPU run — the pattern of test_reference_host.py."""
    assert os.path.exists(ref_host.HIP_SO), "oracle/_ref/libref_host_hip.so missing: run __graft_entry__.build() where the reference tree exists"
    from convnet_amd import _lib     # loads libconvnet_hip.so after torch (one HIP runtime)
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    hip_host = ref_host.RefHost(ref_host.HIP_SO)
    for kinds in KINDS:
        ref = reference("A", kinds)
        net = build(ref["text"], ref["batch"], False, seed=ref["seed"])      # (for the edges' offsets in the flat buffers only)
        g0 = hip_host.gradient(ref["m"], ref["d"], ref["p0"])
        assert_slices_close(net, g0, ref["g0"], TOL, f"reference host on this library: gradient {kinds}")
        p3, metric, loss = hip_host.train(ref["m"], ref["d"], STEPS, ref["p0"])
        assert_slices_close(net, p3, ref["p3"], TOL, f"reference host on this library: parameters after {STEPS} steps {kinds}")
        assert rel_err(loss, ref["loss"]) < TOL, (loss, ref["loss"])
        assert metric == ref["metric"]


def test_a_sliced_net_resumes_from_its_checkpoint(gpu, reference, tmp_path):
    """Net A after one step: Save, Load into a fresh net, and the next step of the two is bit-identical — both groups of h2 (two edges
    between the same two layers) have their own datasets."""
    ref = reference("A", "relu_maxpool")
    a = build(ref["text"], ref["batch"], True, ref["p0"], seed=ref["seed"])
    a.TrainOneBatch()
    path = os.path.join(str(tmp_path), "net_a.h5")
    a.Save(path)
    b = build(ref["text"], ref["batch"], True, seed=ref["seed"])
    b.Load(path)
    assert b.current_iter_ == 1
    pa, pb = a.parameters_.ToNumpy().reshape(-1), b.parameters_.ToNumpy().reshape(-1)
    for e, (off, n) in a.edge_slices_.items():       # (the 128-float padding between the edges' slices is never written: skip it)
        assert np.array_equal(pa[off:off + n], pb[off:off + n]), ("loaded", e.GetName())
    b.train_dataset_.Seek(ref["batch"])
    a.TrainOneBatch()
    b.TrainOneBatch()
    pa2, pb2 = a.parameters_.ToNumpy().reshape(-1), b.parameters_.ToNumpy().reshape(-1)
    for e, (off, n) in a.edge_slices_.items():
        assert np.array_equal(pa2[off:off + n], pb2[off:off + n]), ("next step", e.GetName())
        assert not np.array_equal(pa2[off:off + n], pa[off:off + n])
