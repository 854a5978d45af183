"""GPU: whole nets with logistic and softmax-distribution layers (models.multilabel_small, models.softdist_small) through the python
host, unfused and fused, on both matrix paths, against the reference's unmodified host on its CPU Matrix
(oracle/_ref/libref_host_cpu.so through tests/ref_host.py): same pbtxt, the reference's own initial parameters, the very batches its
data shim generates (ref_host.hash_batch; an output layer's data is batch * num_channels values in [0, num_channels)).

 * the flat gradient of one Fprop(train) / ComputeDeriv / Bprop;
 * after 3 x TrainOneBatch: parameters, per-step loss (0 for CROSS_ENTROPY_BINARY, as the reference reports it) and the summed metric;
   metric golden_cases.rel_err, bound 1e-4 — the reference's own, as in the existing whole-net tests;
 * fused against unfused with dropout on the logistic hidden layers: identical masks, then states, derivatives and gradients to 1e-5;
 * the python GradChecker's verdicts against the reference's compiled GradChecker at the same parameters and batch, on
   multilabel_small with a softmax head (CROSS_ENTROPY_BINARY reports no loss to difference).

The grad-check verdict is a 1 % threshold on difference quotients of an fp32 loss.  Every numerical gradient is a multiple of the
quantum Q = ulp(loss) / (2 eps batch) (~ 1e-6 here at eps = 0.03: loss ~ 14, batch 16), and two fp32 machines that sum the 16 cases'
cross entropies in different orders differ by a few ulp in each of the two losses, i.e. by up to ~ 4 Q per gradient entry, which moves
the reference's criterion (the mean of |analytic - numeric| / |mean of the two|) by up to u = mean(4 Q / |analytic|).  A verdict is
determined by the net, and not by the rounding of the loss, only where criterion + u stays on one side of the limit: the test first
asserts that on the reference's own CPU figures (criterion + u < half the limit for every check), then demands equal verdicts.
models.multilabel_small is smooth (sigmoid units, average pooling) and initialised so that this holds."""
import os

import numpy as np
import pytest

import ref_host
from golden_cases import rel_err

pytestmark = pytest.mark.gpu

BATCH, SEED, STEPS, TOL = 16, 9, 3, 1e-4
PATHS = {"split": 1, "fp32": 0}


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


def model_text(which, dropprob=0.0, grad_check=False):
    from convnet_amd import models
    return getattr(models, which)(image_size=12, dropprob=dropprob, grad_check=grad_check)


class HashData:
    """The data shim's batches for the python host: every data layer's matrix filled in its flat (column-major) order."""

    def __init__(self, net, batch, num_batches, seed):
        from convnet_amd.matrix import Matrix
        self.batch_size_, self.pos_, self.batches_ = batch, 0, []
        for b in range(num_batches):
            per = {}
            for l in net.data_layers_:
                dest = l.GetState() if l.IsInput() else l.GetData()
                m = Matrix()
                m.AllocateGPUMemory(dest.GetRows(), dest.GetCols())
                m.FromNumpy(ref_host.hash_batch(seed, b, dest.GetNumEls(), l.IsInput(), l.GetNumChannels()))
                per[l.GetName()] = m
            self.batches_.append(per)

    def GetBatchSize(self):
        return self.batch_size_

    def GetDataSetSize(self):
        return self.batch_size_ * len(self.batches_)

    def Seek(self, row):
        self.pos_ = row // self.batch_size_

    def Sync(self):
        pass

    def GetBatch(self, data_layers):
        b = self.batches_[self.pos_ % len(self.batches_)]
        self.pos_ += 1
        for l in data_layers:
            (l.GetState() if l.IsInput() else l.GetData()).Set(b[l.GetName()])


def build(text, fused, params=None, cls=None, num_batches=2):
    from convnet_amd.convnet import ConvNet
    net = (cls or ConvNet)(text, fused=fused)
    net.SetBatchsize(BATCH)
    net.AllocateLayerMemory()                      # the data layers' shapes, which the batches follow
    net.SetupDataset(HashData(net, BATCH, num_batches, SEED))
    net.AllocateMemory(False)
    if params is not None:
        assert net.parameters_.GetNumEls() == params.size
        net.parameters_.FromNumpy(params.reshape(1, -1))
    return net


class on_path:
    def __init__(self, path):
        self.path = PATHS[path]

    def __enter__(self):
        from convnet_amd import _lib
        _lib.lib.convnet_hip_set_matrix_path(self.path)

    def __exit__(self, *exc):
        from convnet_amd import _lib
        _lib.lib.convnet_hip_set_matrix_path(1)


def assert_slices_close(net, got, want, tol, what):
    assert got.size == want.size
    for e, (off, n) in net.edge_slices_.items():
        err = rel_err(got[off:off + n], want[off:off + n])
        print(what, e.GetName(), "rel_err", err)
        assert err < tol, (what, e.GetName(), err)


def one_pass(net, seed=None, train=True):
    """TrainOneBatch's sequence stopped before UpdateWeights."""
    from convnet_amd.matrix import Matrix
    if seed is not None:
        Matrix.InitRandom(seed)
    for l in net.layers_:
        l.ResetAddOrOverwrite()
    for e in net.edges_:
        e.NotifyStart()
    net.GetBatch(net.train_dataset_)
    net.Fprop(train)
    net.ComputeDeriv()
    net.Bprop()
    return dict(states={l.GetName(): l.GetState().ToNumpy().reshape(-1) for l in net.layers_},
                derivs={l.GetName(): l.GetDeriv().ToNumpy().reshape(-1) for l in net.layers_ if not l.IsInput()},
                grads=net.grad_parameters_.ToNumpy().reshape(-1).copy())


@pytest.fixture(scope="module")
def reference(cpu_host, tmp_path_factory):
    """The reference host's runs, once per model: initial parameters, gradient at them, the 3-step training run."""
    out = {}
    for which in ("multilabel_small", "softdist_small"):
        text = model_text(which)
        m, d = ref_host.write_configs(tmp_path_factory.mktemp(which), text, BATCH, 2, SEED, which)
        p0 = cpu_host.init_params(m, d)
        g0 = cpu_host.gradient(m, d, p0)
        p3, metric, loss = cpu_host.train(m, d, STEPS, p0)
        out[which] = dict(text=text, p0=p0, g0=g0, p3=p3, metric=metric, loss=np.asarray(loss, np.float64))
    return out


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", ["multilabel_small", "softdist_small"])
def test_gradient_equals_the_reference_host(gpu, reference, which, path, fused):
    ref = reference[which]
    assert np.any(ref["g0"]) and np.all(np.isfinite(ref["g0"]))
    with on_path(path):
        net = build(ref["text"], fused, ref["p0"])
        r = one_pass(net)
    assert_slices_close(net, r["grads"], ref["g0"], TOL, f"gradient {which} {path} fused={fused}")
    if which == "multilabel_small":
        t = net.output_layers_[0].GetData().ToNumpy()
        assert t.shape == (2, BATCH) and set(np.unique(t)) <= {0.0, 1.0}


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", ["multilabel_small", "softdist_small"])
def test_three_training_steps_equal_the_reference_host(gpu, reference, which, path, fused):
    ref = reference[which]
    with on_path(path):
        net = build(ref["text"], fused, ref["p0"])
        if fused:
            net.ReadCorrectCount()
        metric, loss = 0.0, []
        for _ in range(STEPS):
            err = net.TrainOneBatch()
            assert (err is None) == fused, "the fused host keeps the metric on the device"
            if err is not None:
                metric += sum(err)
            loss.append(sum(l.GetLoss() for l in net.output_layers_))
        if fused:
            metric = net.ReadCorrectCount()
        p3 = net.parameters_.ToNumpy().reshape(-1)
    print(which, path, fused, "loss", loss, ref["loss"].tolist(), "metric", metric, ref["metric"])
    assert_slices_close(net, p3, ref["p3"], TOL, f"parameters after {STEPS} steps {which} {path} fused={fused}")
    assert not np.array_equal(p3, ref["p0"])
    assert rel_err(loss, ref["loss"]) < TOL, (loss, ref["loss"])
    assert rel_err([metric], [ref["metric"]]) < TOL, (metric, ref["metric"])
    if which == "multilabel_small":
        assert np.all(ref["loss"] == 0) and 0 < ref["metric"] <= STEPS * BATCH      # binary cross entropy reports no loss
    else:
        assert np.all(ref["loss"] > 0)


@pytest.mark.parametrize("path", list(PATHS))
def test_fused_equals_unfused_with_dropout_on_the_logistic_layers(gpu, reference, path):
    from convnet_amd.layer import LogisticLayer
    text = model_text("multilabel_small", dropprob=0.25)
    p0 = reference["multilabel_small"]["p0"]
    with on_path(path):
        a, b = build(text, False, p0), build(text, True, p0)
        for i, seed in enumerate((101, 202)):
            ra, rb = one_pass(a, seed), one_pass(b, seed)
            dropped = 0
            for l in a.layers_:
                n = l.GetName()
                if l.dropprob_ > 0:
                    assert type(l) is LogisticLayer and not l.store_dropout_noise_
                    ma, mb = ra["states"][n] == 0, rb["states"][n] == 0      # a sigmoid is never 0: a zero state is a dropped unit
                    assert np.array_equal(ma, mb), ("dropout masks differ", n, i)
                    assert 0.1 < ma.mean() < 0.4
                    dropped += 1
                    # the derivative is taken at the dropout-scaled state: exactly 0 for a dropped unit
                    assert np.all(ra["derivs"][n][ma] == 0) and np.all(rb["derivs"][n][mb] == 0)
                assert rel_err(ra["states"][n], rb["states"][n]) < 1e-5, ("state fused vs unfused", n, i)
                if n in ra["derivs"]:
                    assert rel_err(ra["derivs"][n], rb["derivs"][n]) < 1e-5, ("deriv fused vs unfused", n, i)
            assert dropped == 2
            assert rel_err(ra["grads"], rb["grads"]) < 1e-5, ("gradients fused vs unfused", i)
            a.UpdateWeights()
            b.UpdateWeights()
            assert rel_err(a.parameters_.ToNumpy(), b.parameters_.ToNumpy()) < 1e-6
            b.parameters_.Set(a.parameters_)
            for ea, eb in zip(a.edges_, b.edges_):
                if hasattr(ea, "weight_optimizer_"):
                    eb.weight_optimizer_.gradient_history_.Set(ea.weight_optimizer_.gradient_history_)
                    eb.bias_optimizer_.gradient_history_.Set(ea.bias_optimizer_.gradient_history_)
        # Fprop(false): no dropout, same states
        for net in (a, b):
            for l in net.layers_:
                l.ResetAddOrOverwrite()
            net.GetBatch(net.train_dataset_)
            net.Fprop(False)
        for la, lb in zip(a.layers_, b.layers_):
            assert rel_err(la.GetState().ToNumpy(), lb.GetState().ToNumpy()) < 1e-5, ("Fprop(false)", la.GetName())
            if type(la) is LogisticLayer:
                assert not np.any(la.GetState().ToNumpy() == 0), ("dropout at test time", la.GetName())


@pytest.mark.parametrize("path", list(PATHS))
def test_grad_checker_verdicts_equal_the_reference_checker(gpu, cpu_host, tmp_path, path):
    from convnet_amd.grad_check import GradChecker
    text = model_text("multilabel_small", grad_check=True)
    head = "  activation: LOGISTIC\n  loss_function: CROSS_ENTROPY_BINARY\n  performance_metric: CLASSIFICATION_BINARY\n"
    assert text.count(head) == 1
    text = text.replace(head, "  activation: SOFTMAX\n")
    m, d = ref_host.write_configs(tmp_path, text, BATCH, 1, SEED, "gc")
    p0 = cpu_host.init_params(m, d)
    out = os.path.join(str(tmp_path), "gc_cpu.h5")
    flags = cpu_host.grad_check_fixed(m, d, p0, out)
    names = ["input:conv1", "pool1:fc2", "fc2:output"]
    assert len(flags) == len(names)
    res = ref_host.read_grad_check(out, names)
    # the premise (module docstring), from the reference's CPU run alone: every verdict is decided at the first epsilon, clear of the limit
    _, _, loss = cpu_host.train(m, d, 1, p0)
    quantum = float(np.spacing(np.float32(loss[0]))) / (2 * 0.03 * BATCH)
    for name in names:
        for kind, (a, n) in res[name].items():
            crit = ref_host.grad_check_criterion(a, n)
            u = float(np.mean(4 * quantum / np.abs(a)))
            print(name, kind, "reference criterion", crit, "rounding allowance", u)
            assert len(crit) == 1 and crit[0] + u < 0.005, ("the reference's verdict is not clear of the 1 % limit", name, kind, crit, u)
    with on_path(path):
        net = build(text, False, p0, cls=GradChecker, num_batches=1)
        port = net.Run(fixed_batch=True)
    by_edge = {f"{e.GetSource().GetName()}:{e.GetDest().GetName()}": port[e.GetName()] for e in net.edges_ if e.GetName() in port}
    for name, (fw, fb) in zip(names, flags):
        for kind, passed in (("weights", fw), ("bias", fb)):
            p_pass, p_a, _ = by_edge[name][kind]
            a_cpu, n_cpu = res[name][kind]
            print(name, kind, "reference", passed, ref_host.grad_check_criterion(a_cpu, n_cpu), "port", p_pass)
            assert rel_err(p_a, a_cpu) < TOL, ("analytic gradient", name, kind)
            assert bool(p_pass) == passed, ("verdict", name, kind, p_pass, passed)
    assert all(v for pair in flags for v in pair)
