"""CPU: the Adagrad and RMSProp optimizers (convnet_amd/optimizer.py) against the reference's compiled optimizer on its CPU Matrix
(oracle/_ref/libref_host_cpu.so, tests/ref_host.py): one parameter step for step, a whole small net, what stays refused, and what an
SGD-only net allocates."""
import os
import zlib

import numpy as np
import pytest

import oracle
import ref_host
from golden_cases import rel_err
from test_net_gpu import small_alexnet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_host_tiny_alex.npz")
# A different implementation of the same fp32 net against the reference's CPU run: the bound tests/test_reference_host.py puts on this
# repo's host against that run (its TOL, "python host vs reference CPU run"), the reference's own cross-implementation tolerance
# (py/test_conv.py:382-392).  The 1e-6 of test_reference_cpu_host_reproduces_the_committed_golden_run compares one binary with itself.
TOL = 1e-4
f32 = np.float32


@pytest.fixture(scope="module")
def cpu_host():
    if not os.path.exists(ref_host.CPU_SO):
        pytest.skip("oracle/_ref/libref_host_cpu.so not built (needs the reference tree at build time)")
    return ref_host.RefHost(ref_host.CPU_SO)


class NumpyMatrix:
    """The Matrix methods the three optimizers' unfused paths call (src/optimizer.cc:174-279), on a column-major numpy array in
    float32, every statement one rounded operation."""

    def __init__(self, a):
        self.a = np.array(a, np.float32)          # (cols, rows): column-major (rows, cols)

    def GetNumEls(self):
        return self.a.size

    def Set(self, v):
        self.a[...] = f32(v)

    def Mult(self, v):
        self.a *= f32(v)

    def Add(self, other, mult=1.0):
        self.a += f32(mult) * other.a

    def Divide(self, other):
        self.a /= other.a

    def UpperBoundMod(self, v):
        np.clip(self.a, -f32(v), f32(v), out=self.a)

    def NormLimitByAxis(self, axis, val, constraint):
        assert axis == 1
        oracle.port.normlimit_rows(self.a, val, constraint)

    @staticmethod
    def AdagradUpdate(history, gradient, delta):
        c = history.a - f32(delta)
        history.a[...] = f32(delta) + np.sqrt(c * c + gradient.a * gradient.a)

    @staticmethod
    def RMSPropUpdate(history, gradient, factor):
        h, g = history.a, gradient.a
        history.a[...] = np.sqrt(f32(factor) * h * h + (f32(1) - f32(factor)) * g * g)


_A, _R = "optimizer_type: ADAGRAD_SGD ", "optimizer_type: RMSPROP_SGD rms_prop_factor: 0.9 "
_PLAIN = "epsilon: 0.05 initial_momentum: 0.9 final_momentum: 0.9 l2_decay: 0.01"
_LATE = "epsilon: 0.1 start_optimization_after: 2 gradient_clip: 0.3 final_momentum: 0.8"
_DECAY = ("epsilon: 0.05 epsilon_decay: EXPONENTIAL epsilon_decay_timescale: 4 initial_momentum: 0.5 final_momentum: 0.9 "
          "momentum_transition_timescale: 3 l2_decay: 0.001")
_LIMIT = "epsilon: 0.2 final_momentum: 0.5 weight_norm_limit: 1.2"
CONFIGS = {
    "adagrad_momentum_l2": _A + _PLAIN, "rmsprop_momentum_l2": _R + _PLAIN,
    "adagrad_clip_late_start": _A + _LATE, "rmsprop_clip_late_start": _R + _LATE,
    "adagrad_decay_momentum_transition": _A + _DECAY, "rmsprop_decay_momentum_transition": _R + _DECAY,
    "adagrad_norm_limit": _A + _LIMIT, "rmsprop_norm_limit": _R + _LIMIT,
    "adagrad_nesterov": _A + "epsilon: 0.05 initial_momentum: 0.6 final_momentum: 0.9 momentum_transition_timescale: 5 "
                             "nesterov_momentum: true l2_decay: 0.002",
    "adagrad_delta": _A + "adagrad_delta: 0.1 epsilon: 0.05 final_momentum: 0.9 l2_decay: 0.01",
    "rmsprop_nesterov_flag": _R + "epsilon: 0.05 final_momentum: 0.9 nesterov_momentum: true",
}


def _numpy_optimizer(text, like):
    from convnet_amd import pbtxt
    from convnet_amd.optimizer import Optimizer
    opt = Optimizer.ChooseOptimizer(pbtxt.parse(text, cls=pbtxt.Optimizer))
    opt.gradient_history_ = NumpyMatrix(np.zeros_like(like))
    opt.second_history_ = NumpyMatrix(np.full_like(like, opt.second_history_initial_))
    return opt


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_python_optimizer_follows_the_reference_optimizer_step_for_step(cpu_host, name):
    """Schedules, op order, the histories' initial values, Adagrad's update before start_optimization_after, RMSProp's disregard of
    nesterov_momentum inside Optimize: the same parameter, bit for bit, after each of 10 steps.  (The numpy restatement above reproduces
    the oracle build exactly in every config: no config needed a tolerance.)"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rows, cols, steps = 7, 13, 10
    w0 = rng.standard_normal((cols, rows)).astype(np.float32)
    grads = rng.standard_normal((steps, cols, rows)).astype(np.float32)
    want = cpu_host.sgd(CONFIGS[name], w0, grads)
    opt = _numpy_optimizer(CONFIGS[name], w0)
    w = NumpyMatrix(w0)
    for t in range(steps):
        opt.NotifyStart(w)
        opt.Optimize(NumpyMatrix(grads[t]), w)
        assert np.array_equal(w.a, want[t]), (name, t, rel_err(w.a, want[t]))
    assert opt.step_ == steps


def _with_optimizer(text, kind):
    extra = {"ADAGRAD_SGD": "", "RMSPROP_SGD": "    rms_prop_factor: 0.9\n"}[kind]
    out = text.replace("optimizer {\n", "optimizer {\n    optimizer_type: " + kind + "\n" + extra)
    assert out.count(kind) == text.count("optimizer {\n") > 0
    return out


class _Host:
    def __init__(self, a):
        self.a = a

    def ToNumpy(self):
        return self.a


@pytest.mark.parametrize("kind", ["ADAGRAD_SGD", "RMSPROP_SGD"])
def test_small_net_trains_like_the_reference_cpu_host(cpu_host, tmp_path, kind):
    """The AlexNet-topology test net with every optimizer switched: gradients from the CPU oracle on this repo's graph
    (tests/oracle_net.py), steps from this repo's optimizers on numpy, against 3 x ConvNet::TrainOneBatch of the reference's CPU host
    from the same parameters and batches."""
    from convnet_amd.convnet import ConvNet
    from convnet_amd.edge import ConvEdge, EdgeWithWeight
    from oracle_net import forward_backward
    g = np.load(GOLDEN)
    batch, num_batches, seed, _ = (int(v) for v in g["cfg"])
    text, steps = _with_optimizer(small_alexnet(), kind), 3
    m, d = ref_host.write_configs(tmp_path, text, batch, num_batches, seed)
    want, _, _ = cpu_host.train(m, d, steps, g["p0"])

    net = ConvNet(text, fused=False)
    p = g["p0"].copy()
    state, off = [], 0
    for e in net.edges_:
        if not isinstance(e, EdgeWithWeight):
            continue
        n = e.GetParameterMemoryRequirement()
        F = e.GetDest().GetNumChannels()
        nw = n - F
        w, b = p[off:off + nw], p[off + nw:off + n]
        e.GetWeight = (lambda a: lambda: _Host(a))(w if isinstance(e, ConvEdge) else w.reshape(-1, F))
        e.GetBias = (lambda a: lambda: _Host(a))(b)
        for opt, view in ((e.weight_optimizer_, w.reshape(-1, F)), (e.bias_optimizer_, b.reshape(F, 1))):
            assert type(opt).__name__ == {"ADAGRAD_SGD": "AdagradSGDOptimizer", "RMSPROP_SGD": "RMSPropSGDOptimizer"}[kind]
            opt.gradient_history_ = NumpyMatrix(np.zeros_like(view))
            opt.second_history_ = NumpyMatrix(np.full_like(view, opt.second_history_initial_))
        state.append((e, w, b, F))
        off += (n + 127) // 128 * 128
    assert off == p.size
    inp, out = net.input_layers_[0], net.output_layers_[0]
    dims = inp.GetNumChannels() * inp.GetSizeY() * inp.GetSizeX()
    for t in range(steps):
        x = ref_host.hash_batch(seed, t % num_batches, dims * batch, True)
        labels = ref_host.hash_batch(seed, t % num_batches, batch, False, out.GetNumChannels())
        _, _, grads = forward_backward(net, x, labels)
        for e, w, b, F in state:
            dw, db = grads[e.GetName()]
            for opt, param, grad in ((e.weight_optimizer_, w, dw.reshape(-1, F)), (e.bias_optimizer_, b, np.asarray(db).reshape(F, 1))):
                pm = NumpyMatrix(param.reshape(grad.shape))
                opt.Optimize(NumpyMatrix(grad), pm)
                param[...] = pm.a.reshape(-1)
    assert not np.array_equal(p, g["p0"])
    off = 0
    for e, w, b, F in state:
        n = w.size + b.size
        err = rel_err(p[off:off + n], want[off:off + n])
        print(kind, e.GetName(), "rel_err", err)
        assert err < TOL, (kind, e.GetName(), err)
        off += (n + 127) // 128 * 128


@pytest.mark.parametrize("text,word", [("optimizer_type: LBFGS epsilon: 0.1", "LBFGS"), ("epsilon: 0.1 shared_prior: true", "shared_prior"),
                                       ("optimizer_type: ADAGRAD_SGD epsilon: 0.1 shared_prior: true", "shared_prior")])
def test_out_of_scope_optimizers_are_refused_by_name(text, word):
    from convnet_amd import pbtxt
    from convnet_amd.optimizer import Optimizer
    with pytest.raises(SystemExit, match=word):
        Optimizer.ChooseOptimizer(pbtxt.parse(text, cls=pbtxt.Optimizer))


class _CountingMatrix:
    """Stands in for convnet.Matrix while ConvNet.AllocateEdgeMemory runs: records what is allocated, does nothing."""
    allocated = []

    def AllocateGPUMemory(self, rows, cols, name=""):
        _CountingMatrix.allocated.append((name, rows * cols))

    def GetSlice(self, s, a, b):
        pass

    def Set(self, v):
        pass


def _flat_buffers(text, monkeypatch):
    from convnet_amd import convnet
    net = convnet.ConvNet(text)
    _CountingMatrix.allocated = []
    net.parameters_, net.grad_parameters_, net.history_, net.second_history_ = (_CountingMatrix() for _ in range(4))
    for e in net.edges_:
        e.SetMemory = e.SetGradMemory = e.Initialize = lambda *a: None
    with monkeypatch.context() as mp:
        mp.setattr(convnet, "Matrix", _CountingMatrix)
        net.AllocateEdgeMemory(False)
    return [name for name, _ in _CountingMatrix.allocated], {n for _, n in _CountingMatrix.allocated}


def test_sgd_only_net_allocates_no_second_history_buffer(monkeypatch):
    names, sizes = _flat_buffers(small_alexnet(), monkeypatch)
    assert names == ["parameters", "grad parameters", "optimizer history"]
    names, sizes = _flat_buffers(_with_optimizer(small_alexnet(), "ADAGRAD_SGD"), monkeypatch)
    assert names == ["parameters", "grad parameters", "optimizer history", "optimizer second-moment history"] and len(sizes) == 1
    # one Adagrad bias optimizer is enough
    text = small_alexnet().replace("bias_optimizer {\n", "bias_optimizer {\n    optimizer_type: ADAGRAD_SGD\n", 1)
    assert len(_flat_buffers(text, monkeypatch)[0]) == 4


def test_fused_steps_are_planned_and_launched_per_optimizer_kind(monkeypatch):
    """PlanFusedStep of an Adagrad / RMSProp optimizer yields its own kind of item (never a plain SGD item), and RunFusedSteps hands each
    kind to its own multi launch: SGD items still go to Matrix.SGDMomentumStepMulti in one call."""
    from convnet_amd import optimizer as O
    from convnet_amd import pbtxt
    from convnet_amd.matrix import Matrix
    items = []
    for text, cls in ((_PLAIN, O.SGDStep), (_A + _PLAIN, O.AdagradStep), (_R + _PLAIN, O.RMSPropStep), (_PLAIN, O.SGDStep)):
        opt = O.Optimizer.ChooseOptimizer(pbtxt.parse(text, cls=pbtxt.Optimizer))
        assert opt.PlanFusedStep(Matrix(), Matrix()) is None and opt.step_ == 0      # unfused host: Optimize runs
        opt.fused = True
        g, p = Matrix(), Matrix()
        item = opt.PlanFusedStep(g, p)
        assert type(item) is cls and item[0] is g and item[1] is p and opt.step_ == 1
        items.append(item)
    assert items[1].step_scale == 1.0 and items[1].delta == 1.0 and items[2].factor == f32(0.9)
    calls = []
    for name in ("SGDMomentumStepMulti", "AdagradMomentumStepMulti", "RMSPropMomentumStepMulti"):
        monkeypatch.setattr(Matrix, name, staticmethod((lambda n: lambda its: calls.append((n, list(its))))(name)))
    O.RunFusedSteps(items)
    assert sorted(calls) == sorted([("SGDMomentumStepMulti", [items[0], items[3]]), ("AdagradMomentumStepMulti", [items[1]]),
                                    ("RMSPropMomentumStepMulti", [items[2]])])
    calls.clear()
    O.RunFusedSteps([items[0], items[3]])
    assert calls == [("SGDMomentumStepMulti", [items[0], items[3]])]
