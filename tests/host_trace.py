"""The host's library-call trace, recorded without a GPU.

The host classes (convnet.py / edge.py / layer.py / optimizer.py) only issue library calls through ``Matrix``, so "a host change leaves
behaviour as it was" can be checked exactly: ``convnet_amd.matrix.lib`` is swapped for a recorder, ``Matrix`` storage is backed by CPU
tensors, and every call becomes one canonical line — the entry name, each matrix as (allocation index, offset in floats, rows, cols,
is_trans), ``Shape4D`` and ``ConvDesc`` field by field, every scalar (floats as ``float.hex()``).  The recorder answers success to every
entry; ``get_slice`` / ``reshape`` are carried out on the ``cudamat`` structs (and recorded: the deferred epilogues flush on them);
``MaxPoolMask`` answers ERROR_UNSUPPORTED unless the window is 3 x 3 with stride 2 and the batch a multiple of 4 (include/convnet_hip.h).

Traced per net: build, SetBatchsize, AllocateMemory, a do-nothing dataset, two TrainOneBatch, one Fprop(False).  Modes that need streams
and events (overlap_wgrad, overlap_update, a gradient exchange) cannot be reached here; tests/test_net_gpu.py and the data-parallel
tests pin those bit for bit.

tests/test_host_trace_cpu.py compares the traces with tests/golden/host_trace.json.  Only the public surface of the package is used, so
the same file runs on another checkout:  python tests/host_trace.py NET [--fused]  dumps a trace for diffing,  --list  names the nets,
--golden  prints the JSON of every (net, fused) pair."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from convnet_amd import _lib, matrix, models  # noqa: E402
from convnet_amd.convnet import ConvNet  # noqa: E402
from convnet_amd.matrix import Matrix  # noqa: E402

ERROR_UNSUPPORTED = -9


class Recorder:
    """Stands in for the ctypes library object: every attribute is an entry that records its arguments and returns 0."""

    def __init__(self):
        self.lines = []
        self.allocs = []   # (first byte, one past the last, the tensor: kept alive so that no address is handed out twice)

    def register(self, m):
        base = m.mat_.data_device
        if m._t is not None and not any(a <= base < b for a, b, _ in self.allocs):
            self.allocs.append((base, base + 4 * m._t.numel(), m._t))

    def _mat(self, m):
        p = m.data_device
        if p is None:
            where = "unallocated"
        else:
            where = next((f"{i}+{(p - a) // 4}" for i, (a, b, _) in enumerate(self.allocs) if a <= p < b), None)
            if where is None:
                raise AssertionError("a matrix outside every allocation reached the library")
        return f"M({where},{m.size[0]},{m.size[1]},{m.is_trans})"

    def _arg(self, a):
        if a is None:
            return "null"
        if isinstance(a, bool):
            return f"b{int(a)}"
        if isinstance(a, int):
            return f"i{a}"
        if isinstance(a, float):
            return "f" + a.hex()
        if isinstance(a, bytes):
            return repr(a)
        if isinstance(a, _lib.cudamat):
            return self._mat(a)
        if isinstance(a, _lib.Shape4D):
            return "S(" + ",".join(str(v) for v in a.shape) + ")"
        if isinstance(a, _lib.ConvDesc):
            return "D(" + ",".join(f"{n}={getattr(a, n)}" for n, _ in a._fields_) + ")"
        if isinstance(a, _lib.rnd_struct):
            return "rnd"
        if isinstance(a, ctypes.Array):
            return "[" + ",".join(self._arg(v) for v in a) + "]"
        if isinstance(a, ctypes._Pointer):
            return self._arg(a.contents) if a else "null"
        if isinstance(a, ctypes._SimpleCData):
            return type(a).__name__ if isinstance(a, (ctypes.c_void_p, ctypes.c_int)) else self._arg(a.value)
        if hasattr(a, "_obj"):   # ctypes.byref(...)
            return self._arg(a._obj)
        raise AssertionError(f"unexpected argument type {type(a).__name__}")

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            self.lines.append(name + " " + " ".join(self._arg(a) for a in args))
            do = getattr(Recorder, "_do_" + name, None)
            return do(*args) if do else 0
        return entry

    # the two entries whose effect the host reads back (csrc/state.hip: both work on the struct alone)
    @staticmethod
    def _do_reshape(mat, m, n):
        mat = mat._obj
        total = mat.size[0] * mat.size[1]
        if m < 0 and n < 0:
            return -6
        if m < 0:
            m = total // n
        if n < 0:
            n = total // m
        if total != m * n:
            return -1
        mat.size[0], mat.size[1] = m, n
        return 0

    @staticmethod
    def _do_get_slice(source, target, first_col, last_col):
        s, t = source._obj, target._obj
        if s.is_trans:
            return -5
        if last_col > s.size[1] or first_col >= last_col:
            return -1
        rows = s.size[0]
        t.data_host = None
        t.data_device = s.data_device + 4 * first_col * rows
        t.on_device, t.on_host = 1, 0
        t.size[0], t.size[1] = rows, last_col - first_col
        t.is_trans = t.owns_data = t.tex_obj = 0
        return 0

    @staticmethod
    def _do_MaxPoolMask(images, targets, mask, images_shape, targets_shape, d):
        ok = (d.kernel_size_y, d.kernel_size_x, d.stride_y, d.stride_x) == (3, 3, 2, 2) and images._obj.size[0] % 4 == 0
        return 0 if ok else ERROR_UNSUPPORTED


class _NoData:
    """A dataset that leaves the layers as they are."""

    def __init__(self, batch):
        self.batch = batch

    def GetBatchSize(self):
        return self.batch

    def GetBatch(self, data_layers):
        pass


def trace(text, batch, fused):
    """The canonical lines of: build, allocate, two training steps, one test-time forward pass."""
    rec = Recorder()
    saved = (matrix.lib, Matrix._device, Matrix.AllocateGPUMemory, Matrix._temp, Matrix._temp_size, Matrix._ones, Matrix._ones_size)
    allocate = Matrix.AllocateGPUMemory

    def allocate_and_register(self, rows, cols, name=""):
        allocate(self, rows, cols, name)
        rec.register(self)

    matrix.lib = rec
    Matrix._device = torch.device("cpu")
    Matrix.AllocateGPUMemory = allocate_and_register
    Matrix._temp = Matrix._ones = None      # the process-wide pools start empty for every net: a trace does not depend on the one before
    Matrix._temp_size = Matrix._ones_size = 0
    try:
        net = ConvNet(text, fused=fused)
        net.SetBatchsize(batch)
        net.SetupDataset(_NoData(batch))
        net.AllocateMemory(False)
        for _ in range(2):
            rec.lines.append("# TrainOneBatch")
            loss = net.TrainOneBatch()
            rec.lines.append("# loss " + ("None" if loss is None else f"list of {len(loss)}"))
        rec.lines.append("# Fprop(False)")
        for l in net.layers_:
            l.ResetAddOrOverwrite()
        net.Fprop(False)
    finally:
        (matrix.lib, Matrix._device, Matrix.AllocateGPUMemory, Matrix._temp, Matrix._temp_size, Matrix._ones, Matrix._ones_size) = saved
    return rec.lines


def _edit(text, edge, old, new):
    """The model text with ``old`` replaced by ``new`` inside the edges whose block contains ``edge`` (all edges of a type, or one by its
    source line)."""
    blocks = text.split("edge {")
    out = [blocks[0]]
    for b in blocks[1:]:
        if edge in b:
            assert old in b, (edge, old)
            b = b.replace(old, new, 1)
        out.append(b)
    return "edge {".join(out)


def _tied_fc_nin():
    """Two FC edges into one layer sharing their weights, and two 1 x 1 edges sharing theirs."""
    L, C, F, NIN = models._layer, models._conv, models._fc, models._nin
    R = "RECTIFIED_LINEAR"
    s = models._header("tied_fc_nin") + L("input", 3, size=8)
    s += L("c1", 8, R) + L("n1", 8, R) + L("n2", 8, R) + L("f1", 16, R) + L("f2", 16, R) + L("output", 5, "SOFTMAX")
    s += C("input", "c1", 3, 1, 1) + NIN("c1", "n1") + NIN("n1", "n2", grad_check='  tied_to: "c1:n1"\n')
    s += F("n1", "f1") + F("n2", "f2", grad_check='  tied_to: "n1:f1"\n') + F("f1", "output") + F("f2", "output")
    return s


def nets():
    """name -> (model text, batch)."""
    from fused_host_nets import CONFIGS
    from test_data_parallel_gpu import tied_net
    from test_local_cpu import _local_net
    from test_net_gpu import small_alexnet
    conv, fc, nin = "edge_type: CONVOLUTIONAL\n", "edge_type: FC\n", "edge_type: CONV_ONETOONE\n"
    no_bias = "  has_no_bias: true\n"
    out = {f"configs/{k}": v for k, v in CONFIGS.items()}
    out["alexnet67_dropout"] = (models.alexnet(image_size=67), 8)
    out["alexnet224"] = (models.alexnet(), 4)
    out["vgg224"] = (models.vgg(), 4)
    out["vgg_bn224"] = (models.vgg_bn(), 4)
    small = {
        "nin67": models.alexnet_nin(image_size=67), "nin67_no_dropout": models.alexnet_nin(image_size=67, num_classes=10, dropout=False),
        "mnist_conv": models.mnist_conv(), "lenet5": models.lenet5(), "cifar_local": models.cifar_local(),
        "small_bn": models.small_bn(), "small_bn_linear": models.small_bn(relu=False),
        "video_small": models.video_small(),
        "video_small_conv1_bias_per_location": _edit(models.video_small(), 'source: "input"', "shared_bias: true", "shared_bias: false"),
        "video_small_bias_per_location": _edit(models.video_small(), conv, "shared_bias: true", "shared_bias: false"),
        "video_small_no_bias": _edit(models.video_small(), conv, conv, conv + no_bias),
        "multilabel_small": models.multilabel_small(), "multilabel_small_dropout": models.multilabel_small(dropprob=0.3),
        "softdist_small": models.softdist_small(), "softdist_small_dropout": models.softdist_small(dropprob=0.3),
        "tied_conv": tied_net(), "tied_fc_nin": _tied_fc_nin(),
        "local": _local_net(), "local_tied": _local_net(tie=True), "local_no_bias": _local_net(bias=False),
        "small_alexnet": small_alexnet(), "small_alexnet_dropout": small_alexnet(dropprob=0.5),
        "small_alexnet_bias_per_location": _edit(small_alexnet(), conv, "shared_bias: true", "shared_bias: false"),
        "small_alexnet_conv_no_bias": _edit(small_alexnet(), conv, conv, conv + no_bias),
        "small_alexnet_fc_no_bias": _edit(small_alexnet(), fc, fc, fc + no_bias),
        "nin_no_bias": _edit(CONFIGS["c_into_nin"][0], nin, nin, nin + no_bias),
    }
    out.update({k: (v, 8) for k, v in small.items()})
    return out


def digest(lines):
    """What the golden file keeps of a trace: the call count, the SHA-256 of the whole, and three hex digits of each line's own SHA-256
    (enough to name the first line that differs without storing the lines)."""
    return {"calls": sum(not l.startswith("#") for l in lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(),
            "lines": "".join(hashlib.sha256(l.encode()).hexdigest()[:3] for l in lines)}


def key(name, fused):
    return f"{name} {'fused' if fused else 'unfused'}"


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--list" in args:
        print("\n".join(nets()))
    elif "--golden" in args:
        print(json.dumps({key(n, f): digest(trace(t, b, f)) for n, (t, b) in nets().items() for f in (True, False)}, indent=0))
    else:
        text, batch = nets()[args[0]]
        print("\n".join(trace(text, batch, "--fused" in args)))
