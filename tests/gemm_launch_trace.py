"""What the GEMM launch layer (csrc/gather_gemm.hip from the host-side dispatch on, csrc/patch_gemm.hip from patch_mode() on) does for
a fixed list of calls, recorded on the GPU: per row and matrix path

  * the lines of convnet_hip_profile_report without the time — kernel timer name, op, launches, flops, bytes, executed, as the exact
    strings the library prints (which build ran, how often, and every KernelTimer argument);
  * convnet_hip_last_kernel_info — name, grid_blocks, split_k (what note_kernel was told);
  * the SHA-256 of the output bytes (and of the bias gradient where the entry has one).  The kernels are deterministic (fixed-order
    reduces, no atomics), so another split count, K range, tail split or tile gives another digest.

tests/test_gemm_launch_trace_gpu.py compares the records with tests/golden/gemm_launch_trace.json field by field.  A refactor of the
launch layer leaves that file alone (NOTES.md, "Launch-layer refactors are checked by launch trace").

Rows (every one on both matrix paths): every conv and FC row of tests/split_cases.py with its modes and epilogue arguments; the
tail-split shape of test_hip_parity.py plain, accumulating and with bias + ReLU; AlexNet's conv2-5 (forward, input gradient, weight
gradient with bias) and fc6-8 (NT / NN / TN) at 128 and 256 images and conv1's weight gradient at 64, in the library's default modes — the
sizes the launch plans were tuned at; one row for the three-blocks-per-CU gg_kernel build; one strided input gradient with N % 4 != 0.

Also the home of the row runners tests/test_split_arithmetic_gpu.py and tests/test_gemm_exact_gpu.py share (both_paths, run_case,
one_path, the per-entry callers, which take an operand factory: Whole here, Guarded in tests/gemm_exact.py) and of
alex_geoms (tests/test_full_geometry_gpu.py).  Plain helper, no pytest:

    python tests/gemm_launch_trace.py ROW      one row's record, for a diff against another checkout
    python tests/gemm_launch_trace.py --list   the row ids
    python tests/gemm_launch_trace.py --golden the whole golden file"""
import ctypes
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from oracle import Geom  # noqa: E402
from split_cases import CASES, Case  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "gemm_launch_trace.json")
PATHS = (("split", 1), ("fp32", 0))


# ---- shared with tests/test_split_arithmetic_gpu.py -------------------------------------------------------------------------------
def both_paths(fn):
    """fn() on the bf16-split path and on the fp32-instruction path."""
    from convnet_amd import _lib
    out = {}
    try:
        for name, v in PATHS:
            _lib.lib.convnet_hip_set_matrix_path(v)
            out[name] = fn()
    finally:
        _lib.lib.convnet_hip_set_matrix_path(1)
    return out["split"], out["fp32"]


def run_case(case, fn, wrap=None):
    """fn() on both paths with the patch / wgrad-tile modes of the row; the split path's timer names.  `wrap(fn)`, when given, runs in
    fn's place on BOTH paths (the launch trace records around it) and its result is what comes back; the names are then empty."""
    from convnet_amd import _lib
    names = set()
    pm, wt = _lib.lib.convnet_hip_get_patch_mode(), _lib.lib.convnet_hip_get_wgrad_tile()

    def call():
        on_split = _lib.lib.convnet_hip_get_matrix_path() == 1
        if on_split:
            _lib.profile_report()
            _lib.profile_enable(True)
        try:
            out = fn()
        finally:
            if on_split:
                names.update(r["kernel"] for r in _lib.profile_report())
                _lib.profile_enable(False)
        return out
    try:
        if case.patch_mode >= 0:
            _lib.lib.convnet_hip_set_patch_mode(case.patch_mode)
        if case.wgrad_tile >= 0:
            _lib.lib.convnet_hip_set_wgrad_tile(case.wgrad_tile)
        s, f = both_paths(call if wrap is None else lambda: wrap(fn))
    finally:
        _lib.lib.convnet_hip_set_patch_mode(pm)
        _lib.lib.convnet_hip_set_wgrad_tile(wt)
    return s, f, names


def conv_geom(case):
    N, C, H, W, F, Ky, Kx, sy, sx, pad = case.shape
    return Geom(N=N, C=C, H=H, W=W, F=F, Ky=Ky, Kx=Kx, sy=sy, sx=sx, pady=pad, padx=pad)


class Whole:
    """The operand factory of the plain rows: every operand a device matrix of its own.  A factory's mat() turns a numpy array into the
    (rows, cols) matrix the library is handed — role "act" (activations, derivatives), "param" (banks, bank gradients) or "vec" (biases,
    bias gradients, masks), target: the call writes it — and read() brings a target back.  tests/gemm_exact.py has the factory that places
    every operand between guard floats of one flat allocation."""

    def mat(self, a, rows, cols, shape4=None, role="act", target=False):
        from hip_adapter import _mat
        return _mat(a, rows, cols, shape4)

    def read(self, m):
        return m.ToNumpy()


WHOLE = Whole()


def one_path(case, fn, path):
    """fn() on one matrix path (1 = split, 0 = fp32) with the patch / wgrad-tile modes of the row: (result, the timer names that ran)"""
    from convnet_amd import _lib
    pm, wt = _lib.lib.convnet_hip_get_patch_mode(), _lib.lib.convnet_hip_get_wgrad_tile()
    names = set()
    try:
        if case.patch_mode >= 0:
            _lib.lib.convnet_hip_set_patch_mode(case.patch_mode)
        if case.wgrad_tile >= 0:
            _lib.lib.convnet_hip_set_wgrad_tile(case.wgrad_tile)
        _lib.lib.convnet_hip_set_matrix_path(path)
        _lib.profile_report()
        _lib.profile_enable(True)
        try:
            out = fn()
        finally:
            names.update(r["kernel"] for r in _lib.profile_report())
            _lib.profile_enable(False)
    finally:
        _lib.lib.convnet_hip_set_matrix_path(1)
        _lib.lib.convnet_hip_set_patch_mode(pm)
        _lib.lib.convnet_hip_set_wgrad_tile(wt)
    return out, names


def _act(ops, a, N, W, H, C, target=False):
    return ops.mat(a, N, W * H * C, (N, W, H, C), "act", target)


def _bank(ops, g, w, target=False):
    return ops.mat(w, g.F, g.K, (g.F, g.Kx, g.Ky, g.C), "param", target)


def call_conv_fprop(case, g, x, w, t0=None, bias=None, ops=WHOLE):
    """convUp / convUpBiasAct of the row: the targets (F, My, Mx, N)"""
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc
    X, Wm = _act(ops, x, g.N, g.W, g.H, g.C), _bank(ops, g, w)
    T = _act(ops, t0 if t0 is not None else np.zeros(g.out_shape(), np.float32), g.N, g.Mx, g.My, g.F, True)
    if bias is not None:
        Matrix.ConvUpBiasAct(X, Wm, ops.mat(bias, 1, g.F, None, "vec"), T, _desc(g), case.st, bool(case.relu))
    else:
        Matrix.ConvUp(X, Wm, T, _desc(g), case.st)
    return ops.read(T).reshape(g.out_shape())


def call_conv_dgrad(case, g, dy, w, t0=None, mask=None, ops=WHOLE):
    """convDown / convDownMask of the row: the targets (C, H, W, N)"""
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc
    D, Wm = _act(ops, dy, g.N, g.Mx, g.My, g.F), _bank(ops, g, w)
    T = _act(ops, t0 if t0 is not None else np.zeros(g.in_shape(), np.float32), g.N, g.W, g.H, g.C, True)
    if mask is not None:
        S = ops.mat(mask, g.N, g.W * g.H * g.C, (g.N, g.W, g.H, g.C), "vec")
        Matrix.ConvDownMask(D, Wm, S, T, _desc(g), case.st, case.post_scale)
    else:
        Matrix.ConvDown(D, Wm, T, _desc(g), case.st)
    return ops.read(T).reshape(g.in_shape())


def call_conv_wgrad(case, g, x, dy, t0, b0, ops=WHOLE):
    """convOutpBias (dW, db) or convOutp (dW, None) of the row"""
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc
    X, D = _act(ops, x, g.N, g.W, g.H, g.C), _act(ops, dy, g.N, g.Mx, g.My, g.F)
    T = _bank(ops, g, t0, True)
    if case.entry == "convOutpBias":
        B = ops.mat(b0.reshape(1, g.F), 1, g.F, None, "vec", True)
        Matrix.ConvOutpBias(X, D, T, B, _desc(g), case.st, case.so)
        return ops.read(T).reshape(g.filt_shape()), ops.read(B).reshape(g.F)
    Matrix.ConvOutp(X, D, T, _desc(g), 0, 0, case.st, case.so)
    return ops.read(T).reshape(g.filt_shape()), None


def dot_mask(Am, Bm, mask, T, case, out_shape, ta, tb, ops=WHOLE):
    from convnet_amd._lib import lib
    am = Am.GetMatTranspose() if ta else Am.GetMat()
    bm = Bm.GetMatTranspose() if tb else Bm.GetMat()
    S = ops.mat(mask, out_shape[1], out_shape[0], None, "vec")
    rc = lib.dotMask(am, bm, S.GetMat(), T.GetMat(), float(case.st), float(case.so), float(case.post_scale))
    assert rc == 0, rc


def call_dot(case, A, B, t0, out_shape, ta, tb, bias=None, mask=None, ops=WHOLE):
    """dot / dotBiasAct / dotMask of the row on numpy (cols, rows) operands: the target in out_shape.  The weights are B on the NT and
    NN rows and the target on the TN rows (role "param"); everything else is an activation or a derivative."""
    from convnet_amd.matrix import Matrix
    tn = case.trans == "TN"
    Am, Bm = ops.mat(A, A.shape[1], A.shape[0]), ops.mat(B, B.shape[1], B.shape[0], None, "act" if tn else "param")
    T = ops.mat(t0, out_shape[1], out_shape[0], None, "param" if tn else "act", True)
    if case.entry == "dotBiasAct":
        Matrix.DotBiasAct(Am, Bm, ops.mat(bias, 1, out_shape[0], None, "vec"), T, case.st, case.so, ta, tb, bool(case.relu))
    elif case.entry == "dotMask":
        dot_mask(Am, Bm, mask, T, case, out_shape, ta, tb, ops)
    else:
        Matrix.Dot(Am, Bm, T, case.st, case.so, ta, tb)
    return ops.read(T).reshape(out_shape)


def _local_mats(ops, g, x=None, y=None, w=None, target=None):
    """the LOCAL geometry's (activations, outputs, bank) that are given, as matrices; `target` names the one the call writes"""
    out = []
    if x is not None:
        out.append(ops.mat(x, g.N, g.W * g.H * g.C, (g.N, g.W, g.H, g.C), "act", target == "x"))
    if y is not None:
        out.append(ops.mat(y, g.N, g.Mx * g.My * g.F, (g.N, g.Mx, g.My, g.F), "act", target == "y"))
    if w is not None:
        out.append(ops.mat(w, g.F, g.K * g.M, (g.F, g.Kx, g.Ky, g.C * g.M), "param", target == "w"))
    return out


def call_local_up(case, g, x, w, t0=None, bias=None, ops=WHOLE):
    """localUp / localUpBiasAct of the row (bias (F, My, Mx)): the targets (F, My, Mx, N)"""
    from convnet_amd._lib import lib
    from convnet_amd.matrix import _conv_call
    from hip_adapter import _desc
    X, T, Wm = _local_mats(ops, g, x, t0 if t0 is not None else np.zeros(g.out_shape(), np.float32), w, "y")
    if bias is not None:
        _conv_call(lib.localUpBiasAct, (X, Wm, ops.mat(bias, 1, g.F * g.M, None, "vec"), T), _desc(g), float(case.st), int(case.relu), unshaped=2)
    else:
        _conv_call(getattr(lib, case.entry), (X, Wm, T), _desc(g), float(case.st))
    return ops.read(T).reshape(g.out_shape())


def call_local_down(case, g, dy, w, t0=None, ops=WHOLE):
    from convnet_amd._lib import lib
    from convnet_amd.matrix import _conv_call
    from hip_adapter import _desc
    T, D, Wm = _local_mats(ops, g, t0 if t0 is not None else np.zeros(g.in_shape(), np.float32), dy, w, "x")
    _conv_call(getattr(lib, case.entry), (D, Wm, T), _desc(g), float(case.st))
    return ops.read(T).reshape(g.in_shape())


def call_local_outp(case, g, x, dy, t0=None, ops=WHOLE):
    from convnet_amd._lib import lib
    from convnet_amd.matrix import _conv_call
    from hip_adapter import _desc
    X, D, T = _local_mats(ops, g, x, dy, t0 if t0 is not None else np.zeros(g.bank_shape(), np.float32), "w")
    _conv_call(getattr(lib, case.entry), (X, D, T), _desc(g), float(case.st), float(case.so))
    return ops.read(T).reshape(g.bank_shape())


# ---- shared with tests/test_full_geometry_gpu.py -----------------------------------------------------------------------------------
def alex_geoms(N=256):
    """The conv geometries of the real model at N images, read off the built graph."""
    from convnet_amd import models, pbtxt
    from convnet_amd.edge import ConvEdge
    from convnet_amd.convnet import ConvNet
    net = ConvNet(pbtxt.parse(models.alexnet()))
    out = {}
    for e in net.edges_:
        if isinstance(e, ConvEdge):
            s, d = e.GetSource(), e.conv_desc_
            out[e.GetDest().GetName()] = Geom(N, s.GetNumChannels(), s.GetSizeY(), s.GetSizeX(), d.num_output_channels, d.kernel_size_y,
                                              d.kernel_size_x, d.stride_y, d.stride_x, -d.padding_y, -d.padding_x)
    return out


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
ALEX_FC = {"fc6": (9216, 4096), "fc7": (4096, 4096), "fc8": (4096, 1000)}   # (inputs, outputs) of the real model's FC edges
TAIL_SHAPE = (256, 64, 18, 18, 256, 3, 3, 1, 1, 1)    # test_hip_parity.py::test_conv_up_tail_split_more_tiles_than_slots
O3_ROW = "o3_three_blocks_per_cu"
O3_SHAPE = (256, 8, 40, 40, 128, 3, 3, 1, 1, 1)       # path 0, C % 16 != 0, F in 97..128, N % 4 == 0, 1600 tiles of 128 x 256


def _shape_of(g):
    assert g.pady == g.padx
    return (g.N, g.C, g.H, g.W, g.F, g.Ky, g.Kx, g.sy, g.sx, g.pady)


def rows():
    """[Case]: every row of the trace, in the golden file's order (expect stays empty on the rows that are not split_cases')"""
    out = [c for c in CASES if not c.entry.startswith("local")]
    out += [Case("tail_split_plain", "convUp", TAIL_SHAPE, ()), Case("tail_split_accumulate", "convUp", TAIL_SHAPE, (), st=1.0),
            Case("tail_split_bias_relu", "convUpBiasAct", TAIL_SHAPE, (), relu=1)]
    for N in (128, 256):
        geoms = alex_geoms(N)
        for layer in ("conv2", "conv3", "conv4", "conv5"):
            shape = _shape_of(geoms[f"hidden{layer[-1]}_conv"])
            out += [Case(f"alex_{layer}_fprop_n{N}", "convUp", shape, ()), Case(f"alex_{layer}_dgrad_n{N}", "convDown", shape, ()),
                    Case(f"alex_{layer}_wgrad_n{N}", "convOutpBias", shape, ())]
        for fc, (D, F) in ALEX_FC.items():
            out += [Case(f"alex_{fc}_{t.lower()}_n{N}", "dot", (N, D, F), (), trans=t) for t in ("NT", "NN", "TN")]
    out.append(Case("alex_conv1_wgrad_n64", "convOutpBias", _shape_of(alex_geoms(64)["hidden1_conv"]), ()))
    out.append(Case(O3_ROW, "convUp", O3_SHAPE, ()))
    out.append(Case("dgrad_classes_scalar_n30", "convDown", (30, 128, 13, 13, 64, 3, 3, 2, 2, 1), (),
                    note="N % 4 != 0: the scalar-load builds through gg_run_classes, dgrad_filter_kernel per class"))
    assert len({c.id for c in out}) == len(out)
    return out


def _normal(rng, shape):
    return rng.standard_normal(shape, dtype=np.float32)


def _runner(case):
    """fn() -> (output, bias gradient or None) on inputs seeded from the row id: standard normals, a non-zero prior target where the row
    accumulates, a 0 / positive state tensor for the mask entries"""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    if case.entry.startswith("dot"):
        N, D, F = case.shape
        if case.trans == "NT":
            A, B, out_shape, ta, tb = _normal(rng, (D, N)), _normal(rng, (D, F)), (F, N), False, True
        elif case.trans == "NN":
            A, B, out_shape, ta, tb = _normal(rng, (F, N)), _normal(rng, (D, F)), (D, N), False, False
        else:
            A, B, out_shape, ta, tb = _normal(rng, (F, N)), _normal(rng, (D, N)), (D, F), True, False
        t0 = _normal(rng, out_shape) if case.st else np.zeros(out_shape, np.float32)
        bias = _normal(rng, (out_shape[0],)) if case.entry == "dotBiasAct" else None
        mask = np.maximum(_normal(rng, out_shape), 0) if case.entry == "dotMask" else None
        return lambda: (call_dot(case, A, B, t0, out_shape, ta, tb, bias, mask), None)
    g = conv_geom(case)
    if case.op == "fprop":
        x, w = _normal(rng, g.in_shape()), _normal(rng, g.filt_shape())
        t0 = _normal(rng, g.out_shape()) if case.st else None
        bias = _normal(rng, (g.F,)) if case.entry == "convUpBiasAct" else None
        return lambda: (call_conv_fprop(case, g, x, w, t0, bias), None)
    if case.op == "dgrad":
        dy, w = _normal(rng, g.out_shape()), _normal(rng, g.filt_shape())
        t0 = _normal(rng, g.in_shape()) if case.st else None
        mask = np.maximum(_normal(rng, g.in_shape()), 0) if case.entry == "convDownMask" else None
        return lambda: (call_conv_dgrad(case, g, dy, w, t0, mask), None)
    x, dy = _normal(rng, g.in_shape()), _normal(rng, g.out_shape())
    t0 = _normal(rng, g.filt_shape()) if case.st else np.zeros(g.filt_shape(), np.float32)
    b0 = _normal(rng, (g.F,)) if case.st else np.zeros((g.F,), np.float32)
    return lambda: call_conv_wgrad(case, g, x, dy, t0, b0)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def _recorded(fn):
    """fn() with the profile on: {profile, kernel, out[, bias]}"""
    from convnet_amd import _lib
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.lib.convnet_hip_profile_report(buf, len(buf))   # forget what ran before
    _lib.profile_enable(True)
    try:
        out, db = fn()
        n = _lib.lib.convnet_hip_profile_report(buf, len(buf))
    finally:
        _lib.profile_enable(False)
    lines = []
    for line in buf.value.decode().splitlines() if n else []:
        k, op, cnt, _ms, fl, by, ex = line.split("|")
        lines.append("|".join((k, op, cnt, fl, by, ex)))
    from hip_adapter import last_kernel
    rec = {"profile": lines, "kernel": list(last_kernel()[:3]), "out": _sha(out)}
    if db is not None:
        rec["bias"] = _sha(db)
    return rec


def record(case):
    """{"split": {...}, "fp32": {...}}: the row on both matrix paths"""
    s, f, _ = run_case(case, _runner(case), wrap=_recorded)
    return {"split": s, "fp32": f}


def setup_device():
    import torch
    assert torch.cuda.is_available(), "the launch trace needs a GPU"
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)


def first_difference(got, want):
    """(path, field, got, want) of the first field of a row's record that differs from the golden's, or None"""
    for path, _ in PATHS:
        for field in ("kernel", "profile", "out", "bias"):
            a, b = got[path].get(field), want.get(path, {}).get(field)
            if a != b:
                return path, field, a, b
    return None


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--list" in args:
        print("\n".join(c.id for c in rows()))
    else:
        setup_device()
        if "--golden" in args:
            print(json.dumps({c.id: record(c) for c in rows()}, indent=0))
        else:
            print(json.dumps(record({c.id: c for c in rows()}[args[0]]), indent=1))
