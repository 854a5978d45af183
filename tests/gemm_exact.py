"""Exact rows for every GEMM kernel build: the data, the float64 reference and the guarded operand views tests/test_gemm_exact_gpu.py
runs the rows of tests/split_cases.py on, and tests/test_gemm_exact_cpu.py checks without a GPU.  Plain helper, no pytest.

With small-integer operands and dyadic epilogue factors every product and every partial sum of a row is a multiple of a value grid u
and below 2^24 u, hence exactly representable in fp32 in ANY summation order, on the fp32 instruction and on the bf16-split path alike
(whose h and m planes then carry the operand exactly and whose l plane is zero).  A correct kernel of any tiling reproduces the float64
reference bit for bit over the whole tensor.

Operand families (FAMILIES), from a generator seeded by row and family:
  h     both GEMM operands integers in [-r, r];
  a_hm  the first operand a 2^8 + b with integers a, b in [-r, r] (its bf16 split has non-zero h and m planes and l = 0), the second
        operand integers in [-r, r];
  b_hm  the same with the roles swapped.
The first / second operand are (activations, bank) on the forward rows, (derivatives, bank) on the input-gradient rows and
(activations, derivatives) on the weight-gradient rows; on the FC rows (in, W), (dout, W), (dout, in).

r is 4 and is narrowed per row to 2 or 1 by the worst case of the exactness condition (radius()): the *_hm families of
wgrad_reduce_two_level (46 656 terms per output) run at r = 1 and those of wgrad_bias_fallback (scaleOutput 2) at r = 2; every h
family runs at r = 4.  No row has to give up a *_hm family for its reduction length;
the rows whose reference exceeds 10^10 multiply-adds (H_ONLY: dgrad_mask_tail, fwd_gpw_tail) run h only.

Epilogue operands: prior targets and prior bias gradients are multiples of 4 (a target the call overwrites, scaleTargets == 0, holds
STALE instead, which the reference ignores); biases are integers; masks are integers in [-2, 2] of which only the sign counts.

The exactness condition is asserted, not measured: for every output (|st t0| + |so| sum|a_k b_k| + |bias|) / u < 2^24, the magnitude
sum computed by the same reference on the operands' absolute values (Row.condition)."""
import os
import sys
import zlib
from dataclasses import dataclass
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import local_ref as L  # noqa: E402
from local_ref import LocalGeom  # noqa: E402
from oracle import Geom  # noqa: E402
from split_cases import CASES  # noqa: E402

FAMILIES = ("h", "a_hm", "b_hm")
LIMIT = 2.0 ** 24
MAX_MACS = 1e10
STALE = 5.0                    # what a target holds before a call that overwrites it
T0_MAX, BIAS_MAX = 16, 8       # prior targets: multiples of 4 in [-16, 16]; biases: integers in [-8, 8]
TARGET_GUARD, TAIL = 7.0, 37   # guard value of the targets (the sources' is NaN); guard floats behind every operand
# leads (floats) per operand role (gemm_launch_trace.Whole) of the `aligned` layout: 16-byte bases that are not 32-byte ones
ALIGNED = {"act": 36, "param": 20, "vec": 12}
# ... and of `params_unaligned`: banks, bank gradients, biases, bias gradients and masks 4-byte aligned only, then 8-byte aligned; then
# what an edge's slices of the package's flat buffers look like: an aligned bank with only the bias, bias gradient and mask off by a float
UNALIGNED = (dict(ALIGNED, param=1, vec=1), dict(ALIGNED, param=2, vec=2), dict(ALIGNED, vec=1))


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def geom(case):
    N, C, H, W, F, Ky, Kx, sy, sx, pad = case.shape
    cls = LocalGeom if case.entry.startswith("local") else Geom
    return cls(N=N, C=C, H=H, W=W, F=F, Ky=Ky, Kx=Kx, sy=sy, sx=sx, pady=pad, padx=pad)


def reduction_length(case):
    """the largest number of products one output of the row sums (its bias gradient included)"""
    if case.entry.startswith("dot"):
        N, D, F = case.shape
        return {"NT": D, "NN": F, "TN": N}[case.trans]
    g = geom(case)
    if case.op in ("fprop", "local_up"):
        return g.K
    if case.op in ("dgrad", "local_down"):
        return g.F * -(-g.Ky // g.sy) * -(-g.Kx // g.sx)
    return g.N if case.op == "local_outp" else g.N * g.My * g.Mx


def macs(case):
    if case.entry.startswith("dot"):
        N, D, F = case.shape
        return N * D * F
    g = geom(case)
    return g.N * g.F * g.K * g.My * g.Mx


H_ONLY = tuple(c.id for c in CASES if macs(c) > MAX_MACS)


def families(case):
    """the families the row runs: all three, h alone where the float64 reference would cost more than MAX_MACS multiply-adds or where
    no radius satisfies the condition for a *_hm family (no row of split_cases.py today)"""
    return tuple(f for f in FAMILIES if f == "h" or (case.id not in H_ONLY and radius(case, f)))


def grid(case):
    """u: the power of two every term of an output is a multiple of (operands integers, prior targets multiples of 4)"""
    so, st = Fraction(abs(case.so)), Fraction(case.st)
    assert so.numerator == 1 or so.denominator == 1, (case.id, "scaleOutput is no power of two")
    return float(min(Fraction(1), so, Fraction(4, st.denominator)))   # st = p / 2^q, p odd: st * 4 j is a multiple of 4 / 2^q


def radius(case, family):
    """the largest r of (4, 2, 1) whose worst case meets the condition on every output of the row, or 0"""
    k = reduction_length(case)
    for r in (4, 2, 1):
        big = (256 * r + r) if family != "h" else r
        worst = abs(case.st) * T0_MAX + abs(case.so) * k * big * r + BIAS_MAX
        if worst / grid(case) < LIMIT:
            return r
    return 0


# ---- the bf16 split, restated (gather_gemm.h: split8) -------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split3(x):
    """(h, m, l): round to bf16, subtract, repeat"""
    x = np.asarray(x, np.float32)
    h = bf16_rne(x)
    m = bf16_rne(x - h)
    return h, m, bf16_rne(x - h - m)


# ---- float64 references ---------------------------------------------------------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def conv_fprop64(g, x, w):
    """x (C, H, W, N), w (C, Ky, Kx, F) -> (F, My, Mx, N)"""
    import torch.nn.functional as Fn
    y = Fn.conv2d(_t(x).permute(3, 0, 1, 2), _t(w).permute(3, 0, 1, 2), stride=(g.sy, g.sx), padding=(g.pady, g.padx))
    return y.permute(1, 2, 3, 0).contiguous().numpy()


def conv_dgrad64(g, dy, w):
    """dy (F, My, Mx, N), w (C, Ky, Kx, F) -> (C, H, W, N)"""
    import torch.nn.functional as Fn
    opy, opx = g.H - ((g.My - 1) * g.sy - 2 * g.pady + g.Ky), g.W - ((g.Mx - 1) * g.sx - 2 * g.padx + g.Kx)
    dx = Fn.conv_transpose2d(_t(dy).permute(3, 0, 1, 2), _t(w).permute(3, 0, 1, 2), stride=(g.sy, g.sx), padding=(g.pady, g.padx),
                             output_padding=(opy, opx))
    return dx.permute(1, 2, 3, 0).contiguous().numpy()


def conv_wgrad64(g, x, dy):
    """x (C, H, W, N), dy (F, My, Mx, N) -> (C, Ky, Kx, F): unfold, one matmul per image, summed"""
    import torch.nn.functional as Fn
    U = Fn.unfold(_t(x).permute(3, 0, 1, 2), (g.Ky, g.Kx), padding=(g.pady, g.padx), stride=(g.sy, g.sx))   # (N, K, M)
    D = _t(dy).reshape(g.F, g.My * g.Mx, g.N).permute(2, 1, 0)                                              # (N, M, F)
    return (U @ D).sum(0).reshape(g.filt_shape()).numpy()


def product64(case, g, a, b):
    """the row's GEMM on float64 copies of its two operands: the accumulator of every output, before the epilogue"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if case.op == "fprop":
        return conv_fprop64(g, a, b)
    if case.op == "dgrad":
        return conv_dgrad64(g, a, b)
    if case.op == "wgrad":
        return conv_wgrad64(g, a, b)
    if case.op == "local_up":
        return L.torch_up(g, a, b)
    if case.op == "local_down":
        return L.torch_down(g, a, b)
    if case.op == "local_outp":
        return L.torch_outp(g, a, b)
    if case.op == "fc_nt":                      # a in (D, N), b W (D, F): out (F, N)
        return b.T @ a
    if case.op == "fc_nn":                      # a dout (F, N), b W (D, F): din (D, N)
        return b @ a
    return (a @ b.T).T                          # a dout (F, N), b in (D, N): dW (D, F)


def epilogue64(case, acc, t0=None, bias=None, mask=None):
    """st t0 + so acc + bias, then ReLU, then the mask with post_scale (test_split_arithmetic_gpu.py: _epilogue_err)"""
    exact = case.so * acc
    if case.st:
        exact = exact + case.st * np.asarray(t0, np.float64)
    if bias is not None:
        exact = exact + np.asarray(bias, np.float64)
    if case.relu:
        exact = np.maximum(exact, 0.0)
    if mask is not None:
        exact = np.where(mask > 0, case.post_scale * exact, 0.0)
    return exact


# ---- one row's data and expected bits -----------------------------------------------------------------------------------------------
def _shapes(case, g):
    """(first operand, second operand, output, bias or None, has a bias gradient) as numpy shapes; bias broadcasts against the output"""
    if case.entry.startswith("dot"):
        N, D, F = case.shape
        a, b, out = {"NT": ((D, N), (D, F), (F, N)), "NN": ((F, N), (D, F), (D, N)), "TN": ((F, N), (D, N), (D, F))}[case.trans]
        return a, b, out, ((out[0], 1) if case.entry == "dotBiasAct" else None), False
    if case.op in ("fprop", "local_up"):
        w = g.filt_shape() if case.op == "fprop" else g.bank_shape()
        bias = {"convUpBiasAct": (g.F, 1, 1, 1), "localUpBiasAct": (g.F, g.My, g.Mx, 1)}.get(case.entry)
        return g.in_shape(), w, g.out_shape(), bias, False
    if case.op in ("dgrad", "local_down"):
        return g.out_shape(), (g.filt_shape() if case.op == "dgrad" else g.bank_shape()), g.in_shape(), None, False
    return g.in_shape(), g.out_shape(), (g.filt_shape() if case.op == "wgrad" else g.bank_shape()), None, case.entry == "convOutpBias"


def _ints(rng, shape, r, step=1):
    return (rng.integers(-r, r + 1, shape) * step).astype(np.float32)


@dataclass
class Row:
    case: object
    family: str
    g: object
    a: np.ndarray
    b: np.ndarray
    t0: np.ndarray            # the prior target: multiples of 4, or STALE where the call overwrites it
    bias: np.ndarray = None   # shaped to broadcast against the output
    mask: np.ndarray = None
    b0: np.ndarray = None     # the prior bias gradient (F,) of convOutpBias
    want: np.ndarray = None   # float32, the whole target
    want_db: np.ndarray = None
    condition: float = 0.0    # max over outputs of (|st t0| + |so| sum|ab| + |bias|) / u, asserted < 2^24


def operands(case, family):
    """the row's operands without its reference (cheap): a Row with want unset"""
    assert family in families(case), (case.id, family)
    rng = np.random.default_rng([zlib.crc32(case.id.encode()), FAMILIES.index(family)])
    g = None if case.entry.startswith("dot") else geom(case)
    sa, sb, so, sbias, with_db = _shapes(case, g)
    r = radius(case, family)
    a, b = _ints(rng, sa, r), _ints(rng, sb, r)
    if family == "a_hm":
        a = _ints(rng, sa, r, 256) + a
    elif family == "b_hm":
        b = _ints(rng, sb, r, 256) + b
    t0 = _ints(rng, so, T0_MAX // 4, 4) if case.st else np.full(so, STALE, np.float32)
    row = Row(case, family, g, a, b, t0)
    if sbias is not None:
        row.bias = _ints(rng, sbias, BIAS_MAX)
    if case.entry in ("convDownMask", "dotMask"):
        row.mask = _ints(rng, so, 2)
    if with_db:
        row.b0 = _ints(rng, (so[-1],), T0_MAX // 4, 4) if case.st else np.full((so[-1],), STALE, np.float32)
    return row


def _checked(case, exact, den):
    """the float32 bits of an exact float64 result, with the exactness condition asserted on its magnitude bound"""
    worst = float(den.max()) / grid(case)
    assert worst < LIMIT, (case.id, "a partial sum could round", worst)
    out = exact.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), exact), (case.id, "the reference is not an fp32 value")
    return out, worst


def reference(row):
    """fill want / want_db / condition of the row from the float64 reference (also run on the operands' absolute values)"""
    case, g = row.case, row.g
    acc, mag = product64(case, g, row.a, row.b), product64(case, g, np.abs(row.a), np.abs(row.b))
    den = abs(case.so) * mag + (abs(case.st) * np.abs(row.t0) if case.st else 0.0) + (np.abs(row.bias) if row.bias is not None else 0.0)
    row.want, row.condition = _checked(case, epilogue64(case, acc, row.t0, row.bias, row.mask), den)
    if row.b0 is not None:
        d = np.asarray(row.b, np.float64).reshape(g.F, -1)
        bden = abs(case.so) * np.abs(d).sum(1) + (abs(case.st) * np.abs(row.b0) if case.st else 0.0)
        row.want_db, worst = _checked(case, case.so * d.sum(1) + (case.st * row.b0.astype(np.float64) if case.st else 0.0), bden)
        row.condition = max(row.condition, worst)
    return row


_CACHE = {}


def row(case, family):
    """the row with its reference, computed once per (row, family); the last two are kept (the tests run row by row)"""
    key = (case.id, family)
    if key not in _CACHE:
        while len(_CACHE) >= 2:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = reference(operands(case, family))
    return _CACHE[key]


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------
def guarded(a, lead, tail, fill):
    """the flat allocation of one operand: lead floats of `fill`, the tensor, tail floats of `fill`"""
    a = np.asarray(a, np.float32).reshape(-1)
    return np.concatenate([np.full(lead, fill, np.float32), a, np.full(tail, fill, np.float32)])


def damaged(buf, lead, n, fill):
    """the offsets (relative to the tensor's first float) of the guard floats of `buf` that no longer hold `fill`"""
    buf = np.asarray(buf, np.float32).reshape(-1)
    idx = np.concatenate([np.arange(lead), np.arange(lead + n, buf.size)])
    g = buf[idx]
    bad = ~np.isnan(g) if np.isnan(fill) else g.view(np.uint32) != np.float32(fill).view(np.uint32)
    return (idx[bad] - lead).tolist()


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def first_mismatch(got, want):
    """None when the two tensors are bit-equal, else (count, index, got, want) of the first differing element"""
    bad = np.flatnonzero(bits(got) != bits(want))
    if bad.size == 0:
        return None
    i = np.unravel_index(int(bad[0]), np.shape(want))
    return int(bad.size), tuple(int(j) for j in i), float(np.asarray(got).reshape(-1)[bad[0]]), float(np.asarray(want).reshape(-1)[bad[0]])


class Guarded:
    """The operand factory of the exact rows (gemm_launch_trace.Whole is the plain one): every operand is a GetSlice view of a flat
    allocation, `leads[role]` floats in front and TAIL behind, then Reshape / SetShape4D.  Targets sit between guards of 7.0 that
    read() requires intact; sources sit between NaN, so a kernel that feeds an out-of-tensor read into its products poisons the
    output.  sources_intact() says whether any source, or a NaN guard, was written."""

    def __init__(self, leads):
        self.leads, self.held = leads, []

    def mat(self, a, rows, cols, shape4=None, role="act", target=False):
        from convnet_amd.matrix import Matrix
        a = np.asarray(a, np.float32).reshape(-1)
        assert a.size == rows * cols, (a.size, rows, cols)
        lead, fill = self.leads[role], TARGET_GUARD if target else np.nan
        full, m = Matrix(), Matrix()
        full.AllocateGPUMemory(1, lead + a.size + TAIL)
        full.FromNumpy(guarded(a, lead, TAIL, fill))
        full.GetSlice(m, lead, lead + a.size)
        m.Reshape(rows, cols)
        if shape4:
            m.SetShape4D(*shape4)
        self.held.append((m, full, lead, a, fill, target))
        return m

    def read(self, m):
        _, full, lead, a, fill, _ = next(h for h in self.held if h[0] is m)
        buf = full.ToNumpy().reshape(-1)
        bad = damaged(buf, lead, a.size, fill)
        assert not bad, ("guard floats overwritten at offsets", bad[:8], "of a target of", a.size, "floats")
        return buf[lead:lead + a.size].copy()

    def sources_intact(self):
        for _, full, lead, a, fill, target in self.held:
            if not target:
                buf = full.ToNumpy().reshape(-1)
                if damaged(buf, lead, a.size, fill) or not np.array_equal(bits(buf[lead:lead + a.size]), bits(a)):
                    return False
        return True


# ---- running a row (GPU) --------------------------------------------------------------------------------------------------------------
def run(row, ops, path):
    """the row through its ABI entry on operands from `ops`, on one matrix path: (target, bias gradient or None, timer names)"""
    import gemm_launch_trace as T
    case, g = row.case, row.g
    t0 = row.t0
    bias = None if row.bias is None else row.bias.reshape(-1)

    def fn():
        if case.op == "fprop":
            return T.call_conv_fprop(case, g, row.a, row.b, t0, bias, ops), None
        if case.op == "dgrad":
            return T.call_conv_dgrad(case, g, row.a, row.b, t0, row.mask, ops), None
        if case.op == "wgrad":
            return T.call_conv_wgrad(case, g, row.a, row.b, t0, row.b0 if row.b0 is not None else np.zeros(g.F, np.float32), ops)
        if case.op == "local_up":
            return T.call_local_up(case, g, row.a, row.b, t0, bias, ops), None
        if case.op == "local_down":
            return T.call_local_down(case, g, row.a, row.b, t0, ops), None
        if case.op == "local_outp":
            return T.call_local_outp(case, g, row.a, row.b, t0, ops), None
        ta, tb = {"NT": (False, True), "NN": (False, False), "TN": (True, False)}[case.trans]
        return T.call_dot(case, row.a, row.b, t0, row.want.shape, ta, tb, bias, row.mask, ops), None
    (out, db), names = T.one_path(case, fn, path)
    return out, db, names


VIEWS = os.path.join(os.path.dirname(HERE), "profiles", "gemm_exact_views.txt")


def views_table():
    """the builds every row runs on the layouts of UNALIGNED, on both matrix paths: the lines of profiles/gemm_exact_views.txt"""
    lines = ["# The kernel timer names every row of tests/split_cases.py runs (h family) when its parameter operands are views that are not",
             "# 16-byte aligned (tests/test_gemm_exact_gpu.py, layout params_unaligned; activations and derivatives stay 16-byte aligned).",
             "# row | matrix path | lead in floats of banks and bank gradients / of biases, bias gradients and masks | timer names",
             "# `=` marks a split-path line that ran every build the row pins on whole matrices (Case.expect)."]
    for case in CASES:
        r = row(case, "h")
        for path in (1, 0):
            for leads in UNALIGNED:
                names = sorted(run(r, Guarded(leads), path)[2])
                same = all(n in names for n in case.expect) if path == 1 else None
                lines.append(f"{case.id} | {'split' if path else 'fp32'} | {leads['param']} / {leads['vec']} | {' + '.join(names)}" + (" | =" if same else ""))
    return lines


if __name__ == "__main__":
    from gemm_launch_trace import setup_device
    setup_device()
    text = "\n".join(views_table()) + "\n"
    with open(sys.argv[1] if len(sys.argv) > 1 else VIEWS, "w") as f:
        f.write(text)
    print(text, end="")
