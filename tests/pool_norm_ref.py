"""float64 reference, error bounds, data and case lists of the 2-D pooling and cross-map response-norm entries
(include/convnet_hip.h; convnet_amd/csrc/pool_norm.hip), shared by tests/test_pool_norm_ref_cpu.py and tests/test_pool_norm_gpu.py.

The operations themselves are tests/conv3d_ref.py's, called with one frame: they clip boxes, route every tie, divide by the clipped box
and take any rectangular geometry.  Added here, from the header's definitions: the forward scales, MaxPoolUndoRelu, the per-element
error scales and bounds of the averages and of the response norm, and `expected_path` / `launched`.  2-D arrays are (C, H, W, N)."""
import collections
import functools

import numpy as np

import conv3d_ref as R3
from conv3d_ref import Geom3D

U = 2.0 ** -24          # half an ulp of 1.0f: the relative error of one correctly rounded float32 operation
PARAMS = [(0.005, 0.75), (0.001, 0.5), (0.02, 1.0)]          # (addScale, powScale)
SCALES = [(0.0, 1.0), (1.0, 1.0), (-2.0, 0.5), (0.5, -2.0)]  # (scaleTargets, scaleOutput) of the forward calls
UNDO_SCALES = [0.0, 1.0, -2.0]


def geom(N, C, H, W, Ky, Kx=None, sy=1, sx=None, pady=0, padx=None):
    Kx, sx, padx = Ky if Kx is None else Kx, sy if sx is None else sx, pady if padx is None else padx
    return Geom3D(N=N, C=C, H=H, W=W, T=1, F=C, Ky=Ky, Kx=Kx, sy=sy, sx=sx, pady=pady, padx=padx)


def shape_in(g):
    return (g.C, g.H, g.W, g.N)


def shape_out(g):
    return (g.C, g.My, g.Mx, g.N)


def _f(a):
    return np.asarray(a, np.float64)[None]


# ---- pooling ------------------------------------------------------------------------------------------------------------------------------
def max_fwd(g, x, t0=0.0, st=0.0, so=1.0):
    """MaxPoolGemm: targets = scaleTargets * targets + scaleOutput * max over the clipped window"""
    return st * np.asarray(t0, np.float64) + so * R3.max_pool(g, _f(x))[0]


def box_sizes(g):
    """n (My, Mx): the clipped window's size;  m (H, W): how many windows cover an input pixel"""
    n, m = np.zeros((g.My, g.Mx)), np.zeros((g.H, g.W))
    for (_, my, mx), b in R3.boxes(g):
        n[my, mx] = (b[2].stop - b[2].start) * (b[3].stop - b[3].start)
        m[b[2], b[3]] += 1
    return n, m


def avg_fwd(g, x, t0=0.0, st=0.0, so=1.0):
    """AvgPoolGemm -> (exact, bound).  n - 1 roundings of the sum, one each for the division, the product with scaleOutput and the
    accumulate: (n + 3) * 2^-24 * (|so| * sum|x| / n + |st * t0|) per element."""
    t0 = np.asarray(t0, np.float64)
    n = box_sizes(g)[0][None, :, :, None]
    exact = st * t0 + so * R3.avg_pool(g, _f(x))[0]
    return exact, (n + 3) * U * (abs(so) * R3.avg_pool(g, np.abs(_f(x)))[0] + np.abs(st * t0))


def max_undo(g, x, dy, y, t0=0.0, st=0.0, relu=False):
    """MaxPoolUndoGemm; relu: MaxPoolUndoRelu = (x > 0) ? scaleTargets * targets + undo : 0 (the accumulated target is masked too)"""
    out = st * np.asarray(t0, np.float64) + R3.max_pool_undo(g, _f(x), _f(dy), _f(y))[0]
    return np.where(np.asarray(x) > 0, out, 0.0) if relu else out


def avg_undo(g, dy, t0=0.0, st=0.0):
    """AvgPoolUndoGemm -> (exact, bound, covered).  Each of the m covering windows gives dy / size with two roundings (the reciprocal,
    the product), m - 1 for their sum, two for the accumulate: (m + 4) * 2^-24 * (sum |dy| / size + |st * t0|).  Where no window
    covers a pixel (covered == False) the formula leaves 4 * 2^-24 * |st * t0|, which is looser than what holds there: the result is
    exactly the float32 product st * t0, and both test files compare those pixels with np.array_equal as well."""
    t0 = np.asarray(t0, np.float64)
    m = box_sizes(g)[1][None, :, :, None]
    exact = st * t0 + R3.avg_pool_undo(g, _f(dy))[0]
    bound = (m + 4) * U * (R3.avg_pool_undo(g, np.abs(_f(dy)))[0] + np.abs(st * t0))
    return exact, bound, np.broadcast_to(m > 0, exact.shape)


# ---- response norm ------------------------------------------------------------------------------------------------------------------------
def rnorm_fwd(x, size_f, a, b, blocked=False):
    """-> (exact, s): s_j = |x_j| * D_j^-b, the error scale: the result's own magnitude"""
    exact = R3.rnorm(_f(x), size_f, a, b, blocked)[0]
    return exact, np.abs(exact)


def rnorm_undo(dy, x, size_f, a, b, blocked=False):
    """-> (exact, s): s_j = |dy_j| * D_j^-b + 2ab * |x_j| * sum_i |dy_i * x_i| * D_i^(-b-1): the two terms with every product's sign
    dropped, so cancellation between them (and inside the window sum) does not shrink the scale"""
    dy, x = _f(dy), _f(x)
    M = R3.rnorm_windows(x.shape[1], size_f, blocked)
    D = 1 + a * np.einsum("ji,ti...->tj...", M, x * x)
    s = np.abs(dy) * D ** -b + 2 * a * b * np.abs(x) * np.einsum("ij,ti...->tj...", M, np.abs(dy * x) * D ** (-b - 1))
    return R3.rnorm_undo(dy, x, size_f, a, b, blocked)[0], s[0]


def units(got, exact, s):
    """largest |got - exact| in units of 2^-24 * s; where s == 0 the result must be exactly 0 (inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64) - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(s > 0, err / (U * s), np.where(err == 0, 0.0, np.inf))
    return float(u.max())


def rnorm_allowed(e_case):
    """4 * (the fp32 oracle's own error on the same arrays) + 34: see the GPU file's docstring"""
    return 4.0 * e_case + 34.0


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def integers(rng, shape, lo=-4, hi=4):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def normal(rng, shape):
    return rng.standard_normal(shape).astype(np.float32)


def wide(rng, shape):
    """N(0, 1) scaled per element by 2^k, k in [-6, 6]"""
    return (rng.standard_normal(shape) * 2.0 ** rng.integers(-6, 7, shape)).astype(np.float32)


def _seed(name):
    return [71] + [ord(c) for c in name]


@functools.lru_cache(maxsize=None)
def pool_data(name):
    """the arrays of one pooling case, made once: integer x / dy / t0 (t0 on the input and on the pooled side), their N(0, 1) and wide
    counterparts.  Read-only."""
    g = POOL_GEOMS[name]
    rng = np.random.default_rng(_seed(name))
    d = {"xi": integers(rng, shape_in(g)), "dyi": integers(rng, shape_out(g)), "ti_in": integers(rng, shape_in(g)),
         "ti_out": integers(rng, shape_out(g)), "xn": normal(rng, shape_in(g)), "xw": wide(rng, shape_in(g)),
         "dyn": normal(rng, shape_out(g)), "dyw": wide(rng, shape_out(g)), "tn_in": normal(rng, shape_in(g)),
         "tn_out": normal(rng, shape_out(g)), "x5": np.full(shape_in(g), -5.0, np.float32)}
    # half of the (channel, image) maps are negative throughout (still integers in [-4, 4]): a 4 x 4 window of uniform integers has a
    # negative maximum once in 10^5 draws, and negative maxima are what the integer cases are for
    neg = rng.integers(0, 2, (g.C, 1, 1, g.N)).astype(bool)
    d["xi"] = np.where(neg, integers(rng, shape_in(g), -4, -1), d["xi"])
    d["yi"] = R3.max_pool(g, d["xi"][None])[0].astype(np.float32)        # a selection: exact in float32
    d["yn"] = R3.max_pool(g, d["xn"][None])[0].astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def rnorm_data(name):
    shape = RNORM_CASES[name][2]
    rng = np.random.default_rng(_seed(name))
    d = {"xn": normal(rng, shape), "dyn": normal(rng, shape), "xw": wide(rng, shape), "dyw": wide(rng, shape)}
    for k in ("xn", "xw"):
        d[k].reshape(-1)[::11] = 0.0          # x_j == 0 must give exactly 0 forward
    for v in d.values():
        v.setflags(write=False)
    return d


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
_GENERIC = {"k4s2_9x9": dict(C=3, H=9, W=9, Ky=4, sy=2), "k3s1_6x7_p1p2": dict(C=3, H=6, W=7, Ky=3, sy=1, pady=1, padx=2),
            "k2s3_8x8": dict(C=3, H=8, W=8, Ky=2, sy=3),          # pixels that no window covers
            "k3x2s2x1_9x7_p1p0": dict(C=3, H=9, W=7, Ky=3, Kx=2, sy=2, sx=1, pady=1, padx=0)}
POOL_GEOMS = {}
for _n, _k in _GENERIC.items():
    POOL_GEOMS[f"{_n}_N4"] = geom(N=4, **_k)
    POOL_GEOMS[f"{_n}_N6"] = geom(N=6, **_k)
POOL_GEOMS.update({
    "f32_9x13_C2": geom(4, 2, 9, 13, 3, sy=2),                          # fewer than 64 blocks: the plain 3-D grid
    "f32_11x11_p1_C13": geom(4, 13, 11, 11, 3, sy=2, pady=1),           # 78 forward blocks: 8 * 10 launched, two idle
    "f32_19x19_C4_N128": geom(128, 4, 19, 19, 3, sy=2),                 # two x-blocks forward, three on the undo side
    "f32_11x9_p1p0": geom(4, 3, 11, 9, 3, sy=2, pady=1, padx=0),        # mixed padding
    "f22_8x8": geom(4, 3, 8, 8, 2, sy=2), "f22_9x7": geom(4, 3, 9, 7, 2, sy=2), "f22_7x7_p1": geom(4, 3, 7, 7, 2, sy=2, pady=1),
    "blk_43x41_C2": geom(4, 2, 43, 41, 3, sy=2),                        # pooled 21 x 20 = 420, odd pooled rows; undo: odd H and W
    "blk_39x39_p1_C2": geom(4, 2, 39, 39, 3, sy=2, pady=1),             # pooled 20 x 20
    "blk_21x20_p1_C3": geom(4, 3, 21, 20, 3, sy=2, pady=1),             # H * W = 420, odd H: the undo block kernel only
    "blk_43x41_C7": geom(4, 7, 43, 41, 3, sy=2),                        # the block kernels in XCD order: 77 and 154 blocks (the other block maps stay below 64)
})
# (name, misaligned): every N = 4 geometry runs in both placements, the others aligned
POOL_CASES = [(n, mis) for n, g in POOL_GEOMS.items() for mis in ((False, True) if g.N == 4 else (False,))]
FIXED_CASES = [n for n, g in POOL_GEOMS.items() if n[0] in "fb" and g.N == 4]
SQUARE_CASES = [n for n, g in POOL_GEOMS.items() if g.H == g.W and g.Ky == g.Kx and g.sy == g.sx and g.pady == g.padx]

# name -> (sizeF, blocked, (C, H, W, N), misaligned)
RNORM_CASES = {
    "fast64_C100": (64, False, (100, 3, 3, 4), False), "fast64_C72": (64, False, (72, 3, 3, 4), False),
    "fast24_C90": (24, False, (90, 3, 3, 4), False), "lds_C160_w5": (5, False, (160, 2, 3, 4), False),
    "lds_C300_w24": (24, False, (300, 3, 3, 4), False), "lds_C520_w5": (5, False, (520, 3, 3, 4), False),
    "gen_C800_w64": (64, False, (800, 1, 2, 4), False), "gen_C800_w64_locs6": (64, False, (800, 1, 3, 2), False),
    "gen_C800_w7_blocked": (7, True, (800, 1, 2, 4), False),
    "mis_C96_w24": (24, False, (96, 3, 3, 4), True), "mis_C300_w24": (24, False, (300, 3, 3, 4), True),
    "w1_C32": (1, False, (32, 3, 3, 4), False), "w6_C32": (6, False, (32, 3, 3, 4), False), "w40_C32": (40, False, (32, 3, 3, 4), False),
}


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------------
# name: what the library reports for the call (convnet_hip_last_kernel_info);  grid_blocks: the blocks it launched, idle XCD-order blocks
# included, or None where the grid comes from the runtime's occupancy figure (the persistent fast kernels): then grid_cap bounds it;
# label: name + the launch form, the vocabulary of the test ids and of REQUIRED_PATHS
Path = collections.namedtuple("Path", "name grid_blocks grid_cap label")


def _divup(a, b):
    return -(-a // b)


def _grid_for(items):
    return max(1, min(4096, _divup(items, 256)))


def _rn_fast(C, size_f, blocked, vec, undo):
    """(LT, CG) of the fast kernel build that takes the call, or None"""
    if blocked or not vec or C < size_f or size_f not in (24, 64):
        return None
    CG = 8 if size_f == 64 else (12 if C <= 96 else 6)
    G, LT = _divup(C, CG), 128
    while LT > 16 and G * LT > 512:
        LT //= 2
    if LT == 128 and CG != 24:
        LT = 64
    if G * LT > 512:
        return None
    H = size_f // 2
    SS = min(CG, H)
    rows, seg = H + C + CG + H + 1, G * (CG // SS) + 2 * (H // SS)
    if 4 * LT * (2 * rows + 2 * seg if undo else rows + C + CG + seg) > 160 * 1024:
        return None
    return LT, CG


def _rn_segments(locs, C, size_f):
    quads = (locs + 3) // 4
    n = max(1, min(_divup(1 << 20, quads), max(1, C // max(size_f, 8))))
    cseg = _divup(C, n)
    return cseg, _divup(C, cseg)


def expected_path(op, g=None, aligned=True, C=0, size_f=0, blocked=False, locs=0):
    """The kernel a call takes and its grid, as a Path.  This RESTATES the dispatch of convnet_amd/csrc/pool_norm.hip by hand; the GPU
    tests hold it against what the library reports after each call (launched), so a moved threshold fails them, and one assertion
    checks that the case lists reach every label in REQUIRED_PATHS.  op: max_fwd, avg_fwd, max_undo, avg_undo (g, aligned), mask_fwd,
    mask_undo (g: the mask pair, tests/test_pool_mask_gpu.py) or
    rnorm_fwd, rnorm_undo (C, size_f, blocked, locs, aligned)."""
    if op.startswith("rnorm"):
        vec = locs % 4 == 0 and aligned
        arm, undo = "vec" if vec else "scalar", op == "rnorm_undo"
        LT = (64 if C <= 64 else 16 if C <= 256 else 8 if C <= 512 else 0) if undo else (64 if C <= 192 else 32 if C <= 384 else 16 if C <= 768 else 0)
        fast = _rn_fast(C, size_f, blocked, vec, undo) if LT or not undo else None
        way = "undo" if undo else "fwd"
        if fast:
            name = f"rnorm_{way}_fast_kernel<{fast[0]}, {fast[1]}, {size_f}>"
            return Path(name, None, 8 * _divup(_divup(locs, fast[0]), 8), name)
        if LT:
            name = f"rnorm_undo_lds_kernel<{LT}>/{512 if C > 128 else 256}/{arm}" if undo else f"rnorm_fwd_lds_kernel<{LT}>/{arm}"
            return Path(name, 8 * _divup(_divup(locs, LT), 8), None, name)
        cseg, nseg = _rn_segments(locs, C, size_f)
        grid = _grid_for((locs + 3) // 4 * nseg)
        if undo:
            name = f"rnorm_undo1_kernel+rnorm_undo2_kernel/{arm}"
            return Path(name, grid, None, name)
        name = f"rnorm_fwd_kernel/{arm}"
        return Path(name, grid, None, f"{name}/{'segments' if nseg > 1 else 'one segment'}")
    kind, way = op.split("_")
    if kind == "mask":      # MaxPoolMask / MaxPoolUndoMask: block kernels only, at every map size (refused unless 3 x 3 stride 2 on float4 rows)
        rows, cols = (g.My, g.Mx) if way == "fwd" else (g.H, g.W)
        total = _divup(((cols + 1) // 2) * _divup(g.N, 4), 256) * ((rows + 1) // 2) * g.C
        xcd = 64 <= total <= 1 << 30
        return Path(f"pool_{way}_max32_mask_kernel", 8 * _divup(total, 8) if xcd else total, None, f"pool_{way}_max32_mask_kernel/{'xcd' if xcd else 'grid3d'}")
    vec = g.N % 4 == 0 and aligned
    fixed = vec and g.Ky == g.Kx and g.sy == g.sx and (g.Ky, g.sy) in ((3, 2), (2, 2))
    nvec = _divup(g.N, 4)
    rows, cols = (g.My, g.Mx) if way == "fwd" else (g.H, g.W)
    if not fixed:
        name = f"pool_{way}_kernel<{kind}>/{'vec' if vec else 'scalar'}"
        return Path(name, _grid_for(g.C * rows * cols * nvec), None, name)
    if g.Ky == 3 and kind == "max" and rows * cols >= 400:
        name, xb, rows = f"pool_{way}_max32_block_kernel", _divup(((cols + 1) // 2) * nvec, 256), (rows + 1) // 2
    else:
        name, xb = f"pool_{way}_fixed_kernel<{kind}, {g.Ky}, {g.sy}>", _divup(cols * nvec, 256)
    total = xb * rows * g.C
    xcd = 64 <= total <= 1 << 30
    return Path(name, 8 * _divup(total, 8) if xcd else total, None, f"{name}/{'xcd' if xcd else 'grid3d'}" + (f"/{xb} x-blocks" if xb > 1 else ""))


def launched(path, name, grid_blocks, split_k=1, flops=0.0):
    """asserts that what the library reported for its last call (convnet_hip_last_kernel_info) is `path`"""
    assert (name, split_k, flops) == (path.name, 1, 0.0), ((name, split_k, flops), path)
    if path.grid_blocks is not None:
        assert grid_blocks == path.grid_blocks, (name, grid_blocks, path)
    else:
        assert grid_blocks > 0 and grid_blocks % 8 == 0 and grid_blocks <= path.grid_cap, (name, grid_blocks, path)


def pool_path(name, mis, op):
    return expected_path(op, POOL_GEOMS[name], not mis)


def rnorm_path(name, op):
    size_f, blocked, shape, mis = RNORM_CASES[name]
    return expected_path(op, C=shape[0], size_f=size_f, blocked=blocked, locs=int(np.prod(shape[1:])), aligned=not mis)


def pool_paths(name, mis):
    return {op: pool_path(name, mis, op).label for op in ("max_fwd", "avg_fwd", "max_undo", "avg_undo")}


def rnorm_paths(name):
    return {op: rnorm_path(name, op).label for op in ("rnorm_fwd", "rnorm_undo")}


REQUIRED_PATHS = (
    [f"pool_{w}_kernel<{k}>/{a}" for w in ("fwd", "undo") for k in ("max", "avg") for a in ("vec", "scalar")]
    + [f"pool_{w}_fixed_kernel<{k}, 3, 2>/{o}" for w in ("fwd", "undo") for k in ("max", "avg") for o in ("grid3d", "xcd")]
    + [f"pool_fwd_fixed_kernel<{k}, 3, 2>/xcd/2 x-blocks" for k in ("max", "avg")]
    + [f"pool_{w}_fixed_kernel<{k}, 2, 2>/grid3d" for w in ("fwd", "undo") for k in ("max", "avg")]
    + [f"pool_{w}_max32_block_kernel/{o}" for w in ("fwd", "undo") for o in ("grid3d", "xcd")]
    + ["rnorm_fwd_fast_kernel<32, 8, 64>", "rnorm_undo_fast_kernel<32, 8, 64>", "rnorm_fwd_fast_kernel<64, 12, 24>",
       "rnorm_undo_fast_kernel<64, 12, 24>", "rnorm_fwd_lds_kernel<64>/vec", "rnorm_fwd_lds_kernel<32>/vec", "rnorm_fwd_lds_kernel<16>/vec",
       "rnorm_fwd_lds_kernel<64>/scalar", "rnorm_fwd_lds_kernel<32>/scalar", "rnorm_fwd_kernel/vec/segments", "rnorm_fwd_kernel/scalar/segments",
       "rnorm_undo_lds_kernel<64>/256/vec", "rnorm_undo_lds_kernel<16>/512/vec", "rnorm_undo_lds_kernel<16>/256/scalar",
       "rnorm_undo_lds_kernel<8>/512/vec", "rnorm_undo_lds_kernel<8>/512/scalar", "rnorm_undo1_kernel+rnorm_undo2_kernel/vec",
       "rnorm_undo1_kernel+rnorm_undo2_kernel/scalar"])
