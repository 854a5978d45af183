"""numpy restatements of the element-wise, reduction, output-layer and fused-SGD entries of include/convnet_hip.h, written from that header
and from the reference's CPU semantics (eigenmat/eigenmat.cc), not from the HIP code.

Layout: a column-major (rows, cols) matrix is a numpy array of shape (cols, rows), as in oracle/__init__.py; `a[j, i]` is row i of
column j.  Where the library promises separately rounded fp32 operations every statement below is ONE np.float32 operation (numpy
rounds each to nearest; sqrt and / are correctly rounded).  The `_f64` forms are for entries that promise a tolerance only.
tests/test_elementwise_ref_cpu.py holds these against the oracle's compiled C."""
import numpy as np

f32 = np.float32
EPS = 2.0 ** -23          # one rounding of an fp32 result, relative to the result's magnitude


# ---- element for element (cudamat.cuh:170-263; eigenmat.cc:656-713, 1805-1900) ------------------------------------------------------
def add_elementwise(x, y):
    return x + y


def subtract_elementwise(x, y):
    return x - y


def mult_elementwise(x, y):
    return x * y


def mult_by_scalar(x, alpha):
    return x * f32(alpha)


def mult_by_scalar_f64(x, alpha, t, scale_targets):
    """target = scale_targets*target + x*alpha, which the library may contract: (exact value, two roundings' worth of it)"""
    a, b = np.float64(f32(scale_targets)) * t.astype(np.float64), x.astype(np.float64) * np.float64(f32(alpha))
    return a + b, EPS * (np.abs(a) + np.abs(b))


def divide_by_scalar(x, alpha):
    return x / f32(alpha)


def add_scalar(x, alpha):
    return x + f32(alpha)


def apply_sqrt(x):
    return np.sqrt(x)


def assign_scalar(x, alpha):
    return np.full_like(x, f32(alpha))


def lower_bound_scalar(x, val):
    return np.where(x > f32(val), x, f32(val))


def upper_bound_mod_scalar(x, val):
    v = f32(val)
    return np.where(x > v, v, np.where(x < -v, -v, x))


def relu_deriv(d, s):
    """deriv * (state > 0): a masked-out derivative keeps its sign (0 * d)"""
    return d * (s > 0).astype(np.float32)


def add_mult(x, y, alpha):
    """x += alpha*y: the product rounded, then the sum"""
    t = f32(alpha) * y
    return x + t


# ---- row / column vectors (eigenmat.cc:325-370, 439-560) -----------------------------------------------------------------------------
def add_row_mult(mat, vec, mult=1.0):
    """mat[:, j] += mult*vec[j]; vec has one entry per column"""
    t = f32(mult) * vec
    return mat + t[:, None]


def add_col_mult(mat, vec, mult=1.0):
    """mat[i, :] += mult*vec[i]; vec has one entry per row"""
    t = f32(mult) * vec
    return mat + t[None, :]


def div_by_col_vec(mat, vec):
    return mat / vec[None, :]


def mult_by_row_vec(mat, vec):
    return mat * vec[:, None]


def div_by_row_vec(mat, vec):
    return mat / vec[:, None]


def add_to_each_pixel(mat1, mat2, mult):
    """mat1: (colours*pixels, cases), mat2: (colours, cases) — every pixel of colour c of case n gets mult*mat2[c, n]"""
    per = mat1.shape[0] // mat2.shape[0]
    t = f32(mult) * mat2
    return mat1 + np.repeat(t, per, axis=0)


def vec_f64(mat, vec, mult, along):
    """mat + mult*vec in float64 with a two-roundings bound, for a mult whose product is not exact.  along: "row" | "col" """
    v = np.float64(f32(mult)) * vec.astype(np.float64)
    v = v[:, None] if along == "row" else v[None, :]
    return mat.astype(np.float64) + v, EPS * (np.abs(mat).astype(np.float64) + np.abs(v))


# ---- reductions ------------------------------------------------------------------------------------------------------------------------
def axis_total_exact(mat, axis, sq):
    """int64 column (axis 0) or row (axis 1) sums of an integer-valued matrix [of its squares]"""
    k = np.rint(mat).astype(np.int64)
    assert np.array_equal(k.astype(np.float32), mat), "integer-valued input expected"
    return (k * k if sq else k).sum(axis=1 if axis == 0 else 0)


def sum_by_axis_exact(mat, target, axis, mult, p, sq=False):
    """target = p*target + mult*sum for integer-valued data, mult and p powers of two, an integer-valued target: every term and the result
    are exact in fp32 (test_elementwise_ref_cpu.py proves the bound), so the statements below round nothing.  p == 0 ignores the target."""
    s = axis_total_exact(mat, axis, sq).astype(np.float32)
    old = f32(p) * target if p != 0 else np.zeros_like(target)
    return old + f32(mult) * s


def sum_by_axis_f64(mat, target, axis, mult, p, sq=False):
    m = mat.astype(np.float64)
    s = (m * m if sq else m).sum(axis=1 if axis == 0 else 0)
    return (p * target.astype(np.float64) if p != 0 else 0.0) + mult * s


def sum_all_f64(x):
    return float(x.astype(np.float64).sum())


def vdot_f64(x, y):
    return float(np.dot(x.astype(np.float64).reshape(-1), y.astype(np.float64).reshape(-1)))


def euclid_norm_from(sumsq):
    """euclid_norm = sqrt of the fp32 sum of squares"""
    return np.sqrt(f32(sumsq))


# ---- norm limit (eigenmat.cc:918-968) and the SGD step (src/optimizer.cc:174-200, 75-81) ------------------------------------------------
def normlimit(mat, norm, constraint, axis=1):
    """Every row (axis 1) or column (axis 0) scaled to `norm` when its 2-norm exceeds it (always, under constraint).  The sum of squares
    runs in index order, every step one product and one sum in fp32, as eigenmat's loop; on grid data every order gives the same."""
    m = mat if axis == 1 else mat.T                       # m[k, u]: element k of unit u
    s = np.zeros(m.shape[1], np.float32)
    for k in range(m.shape[0]):
        v = m[k]
        s = s + v * v
    s = np.sqrt(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where((s > f32(norm)) | bool(constraint), f32(norm) / s, f32(1))
    out = m * f[None, :]
    return out if axis == 1 else np.ascontiguousarray(out.T)


def sgd_step(g, w, h, l2, clip, eps, mom, norm_limit=0.0, norm_constraint=0.0):
    """g += l2*w; clip; g *= eps; h = mom*h + g; w -= h; then the row-norm constraint or limit.  Returns (g, w, h)."""
    if l2 > 0:
        t = w * f32(l2)
        g = g + t
    if clip > 0:
        g = upper_bound_mod_scalar(g, clip)
    g = g * f32(eps)
    hm = h * f32(mom)
    h = hm + g
    w = w - h
    if norm_constraint > 0:
        w = normlimit(w, norm_constraint, True)
    elif norm_limit > 0:
        w = normlimit(w, norm_limit, False)
    return g, w, h


# ---- output layer: one case per matrix ROW (eigenmat.cc:1093-1289) ----------------------------------------------------------------------
def softmax_f64(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def softmax_f32(z):
    """eigenmat's loop in fp32: max, exp(x - max), the sum in column order, divide"""
    mx = z.max(axis=0)
    e = np.exp(z - mx[None, :])
    s = np.zeros(z.shape[1], np.float32)
    for j in range(z.shape[0]):
        s = s + e[j]
    return e / s[None, :]


def softmax_grad(p, labels):
    out = p.copy()
    rows = np.arange(p.shape[1])
    out[labels.astype(np.int64), rows] -= f32(1)
    return out


def softmax_correct(p, labels):
    """1 where the FIRST maximum of the row is the label (a scan with strict <)"""
    return (np.argmax(p, axis=0) == labels.astype(np.int64)).astype(np.float32)


def softmax_ce_f64(p, labels, tiny):
    rows = np.arange(p.shape[1])
    return -np.log((p[labels.astype(np.int64), rows] + f32(tiny)).astype(np.float64))


def softmax_ce_f32(p, labels, tiny):
    rows = np.arange(p.shape[1])
    return -np.log(p[labels.astype(np.int64), rows] + f32(tiny))


# ---- inputs whose sums no order of summation can change ----------------------------------------------------------------------------------
def integer_data(rng, shape, bound):
    """integer-valued floats in [-bound, bound]"""
    return rng.integers(-bound, bound + 1, shape).astype(np.float32)


GRID = 8        # grid data: k / GRID with integer |k| <= GRID; squares are multiples of 1/GRID^2 and at most 1


def grid_data(rng, shape):
    k = rng.integers(-GRID, GRID + 1, shape)
    return (k / GRID).astype(np.float32)


def abs_total_in_units(x, unit):
    """sum |x| in units of `unit`, as an exact integer (x must lie on the grid of `unit`)"""
    k = np.rint(x.astype(np.float64) / unit).astype(np.int64)
    assert np.array_equal(k * np.float64(unit), x.astype(np.float64)), "input off the grid"
    return int(np.abs(k).sum())


# ---- the exact-arithmetic cases of tests/test_elementwise_gpu.py: shapes and inputs, shared with test_elementwise_ref_cpu.py, which proves
# ---- on these very arrays that no order of fp32 summation can change a sum ------------------------------------------------------------------
# (rows, cols, misaligned, which launch of axis_sum the shape selects)
AXIS0_SHAPES = [
    (32768, 3, False, "split: vector slabs, 8 splits"),
    (32771, 3, False, "split: scalar slabs, ragged last slab"),
    (32768, 3, True, "split: scalar although rows % 4 == 0"),
    (32768, 300, False, "split: splits limited by 2048 / cols"),
    (2048, 5, False, "block: vector"),
    (2050, 5, False, "block: scalar"),
    (2048, 5, True, "block: scalar by alignment"),
    (5000, 1025, False, "block: cols >= 1024 keeps a tall matrix off the split path"),
    (128, 4096, False, "wave4"),
    (132, 4099, False, "wave4: ragged last block of columns"),
    (2044, 4097, False, "wave4: tallest"),
    (1, 7, False, "wave: one row"),
    (63, 5, False, "wave: fewer rows than lanes"),
    (130, 4100, False, "wave: rows % 4 != 0"),
    (128, 4096, True, "wave: falls off wave4 by alignment"),
]
AXIS1_SHAPES = [(1, 9, False, "rows"), (255, 3, False, "rows"), (257, 1, False, "rows: two blocks"), (300, 70, False, "rows")]
MULT_P = [(1.0, 0.0), (0.5, 1.0), (0.25, 0.5)]
REDUCE_SIZES = [1, 255, 65536 + 3, 2 * (1 << 20) + 5]


def _seed(*parts):
    return np.random.default_rng([int(p) for p in parts])


def axis_inputs(rows, cols, axis, kind):
    """(mat (cols, rows), target): kind "int" — integers in [-8, 8] and an integer target in [-8, 8]; "normal" — N(0, 1) both"""
    rng = _seed(1, rows, cols, axis, kind == "int")
    n_t = cols if axis == 0 else rows
    if kind == "int":
        return integer_data(rng, (cols, rows), 8), integer_data(rng, n_t, 8)
    return rng.standard_normal((cols, rows)).astype(np.float32), rng.standard_normal(n_t).astype(np.float32)


def reduce_inputs(n, kind):
    """two vectors of n: integers in [-8, 8] ([-2, 2] at the largest n), or N(0, 1)"""
    rng = _seed(2, n, kind == "int")
    if kind == "int":
        b = 2 if n > (1 << 20) else 8
        return integer_data(rng, n, b), integer_data(rng, n, b)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


NORMLIMIT_SHAPES = [(12, 30, False), (50, 37, False), (260, 130, False), (257, 321, False), (256, 65, True)]
NORMLIMIT_HUGE = (257, 131137)      # more than 4096 blocks of 256 rows x 64 columns: the chunk doubles once
NORMCOLS_SHAPES = [(1, 4), (300, 7), (1000, 3)]
SGD_NORMLIMIT_SHAPES = [(12, 30), (260, 130), (257, 321)]
SGD_CORNERS = [(0.0, 0.0), (0.25, 2.0)]      # (l2_decay, gradient_clip); epsilon = momentum = 0.5


def normlimit_split(rows):
    """rows [0, split) are the small ones of mode "mixed": a whole block of 256 rows where there is one"""
    return 256 if rows > 256 else rows // 2


def normlimit_inputs(rows, cols, mode, axis=1):
    """(mat (cols, rows) on the grid k/8 without an all-zero row / column, norm).  mode "above": every unit's norm exceeds `norm`;
    "below": none does; "mixed" (axis 1): rows [0, normlimit_split) are below and the others above."""
    rng = _seed(3, rows, cols, axis)
    mat = grid_data(rng, (cols, rows))
    units = rows if axis == 1 else cols
    if mode == "mixed":
        assert axis == 1
        split = normlimit_split(rows)
        mat[:, :split] = (rng.integers(-2, 3, (cols, split)) / GRID).astype(np.float32)
        mat[:, split:] = ((GRID - rng.integers(0, 3, (cols, rows - split))) * rng.choice([-1, 1], (cols, rows - split)) / GRID).astype(np.float32)
    first = mat[0] if axis == 1 else mat[:, 0]          # element 0 of every unit
    first[first == 0] = f32(1.0 / GRID)
    m64 = mat.astype(np.float64)
    norms = np.sqrt((m64 * m64).sum(axis=0 if axis == 1 else 1))
    assert norms.shape == (units,) and norms.min() > 0
    if mode == "above":
        norm = 0.5 * norms.min()
    elif mode == "below":
        norm = 2.0 * norms.max()
    else:
        lo, hi = norms[:split].max(), norms[split:].min()
        assert lo < hi, (lo, hi)
        norm = 0.5 * (lo + hi)
    return mat, float(f32(norm))


def sgd_inputs(rows, cols):
    """gradient, parameter, history: integers in [-4, 4].  With epsilon = momentum = 0.5, l2 = 0.25 and clip = 2 every intermediate of the
    step is a multiple of 1/8 and the stepped parameter is at most 8.5: its squares are multiples of 1/64."""
    rng = _seed(4, rows, cols)
    return tuple(integer_data(rng, (cols, rows), 4) for _ in range(3))
