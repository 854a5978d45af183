"""numpy restatements of the logistic and softmax-distribution entries of include/convnet_hip.h, written from that header and from the
reference's CPU semantics (eigenmat/eigenmat.cc:1133-1151, 1344-1392, 1543-1557, 1771-1786), not from the HIP code.

Layout as in tests/elementwise_ref.py: a column-major (rows, cols) matrix is a numpy array of shape (cols, rows); `a[j, i]` is row i of
column j.  Where the library promises separately rounded fp32 operations every statement below is ONE np.float32 operation; the `_f64`
forms are for entries that promise a tolerance only.  tests/test_logistic_ref_cpu.py pins the semantics on hand-written cases."""
import numpy as np

f32 = np.float32


def sigmoid_f64(x):
    """1 / (1 + exp(-x)) in float64: exactly 1 for large x, 0 for very negative x (exp overflows to inf), NaN for NaN"""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def logistic_deriv(d, y, scale=1.0):
    """((d * scale) * y) * (1 - y), every operation rounded to fp32; scale == 1 skips the first product"""
    d, y = np.asarray(d, f32), np.asarray(y, f32)
    if f32(scale) != f32(1):
        d = d * f32(scale)
    dy = d * y
    om = f32(1) - y
    return dy * om


def logistic_grad(y, t, scale=None):
    """t < 0 ? 0 : y - t (a negative target: don't care); then times scale when given"""
    y, t = np.asarray(y, f32), np.asarray(t, f32)
    g = np.where(t < 0, f32(0), y - t).astype(f32)
    return g if scale is None else g * f32(scale)


def logistic_correct_normalized(p, t):
    """per ROW (the last axis of the (cols, rows) arrays): the share of entries with t >= 0 whose (p >= 0.5) agrees with (t >= 0.5);
    0 where no entry counts.  Integer counts, one fp32 division: (rows,) float32"""
    p, t = np.asarray(p, f32), np.asarray(t, f32)
    counted = ~(t < 0)
    agree = ((t >= 0.5) & (p >= 0.5)) | ((t < 0.5) & (p < 0.5))
    correct = (counted & agree).sum(axis=0).astype(f32)
    total = counted.sum(axis=0).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total > 0, correct / total, f32(0)).astype(f32)


def cross_entropy_f64(t, p, tiny):
    """-t * log(p + tiny); p + tiny is formed in fp32 as the entry forms it, the rest in float64"""
    s = (np.asarray(p, f32) + f32(tiny)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.asarray(t, np.float64) * np.log(s)


def softmax_rows_f64(x):
    """row softmax of a (cols, rows) array in float64"""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def dropout_mask(y, s):
    """the units a dropout(p, 0, scale) pass zeroed, given its input s (which must hold no zero) and its output y"""
    assert np.all(np.asarray(s) != 0)
    return np.asarray(y) == 0
