"""numpy oracle for chunk_moments_u8 and convnet_amd.compute_mean: exact int64 sums, a float64 restatement of the statistics that
shares no arithmetic with the integer path (two passes over centred float64 data), and a float32 restatement of the float op sequence
(the reference's apps/compute_mean.cc order: per-piece sums, E[x^2] - mean^2) that shows what that sequence loses.

``rows`` is always the dataset as stored: (cases, dims) with [colour][row][col] inside a row."""
import numpy as np


def int_moments(rows, num_colors, acc=None):
    """What chunk_moments_u8 adds into ``acc`` (2 * dims + C * C sums) for these rows, as int64."""
    x = np.asarray(rows).astype(np.int64)
    n, dims = x.shape
    C = int(num_colors)
    out = np.zeros(2 * dims + C * C, np.int64) if acc is None else np.array(acc, np.int64)
    out[:dims] += x.sum(0)
    out[dims:2 * dims] += (x * x).sum(0)
    ch = x.reshape(n, C, dims // C)
    out[2 * dims:] += np.einsum("ncp,ndp->cd", ch, ch).reshape(-1)
    return out


def eig_su(pixel_cov):
    """S (C,) and U (C, C) of a correlation matrix: S = sqrt(eigenvalues) descending, clamped at 0; ROW k of U is eigenvector k, its
    largest component positive, so U.T @ diag(S^2) @ U = pixel_cov."""
    w, v = np.linalg.eigh(np.asarray(pixel_cov, np.float64))
    order = np.argsort(w)[::-1]
    U = v[:, order].T.copy()
    for u in U:
        if u[np.argmax(np.abs(u))] < 0:
            u *= -1
    return np.sqrt(np.maximum(w[order], 0.0)), U


def stats_float64(rows, num_colors):
    """Every dataset of a mean file in float64, two passes: centre, then average the squares and the products."""
    x = np.asarray(rows).astype(np.float64)
    n, dims = x.shape
    C = int(num_colors)
    mean = x.mean(0)
    std = np.sqrt(((x - mean) ** 2).mean(0))
    ch = x.reshape(n, C, dims // C).transpose(1, 0, 2).reshape(C, -1)       # (C, cases * pixels)
    pixel_mean = ch.mean(1)
    centred = ch - pixel_mean[:, None]
    pixel_std = np.sqrt((centred ** 2).mean(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        pixel_cov = (centred @ centred.T) / ch.shape[1] / np.outer(pixel_std, pixel_std)
    out = {"mean": mean, "std": std, "pixel_mean": pixel_mean, "pixel_std": pixel_std, "pixel_cov": pixel_cov}
    if np.all(pixel_std > 0):
        out["S"], out["U"] = eig_su(pixel_cov)
    return out


def stats_float32_sequence(rows, num_colors, piece):
    """The float op sequence in float32 numpy, piece by piece: sums of x and x * x per (position in the piece, dim), the C x C product
    scaled by 1 / (cases * pixels) per piece, then column sums, E[x^2] - mean^2, sqrt — every intermediate rounded to float32."""
    f = np.float32
    x = np.asarray(rows).astype(f)
    n, dims = x.shape
    C = int(num_colors)
    P = dims // C
    sums, sqs = {}, {}
    cov = np.zeros((C, C), f)
    for a in range(0, n, piece):
        s = x[a:a + piece]
        k = len(s)
        sums[k] = sums.get(k, np.zeros((k, dims), f)) + s
        sqs[k] = sqs.get(k, np.zeros((k, dims), f)) + s * s
        ch = s.reshape(k, C, P).transpose(1, 0, 2).reshape(C, -1)
        cov = cov + (ch @ ch.T).astype(f) * f(1.0 / (n * P))
    inv_n, inv_p = f(1.0 / n), f(1.0 / P)
    mean = sum((m.sum(0, dtype=f) * inv_n for m in sums.values()), np.zeros(dims, f)).astype(f)
    sq = sum((m.sum(0, dtype=f) * inv_n for m in sqs.values()), np.zeros(dims, f)).astype(f)
    pixel_mean = (mean.reshape(C, P).sum(1, dtype=f) * inv_p).astype(f)
    pixel_sq = (sq.reshape(C, P).sum(1, dtype=f) * inv_p).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(sq - mean * mean)
        pixel_std = np.sqrt(pixel_sq - pixel_mean * pixel_mean)
        pixel_cov = (cov - np.outer(pixel_mean, pixel_mean)) / np.outer(pixel_std, pixel_std)
    out = {"mean": mean, "std": std, "pixel_mean": pixel_mean, "pixel_std": pixel_std, "pixel_cov": pixel_cov.astype(f)}
    if np.all(np.isfinite(pixel_cov)) and np.all(pixel_std > 0):
        S, U = eig_su(pixel_cov)
        out["S"], out["U"] = S.astype(f), U.astype(f)
    return out


def scale_relative_error(got, ref):
    """max |got - ref| / max |ref| of one dataset: the error on the dataset's own scale (entries of pixel_cov and U pass through 0)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def within_ulps(got, ref, ulps=1):
    """``got`` (float32) is within ``ulps`` float32 ulps of ``ref`` (float64), everywhere."""
    got = np.asarray(got)
    assert got.dtype == np.float32, got.dtype
    ref = np.asarray(ref, np.float64)
    step = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return bool(np.all(np.abs(got.astype(np.float64) - ref) <= ulps * step))
