"""numpy restatements of the resampling entries and the colour transform (include/convnet_hip.h: UpSampleGemm, DownSampleGemm, RGBToYUV),
written from their definitions; no code shared with the package.  Shared by tests/test_resample_cpu.py and tests/test_resample_gpu.py.

Layout: a matrix is (N, X*Y*C) with the image index fastest, element (n, x, y, c) at n + N*(x + W*(y + H*c)).  As a C-ordered numpy array
that is shape (C, H, W, N); ``to_chwn`` / ``from_chwn`` go between that and the flat buffer a Matrix holds."""
import numpy as np

# the reference's rows (cudamat_conv_others.cu:298-300)
YUV = ((0.2126, 0.7152, 0.0722), (-0.09991, -0.33609, 0.436), (0.615, -0.55861, -0.05639))


def to_chwn(flat, N, W, H, C):
    return np.asarray(flat).reshape(C, H, W, N)


def from_chwn(t):
    return np.ascontiguousarray(t).reshape(-1)


def upsample(x, f, targets=None, scale_targets=0.0):
    """x: (C, H, W, N) float32.  scale_targets == 0: the replicated input itself.  Otherwise scale_targets * targets + replicated, the
    product and the sum each rounded to float32 (scale_targets == 1: the product is exact)."""
    rep = np.repeat(np.repeat(np.asarray(x, np.float32), f, axis=1), f, axis=2)
    if scale_targets == 0:
        return rep
    prod = (np.float32(scale_targets) * np.asarray(targets, np.float32)).astype(np.float32)
    return (prod + rep).astype(np.float32)


def upsample_reference_forms(x, f):
    """What the two builds of the reference leave for scaleTargets = 0, in float32 arithmetic: the GPU build's (f*f * x) / (f*f) and the
    CPU build's f*f * (x * (1 / (f*f))), each replicated."""
    x = np.asarray(x, np.float32)
    ff = np.float32(f * f)
    gpu = ((ff * x).astype(np.float32) / ff).astype(np.float32)
    cpu = (ff * (x * (np.float32(1) / ff)).astype(np.float32)).astype(np.float32)
    rep = lambda a: np.repeat(np.repeat(a, f, axis=1), f, axis=2)  # noqa: E731
    return rep(gpu), rep(cpu)


def downsample64(x, f):
    """x: (C, H*f, W*f, N).  The mean of each f x f block in float64."""
    C, Hf, Wf, N = x.shape
    return np.asarray(x, np.float64).reshape(C, Hf // f, f, Wf // f, f, N).mean(axis=(2, 4))


def rgb_to_yuv64(x):
    """x: (3, pixels..., N) -> (yuv float64, the bound's sum |a R| + |b G| + |c B| per element)."""
    x = np.asarray(x, np.float64)
    m = np.asarray(YUV, np.float32).astype(np.float64)      # the constants are float32 literals
    out = np.stack([m[k, 0] * x[0] + m[k, 1] * x[1] + m[k, 2] * x[2] for k in range(3)])
    mag = np.stack([abs(m[k, 0] * x[0]) + abs(m[k, 1] * x[1]) + abs(m[k, 2] * x[2]) for k in range(3)])
    return out, mag
