"""float64 restatement of the reference's batch normalisation (src/layer.cc:452-510) and of its three cudamat entries
(cudamat_kernels.cu:2077-2168), quirks included.

Arrays are (C, H): row c is channel c's contiguous run of H = N·X·Y floats — the reference's Reshape(-1, C) of a layer's state read
in memory order, i.e. ``flat.reshape(C, H)``.  Per-channel vectors are (C,)."""
import numpy as np


def fprop(x, gamma, beta, mu, sigma, bn_f, eps, train, relu=False):
    """Layer::ApplyBatchNormalization (+ the ReLU of a RECTIFIED_LINEAR layer).  Returns (y, running mu, running sigma, batch mu,
    batch sigma); the running statistics are averaged over the STD, and the variance is the biased one with eps before the sqrt."""
    x = np.asarray(x, np.float64)
    gamma, beta, mu, sigma = (np.asarray(v, np.float64) for v in (gamma, beta, mu, sigma))
    if train:
        mb = x.mean(axis=1)
        xc = x - mb[:, None]
        sb = np.sqrt((xc * xc).mean(axis=1) + eps)
        xh = xc / sb[:, None]
        mu = bn_f * mu + (1 - bn_f) * mb
        sigma = bn_f * sigma + (1 - bn_f) * sb
    else:
        mb = sb = None
        xh = (x - mu[:, None]) / sigma[:, None]
    y = gamma[:, None] * xh + beta[:, None]
    if relu:
        y = np.maximum(y, 0)
    return y, mu, sigma, mb, sb


def bprop(d, state, gamma, beta, batch_sigma):
    """Layer::ApplyDerivativeofBatchNormalization without the optimizer steps.  `state` is the layer's state as Bprop finds it —
    after the activation and dropout — so ReLU-clipped and dropped units recover y = -beta/gamma, not x-hat (the quirk the library
    mirrors).  Returns (d_in, dgamma, dbeta); dgamma and dbeta are MEANS over the column."""
    d = np.asarray(d, np.float64)
    gamma, beta, batch_sigma = (np.asarray(v, np.float64) for v in (gamma, beta, batch_sigma))
    y = (np.asarray(state, np.float64) - beta[:, None]) / gamma[:, None]
    dbeta = d.mean(axis=1)
    dgamma = (d * y).mean(axis=1)
    d = d - dgamma[:, None] * y
    d = d - d.mean(axis=1, keepdims=True)
    return d * (gamma / batch_sigma)[:, None], dgamma, dbeta


# ---- the cudamat entries (per column: row c here) ------------------------------------------------------------------------------------
def bn_bprop_inplace(d, act):
    d, act = np.asarray(d, np.float64), np.asarray(act, np.float64)
    dgamma = (d * act).mean(axis=1)
    d = d - dgamma[:, None] * act
    return d - d.mean(axis=1, keepdims=True), dgamma


def bn_bprop(d, x, gamma, mu, sigma, target, scale_targets):
    d, x, target = (np.asarray(v, np.float64) for v in (d, x, target))
    gamma, mu, sigma = (np.asarray(v, np.float64)[:, None] for v in (gamma, mu, sigma))
    H = d.shape[1]
    cs = ((x - mu) * d).sum(axis=1, keepdims=True) / ((H - 1) * sigma * sigma)
    val = gamma * (d - (x - mu) * cs) / sigma
    return scale_targets * target + val - val.mean(axis=1, keepdims=True)


def bn_grad(d, x, mu, sigma):
    d, x = np.asarray(d, np.float64), np.asarray(x, np.float64)
    z = (x - np.asarray(mu, np.float64)[:, None]) / np.asarray(sigma, np.float64)[:, None]
    return (z * d).sum(axis=1), d.sum(axis=1)
