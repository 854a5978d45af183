"""The Gaussian-dropout layer's reference arithmetic in numpy (src/layer.cc:369-377 forward, 399-404 and the activation's derivative
backward), for any dtype: np.float32 gives the bits the library's entries must give (every operation below is one IEEE operation,
rounded once, in the order the unfused entry sequence applies them), np.float64 the value tolerances are measured against.

tests/oracle_net.py replays stored noise as a plain multiply; it models neither the divide, nor noise <= 0 under ReLU', nor the clip.

``act``: 0 identity, 1 ReLU, 2 logistic — the codes of include/convnet_hip.h."""
import numpy as np


def noise(z, stddev, dtype=np.float32):
    """FillWithRandn's z -> the multiplier: Mult(stddev), then Add(1)."""
    z = np.asarray(z, dtype)
    return (z * dtype(stddev)).astype(dtype) + dtype(1)


def activation(x, act, dtype=np.float32):
    """The activation alone.  (The device's sigmoid goes through its own expf: for bit comparisons at act 2 take the device's
    apply_sigmoid result and pass act 0.)"""
    x = np.asarray(x, dtype)
    if act == 1:
        return np.where(x > 0, x, dtype(0)).astype(dtype)
    if act == 2:
        with np.errstate(over="ignore"):
            return (dtype(1) / (dtype(1) + np.exp(-x).astype(dtype))).astype(dtype)
    return x


def forward(x, n, act=0, max_act=-1.0, dtype=np.float32):
    """state = clip(act(x) * n): Mult(noise), then UpperBoundMod(max_act) when max_act > 0."""
    y = (activation(x, act, dtype) * np.asarray(n, dtype)).astype(dtype)
    if max_act > 0:
        m = dtype(max_act)
        y = np.where(y > m, m, np.where(y < -m, -m, y)).astype(dtype)
    return y


def backward(deriv, state, n, act=0, dtype=np.float32):
    """(derivative behind dropout' and the activation's derivative, restored state): d = deriv * n, s = state / n, then
    apply_rectified_linear_deriv(d, s) = s > 0 ? d : 0 * d, or apply_logistic_deriv(d, s) = (d * s) * (1 - s), three roundings."""
    deriv, state, n = (np.asarray(a, dtype) for a in (deriv, state, n))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = (deriv * n).astype(dtype)
        s = (state / n).astype(dtype)
        if act == 1:
            d = np.where(s > 0, d, (dtype(0) * d).astype(dtype)).astype(dtype)
        elif act == 2:
            d = ((d * s).astype(dtype) * (dtype(1) - s).astype(dtype)).astype(dtype)
    return d, s
