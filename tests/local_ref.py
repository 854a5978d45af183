"""float64 restatement of the locally connected layer (include/convnet_hip.h, "locally connected layers"; src/local_edge.cc) — the
oracle of the local kernels.  numpy only; test infrastructure.

Arrays are the library's column-major matrices viewed as C-order numpy arrays:
  images  (C, H, W, N)             the (N, H*W*C) activation matrix
  outputs (F, My, Mx, N)           the (N, My*Mx*F) output matrix
  bank    (M, C, Ky, Kx, F)        the (F, Kx*Ky*C*M) filter bank: module m = my*Mx + mx owns the F*K floats at m*F*K
`pad` is the pbtxt (positive) padding; the ConvDesc carries it negated.
"""
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class LocalGeom:
    N: int
    C: int
    H: int
    W: int
    F: int
    Ky: int
    Kx: int
    sy: int = 1
    sx: int = 1
    pady: int = 0
    padx: int = 0

    @property
    def My(self):
        return (self.H + 2 * self.pady - self.Ky) // self.sy + 1

    @property
    def Mx(self):
        return (self.W + 2 * self.padx - self.Kx) // self.sx + 1

    @property
    def M(self):
        return self.My * self.Mx

    @property
    def K(self):
        return self.C * self.Ky * self.Kx

    def in_shape(self):
        return (self.C, self.H, self.W, self.N)

    def out_shape(self):
        return (self.F, self.My, self.Mx, self.N)

    def bank_shape(self):
        return (self.M, self.C, self.Ky, self.Kx, self.F)

    def flops(self):
        return 2.0 * self.N * self.F * self.K * self.M


def _patches(g, x):
    """P[m, c, ky, kx, n] = x[c, my*sy + ky - pady, mx*sx + kx - padx, n] (0 on a padding tap)"""
    xp = np.zeros((g.C, g.H + 2 * g.pady + g.sy * g.Ky, g.W + 2 * g.padx + g.sx * g.Kx, g.N))
    xp[:, g.pady:g.pady + g.H, g.padx:g.padx + g.W] = x
    P = np.empty((g.My, g.Mx, g.C, g.Ky, g.Kx, g.N))
    for ky in range(g.Ky):
        for kx in range(g.Kx):
            v = xp[:, ky:ky + g.sy * g.My:g.sy, kx:kx + g.sx * g.Mx:g.sx]   # (C, My, Mx, N)
            P[:, :, :, ky, kx] = v.transpose(1, 2, 0, 3)
    return P.reshape(g.M, g.C, g.Ky, g.Kx, g.N), xp.shape


def up(g, x, w, target=None, scale_targets=0.0):
    P, _ = _patches(g, np.asarray(x, np.float64))
    out = np.einsum("mckxf,mckxn->fmn", np.asarray(w, np.float64).reshape(g.bank_shape()), P).reshape(g.out_shape())
    return out if target is None or scale_targets == 0 else scale_targets * np.asarray(target, np.float64) + out


def down(g, dy, w, target=None, scale_targets=0.0):
    dP = np.einsum("mckxf,fmn->mckxn", np.asarray(w, np.float64).reshape(g.bank_shape()),
                   np.asarray(dy, np.float64).reshape(g.F, g.M, g.N)).reshape(g.My, g.Mx, g.C, g.Ky, g.Kx, g.N)
    _, shape = _patches(g, np.zeros((g.C, g.H, g.W, 1)))
    xp = np.zeros(shape[:3] + (g.N,))
    for ky in range(g.Ky):
        for kx in range(g.Kx):
            xp[:, ky:ky + g.sy * g.My:g.sy, kx:kx + g.sx * g.Mx:g.sx] += dP[:, :, :, ky, kx].transpose(2, 0, 1, 3)
    out = xp[:, g.pady:g.pady + g.H, g.padx:g.padx + g.W]
    return out if target is None or scale_targets == 0 else scale_targets * np.asarray(target, np.float64) + out


def outp(g, x, dy, target=None, scale_targets=0.0, scale_output=1.0):
    P, _ = _patches(g, np.asarray(x, np.float64))
    dw = scale_output * np.einsum("fmn,mckxn->mckxf", np.asarray(dy, np.float64).reshape(g.F, g.M, g.N), P)
    return dw if target is None or scale_targets == 0 else scale_targets * np.asarray(target, np.float64).reshape(dw.shape) + dw


def up_at(g, x, w, f, my, mx, n):
    """one output element, for layers too large for a whole-tensor pass"""
    m = my * g.Mx + mx
    acc = 0.0
    for ky in range(g.Ky):
        for kx in range(g.Kx):
            iy, ix = my * g.sy + ky - g.pady, mx * g.sx + kx - g.padx
            if 0 <= iy < g.H and 0 <= ix < g.W:
                acc += float(np.dot(x[:, iy, ix, n].astype(np.float64), w[m, :, ky, kx, f].astype(np.float64)))
    return acc


def down_at(g, dy, w, c, iy, ix, n):
    acc = 0.0
    for ky in range(g.Ky):
        for kx in range(g.Kx):
            ty, tx = iy + g.pady - ky, ix + g.padx - kx
            if ty % g.sy or tx % g.sx:
                continue
            my, mx = ty // g.sy, tx // g.sx
            if 0 <= my < g.My and 0 <= mx < g.Mx:
                acc += float(np.dot(dy[:, my, mx, n].astype(np.float64), w[my * g.Mx + mx, c, ky, kx, :].astype(np.float64)))
    return acc


def outp_at(g, x, dy, m, c, ky, kx, f):
    my, mx = divmod(m, g.Mx)
    iy, ix = my * g.sy + ky - g.pady, mx * g.sx + kx - g.padx
    if not (0 <= iy < g.H and 0 <= ix < g.W):
        return 0.0
    return float(np.dot(x[c, iy, ix].astype(np.float64), dy[f, my, mx].astype(np.float64)))


# ---- an independent formulation on torch (CPU, float64): unfold / fold ------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def torch_up(g, x, w):
    import torch.nn.functional as Fn
    U = Fn.unfold(_t(x).permute(3, 0, 1, 2), (g.Ky, g.Kx), padding=(g.pady, g.padx), stride=(g.sy, g.sx))   # (N, K, M)
    Wt = _t(w).reshape(g.M, g.K, g.F)
    out = (U.permute(2, 0, 1) @ Wt)                                                                         # (M, N, F)
    return out.permute(2, 0, 1).reshape(g.out_shape()).numpy()


def torch_down(g, dy, w):
    import torch.nn.functional as Fn
    Wt = _t(w).reshape(g.M, g.K, g.F)
    D = _t(dy).reshape(g.F, g.M, g.N).permute(1, 2, 0)                                                      # (M, N, F)
    dU = (D @ Wt.transpose(1, 2)).permute(1, 2, 0)                                                          # (N, K, M)
    dx = Fn.fold(dU, (g.H, g.W), (g.Ky, g.Kx), padding=(g.pady, g.padx), stride=(g.sy, g.sx))               # (N, C, H, W)
    return dx.permute(1, 2, 3, 0).numpy()


def torch_outp(g, x, dy):
    import torch.nn.functional as Fn
    U = Fn.unfold(_t(x).permute(3, 0, 1, 2), (g.Ky, g.Kx), padding=(g.pady, g.padx), stride=(g.sy, g.sx))   # (N, K, M)
    D = _t(dy).reshape(g.F, g.M, g.N).permute(1, 2, 0)                                                      # (M, N, F)
    dW = U.permute(2, 1, 0) @ D                                                                             # (M, K, F)
    return dW.reshape(g.bank_shape()).numpy()


# ---- the parameter slice of a LocalEdge (src/local_edge.cc) -----------------------------------------------------------------------
def local_edge_sizes(g, has_bias=True):
    """(parameter count, weight slice (rows, cols), bias slice (rows, cols) after Reshape(1, -1), Shape4D of the weights)"""
    input_size = g.Kx * g.Ky * g.C * g.My * g.Mx
    bias_locs = g.My * g.Mx
    n = g.F * (input_size + (bias_locs if has_bias else 0))
    return n, (g.F, input_size), ((1, g.F * bias_locs) if has_bias else None), (g.F, g.Kx, g.Ky, g.C * g.My * g.Mx)
