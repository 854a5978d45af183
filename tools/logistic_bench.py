"""The fused logistic / softmax-distribution entries on one MI355X (csrc/elementwise.hip) against the call sequences they replace, same
library, same process: prints ONE JSON line and writes it to --out.

Each pair is timed with HIP events around --inner back-to-back calls (a single call of the output-layer entries is a few
microseconds), fused and unfused windows alternating, median of --reps windows:
  logistic_dropout        vs apply_sigmoid + dropout                                   hidden layers (256, 4096) and (256, 64*27*27)
  logistic_deriv_scaled   vs mult_by_scalar + apply_logistic_deriv                     the same two
  logistic_ce_grad_correct vs apply_sigmoid + apply_logistic_grad + mult_by_scalar + get_logistic_correct_normalized [+ sum_all]
                                                                                       output layer (256, 1000)
  softmax_dist_ce_grad    vs softmax_row_major + subtract_elementwise + mult_by_scalar + compute_cross_entropy [+ sum_all]
                                                                                       output layer (256, 1000)
sum_all returns a float to the host (a device-to-host copy and a synchronise per step, which the fused entries' on-device accumulator
avoids); the unfused output sequences are timed with it, as the unfused host runs them, and without it (device work only).
Recorded per entry: microseconds per call, the bytes the entry (or each call of the sequence) must move at 4 per float per array
read or written, and the GB/s that is.

    python tools/logistic_bench.py [--reps 30] [--inner 20] [--out profiles/logistic_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)

HIDDEN = [("hidden 256x4096", 256, 4096), ("hidden 256x(64*27*27)", 256, 64 * 27 * 27)]
OUTPUT = [("output 256x1000", 256, 1000)]
P, SCALE, DERIV_SCALE, TINY = 0.4, 1.0 / (1 - 0.4), 0.5, 1e-10


def _window(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def _compare(fns, reps, inner):
    """{name: median microseconds per call}; the candidates' windows alternate."""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_window(fn, inner))
    return {k: statistics.median(v) for k, v in ts.items()}


def _mat(rows, cols, fill):
    import torch
    from convnet_amd.matrix import Matrix
    m = Matrix()
    m.AllocateGPUMemory(rows, cols)
    g = torch.Generator(device="cuda").manual_seed(rows + cols)
    if fill == "normal":
        m.tensor().normal_(generator=g)
    elif fill == "unit":
        m.tensor().uniform_(0.0, 1.0, generator=g)
    else:
        m.Set(fill)
    return m


def _row(shape, entry, n, us, fused_bytes, unfused_bytes, extra=None):
    r = dict(shape=shape, entry=entry, floats=n,
             fused=dict(us=round(us["fused"], 2), bytes=int(fused_bytes), GBps=round(fused_bytes / us["fused"] * 1e-3, 1)),
             unfused=dict(us=round(us["unfused"], 2), bytes=int(unfused_bytes), GBps=round(unfused_bytes / us["unfused"] * 1e-3, 1)),
             fused_over_unfused=round(us["fused"] / us["unfused"], 3))
    if extra:
        r.update(extra)
    return r


def _hidden(reps, inner):
    from convnet_amd._lib import lib
    from convnet_amd.matrix import Matrix
    rows = []
    rnd = ctypes.byref(Matrix._rnd)
    for name, r, c in HIDDEN:
        n = r * c
        x, y, d = _mat(r, c, "normal"), _mat(r, c, "unit"), _mat(r, c, "normal")
        # the state is overwritten by its own sigmoid on every call: it stays in (0, 1) scaled, nothing drifts out of range
        us = _compare({
            "fused": lambda: lib.logistic_dropout(rnd, x.GetMat(), P, SCALE),
            "unfused": lambda: (lib.apply_sigmoid(x.GetMat(), x.GetMat()), lib.dropout(rnd, x.GetMat(), P, 0.0, SCALE))}, reps, inner)
        rows.append(_row(name, "logistic_dropout", n, us, 8.0 * n, 16.0 * n))
        # the derivative shrinks by y (1 - y) <= 1/4 per call and is refilled per shape: denormals are not slower on this path
        us = _compare({
            "fused": lambda: lib.logistic_deriv_scaled(d.GetMat(), y.GetMat(), SCALE),
            "unfused": lambda: (lib.mult_by_scalar(d.GetMat(), SCALE, d.GetMat(), 0.0),
                                lib.apply_logistic_deriv(d.GetMat(), y.GetMat(), d.GetMat()))}, reps, inner)
        rows.append(_row(name, "logistic_deriv_scaled", n, us, 12.0 * n, 20.0 * n))
    return rows


def _output(reps, inner):
    from convnet_amd._lib import lib
    rows = []
    err = ctypes.c_int(0)
    for name, r, c in OUTPUT:
        n = r * c
        logits, t, probs, deriv = _mat(r, c, "normal"), _mat(r, c, "unit"), _mat(r, c, 0.0), _mat(r, c, 0.0)
        share, ce, acc = _mat(r, 1, 0.0), _mat(r, c, 0.0), _mat(1, 1, 0.0)
        L, T, Pm, D, S, C, A = (m.GetMat() for m in (logits, t, probs, deriv, share, ce, acc))

        def logistic_seq(read_back):
            lib.apply_sigmoid(L, Pm)
            lib.apply_logistic_grad(Pm, T, D)
            lib.mult_by_scalar(D, DERIV_SCALE, D, 0.0)
            lib.get_logistic_correct_normalized(Pm, T, S)
            if read_back:
                lib.sum_all(S, ctypes.byref(err))

        us = _compare({"fused": lambda: lib.logistic_ce_grad_correct(L, T, Pm, D, A, DERIV_SCALE),
                       "unfused": lambda: logistic_seq(True), "unfused_device_only": lambda: logistic_seq(False)}, reps, inner)
        rows.append(_row(name, "logistic_ce_grad_correct", n, us, 16.0 * n, (8.0 + 12.0 + 8.0 + 8.0) * n + 8.0 * r,
                         dict(unfused_device_only_us=round(us["unfused_device_only"], 2),
                              fused_over_unfused_device_only=round(us["fused"] / us["unfused_device_only"], 3))))

        def softmax_seq(read_back):
            lib.softmax_row_major(L, Pm)
            lib.subtract_elementwise(Pm, T, D)
            lib.mult_by_scalar(D, DERIV_SCALE, D, 0.0)
            lib.compute_cross_entropy(T, Pm, C, TINY)
            if read_back:
                lib.sum_all(C, ctypes.byref(err))

        us = _compare({"fused": lambda: lib.softmax_dist_ce_grad(L, T, Pm, D, A, DERIV_SCALE, TINY),
                       "unfused": lambda: softmax_seq(True), "unfused_device_only": lambda: softmax_seq(False)}, reps, inner)
        rows.append(_row(name, "softmax_dist_ce_grad", n, us, 16.0 * n, (8.0 + 12.0 + 8.0 + 12.0 + 4.0) * n,
                         dict(unfused_device_only_us=round(us["unfused_device_only"], 2),
                              fused_over_unfused_device_only=round(us["fused"] / us["unfused_device_only"], 3))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logistic_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "logistic_bench needs an MI355X"
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(1)
    rows = _hidden(a.reps, a.inner) + _output(a.reps, a.inner)
    line = dict(tool="logistic_bench", device=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, entries=rows,
                every_fused_entry_no_slower=all(r["fused_over_unfused"] <= 1.0 for r in rows))
    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
