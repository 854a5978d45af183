"""The fused Gaussian-dropout entries on one MI355X (csrc/elementwise.hip: gauss_kernel) against the unfused sequences they replace,
the binary-dropout kernel and a device copy on the same shapes, same library, same process: prints ONE JSON line and writes it to --out.

Per state shape, (256, 4096) (fc6 / fc7 class) and (256, 69984) (AlexNet pool1 class, 72 MB):
  gaussian_dropout         act 1, max_act 10                                                      2 passes over the state
  unfused_forward          lower_bound_scalar, fill_with_randn, mult_by_scalar, add_scalar,
                           mult_elementwise, upper_bound_mod_scalar                               12 passes, and a noise matrix
  gaussian_dropout_undo    act 1, restore_state 0                                                 3 passes
  unfused_backward         mult_elementwise, divide_elementwise, apply_rectified_linear_deriv     9 passes
  relu_dropout             rng_kernel<relu_dropout>, the binary dropout of the same layer         2 passes
  copy                     copy_on_device of the same bytes                                       2 passes
Timed with HIP events around ``inner`` back-to-back calls, ``inner`` chosen per variant so that a window lasts about --window seconds;
after a warm-up the variants' windows alternate, median of --reps windows.  Recorded per variant: microseconds per call, bytes per
element (4 per float per array read or written), achieved GB/s.  The verdict per shape: a fused kernel that moves its bytes at 0.8 of
the copy's rate or better is bound by memory, otherwise by instruction issue (Philox's 32-bit multiplies, logf / sinf / cosf); the
binary-dropout kernel, which draws the same Philox quad without the normal transform, stands beside it.

    python tools/gaussian_dropout_bench.py [--reps 7] [--window 0.2] [--out profiles/gaussian_dropout_bench.json]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("fc 256x4096", 256, 4096), ("pool1 256x69984", 256, 69984)]
STDDEV, MAX_ACT, P = 0.5, 10.0, 0.5
BYTES_PER_ELEMENT = dict(gaussian_dropout=8, unfused_forward=48, gaussian_dropout_undo=12, unfused_backward=36, relu_dropout=8, copy=8)
MEMORY_BOUND_AT = 0.8      # of the copy's rate


def _window(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner      # seconds per call


def _compare(fns, reps, window):
    """{name: (median microseconds per call, calls per window)}; every variant warmed up, then the variants' windows alternate."""
    import torch
    inner = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        inner[k] = max(5, math.ceil(window / _window(fn, 5)))
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(_window(fn, inner[k]))
    return {k: (statistics.median(v) * 1e6, inner[k]) for k, v in ts.items()}


def _mat(rows, cols):
    import torch
    from convnet_amd.matrix import Matrix
    m = Matrix()
    m.AllocateGPUMemory(rows, cols)
    m.tensor().normal_(generator=torch.Generator(device="cuda").manual_seed(rows + cols))
    return m


def _shape(name, r, c, reps, window):
    from convnet_amd._lib import lib
    from convnet_amd.matrix import Matrix
    rnd = ctypes.byref(Matrix._rnd)
    n = r * c
    x, d, noise, other = (_mat(r, c) for _ in range(4))
    X, D, N, O = (m.GetMat() for m in (x, d, noise, other))
    lib.fill_with_randn(rnd, N)                     # the backward sequence's stored noise
    lib.mult_by_scalar(N, STDDEV, N, 0.0)
    lib.add_scalar(N, 1.0, N)
    call_id = 7
    # (the arrays are rewritten in place call after call; no kernel here branches on a value, so what they drift to does not matter)
    us = _compare({
        "gaussian_dropout": lambda: lib.gaussian_dropout(rnd, X, STDDEV, MAX_ACT, 1, None),
        "unfused_forward": lambda: (lib.lower_bound_scalar(X, 0.0, X), lib.fill_with_randn(rnd, O), lib.mult_by_scalar(O, STDDEV, O, 0.0),
                                    lib.add_scalar(O, 1.0, O), lib.mult_elementwise(X, O, X, 0.0), lib.upper_bound_mod_scalar(X, MAX_ACT, X)),
        "gaussian_dropout_undo": lambda: lib.gaussian_dropout_undo(rnd, call_id, STDDEV, D, X, 1, 0),
        "unfused_backward": lambda: (lib.mult_elementwise(D, N, D, 0.0), lib.divide_elementwise(X, N, X),
                                     lib.apply_rectified_linear_deriv(D, X, D)),
        "relu_dropout": lambda: lib.relu_dropout(rnd, X, P, 1.0 / (1 - P)),
        "copy": lambda: lib.copy_on_device(X, O)}, reps, window)
    row = dict(shape=name, floats=n, MB=round(4e-6 * n, 1))
    for k, (t, inner) in us.items():
        b = BYTES_PER_ELEMENT[k]
        row[k] = dict(us=round(t, 2), bytes_per_element=b, GBps=round(b * n / t * 1e-3, 1), calls_per_window=inner)
    copy_rate, binary_rate = row["copy"]["GBps"], row["relu_dropout"]["GBps"]
    for k in ("gaussian_dropout", "gaussian_dropout_undo"):
        row[k]["rate_over_copy"] = round(row[k]["GBps"] / copy_rate, 3)
        row[k]["rate_over_relu_dropout"] = round(row[k]["GBps"] / binary_rate, 3)
        row[k]["bound"] = "memory" if row[k]["GBps"] >= MEMORY_BOUND_AT * copy_rate else "instruction issue"
    row["relu_dropout"]["rate_over_copy"] = round(binary_rate / copy_rate, 3)
    row["forward_fused_over_unfused"] = round(row["gaussian_dropout"]["us"] / row["unfused_forward"]["us"], 3)
    row["backward_fused_over_unfused"] = round(row["gaussian_dropout_undo"]["us"] / row["unfused_backward"]["us"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2, help="seconds a timed window should last")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussian_dropout_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "gaussian_dropout_bench needs an MI355X"
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(1)
    rows = [_shape(name, r, c, a.reps, a.window) for name, r, c in SHAPES]
    line = dict(tool="gaussian_dropout_bench", device=torch.cuda.get_device_name(0), reps=a.reps, window_s=a.window, memory_bound_at=MEMORY_BOUND_AT,
                shapes=rows,
                fused_pair_faster_at_both_shapes=all(r["forward_fused_over_unfused"] < 1.0 and r["backward_fused_over_unfused"] < 1.0 for r in rows))
    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
