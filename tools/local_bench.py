"""Locally connected layer kernels on one MI355X (csrc/local_conv.hip): prints ONE JSON line.

Per geometry and kernel (fprop, dgrad, wgrad) on both matrix paths: the time of the launch alone on the chip (HIP events around it, the
library's per-launch timer, median of `--reps`), algorithmic TFLOP/s, the bytes the kernel needs at least (bank once, activations /
derivatives once, the target twice when it is accumulated) and the fraction of its bound, bound = max(flops / peak, bytes / 6.3 TB/s)
with peak 416.7 TFLOP/s on path 1 (the split bf16 pipe) and 157.3 on path 0 (the fp32 instruction).  Beside it, as a same-call
yardstick: torch unfold + bmm in fp32 on the same GPU (fprop only).  Then the cifar_local training step at batch 128 on path 1:
images/s and the share of the step's kernel time spent in the local kernels.

    python tools/local_bench.py [--reps 10] [--out profiles/local_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

PEAK = {1: 416.7e12, 0: 157.3e12}
HBM = 6.3e12

GEOMS = {
    "cifar_local3_n128": dict(N=128, C=64, H=5, W=5, F=64, Ky=3, Kx=3, pady=1, padx=1),
    "cifar_local4_n128": dict(N=128, C=64, H=5, W=5, F=32, Ky=3, Kx=3, pady=1, padx=1),
    "face_n32": dict(N=32, C=16, H=63, W=63, F=16, Ky=9, Kx=9),
    "face_n128": dict(N=128, C=16, H=63, W=63, F=16, Ky=9, Kx=9),
    "face_n256": dict(N=256, C=16, H=63, W=63, F=16, Ky=9, Kx=9),
    "strided_n128": dict(N=128, C=16, H=25, W=25, F=16, Ky=7, Kx=7, sy=2, sx=2),
}


def _time_kernel(fn, reps):
    from convnet_amd import _lib
    fn()   # warm
    _lib.profile_report()
    ms = []
    for _ in range(reps):
        _lib.profile_enable(True)
        fn()
        _lib.profile_enable(False)
        rows = _lib.profile_report()
        ms.append(sum(r["ms"] for r in rows if r["kernel"].startswith("lc_kernel")))
    return statistics.median(ms)


def bench_geometry(g, reps):
    import ctypes

    import torch
    import torch.nn.functional as Fn
    from convnet_amd import _lib
    from hip_adapter import _desc, _w_local, _x, _y
    lib = _lib.lib
    rng = np.random.default_rng(0)
    x = rng.standard_normal(g.in_shape()).astype(np.float32)
    w = rng.standard_normal(g.bank_shape()).astype(np.float32)
    dy = rng.standard_normal(g.out_shape()).astype(np.float32)
    X, W, D = _x(g, x), _w_local(g, w), _y(g, dy)
    T, DX, DW = _y(g, np.zeros(g.out_shape())), _x(g, np.zeros(g.in_shape())), _w_local(g, np.zeros(g.bank_shape()))
    d = _desc(g)
    b = ctypes.byref
    calls = {
        "fprop": lambda: lib.localUpGemm(X.GetMat(), W.GetMat(), T.GetMat(), b(X.shape_), b(W.shape_), b(T.shape_), d, 0.0),
        "dgrad": lambda: lib.localDownGemm(D.GetMat(), W.GetMat(), DX.GetMat(), b(D.shape_), b(W.shape_), b(DX.shape_), d, 0.0),
        "wgrad": lambda: lib.localOutpGemm(X.GetMat(), D.GetMat(), DW.GetMat(), b(X.shape_), b(D.shape_), b(DW.shape_), d, 0.0, 1.0 / g.N),
    }
    act, out, bank = 4.0 * g.N * g.C * g.H * g.W, 4.0 * g.N * g.F * g.M, 4.0 * g.F * g.K * g.M
    need = {"fprop": bank + act + out, "dgrad": bank + out + act, "wgrad": act + out + bank}
    res = {"geom": {k: getattr(g, k) for k in ("N", "C", "H", "W", "F", "Ky", "Kx", "sy", "sx", "pady", "padx")},
           "modules": [g.My, g.Mx], "gflop": g.flops() / 1e9, "bank_mb": bank / 1e6}
    for path in (1, 0):
        lib.convnet_hip_set_matrix_path(path)
        for k, fn in calls.items():
            ms = _time_kernel(fn, reps)
            bound_s = max(g.flops() / PEAK[path], need[k] / HBM)
            res[f"{k}_p{path}"] = {"ms": round(ms, 4), "tflops": round(g.flops() / (ms * 1e-3) / 1e12, 2), "bytes": need[k],
                                   "bound_ms": round(bound_s * 1e3, 4), "frac_of_bound": round(bound_s / (ms * 1e-3), 3),
                                   "bound": "mfma" if g.flops() / PEAK[path] >= need[k] / HBM else "hbm"}
    lib.convnet_hip_set_matrix_path(1)
    # yardstick: torch unfold + bmm, fp32, same GPU
    xt = torch.from_numpy(x).cuda().permute(3, 0, 1, 2).contiguous()
    wt = torch.from_numpy(w).cuda().reshape(g.M, g.K, g.F)

    def torch_fprop():
        U = Fn.unfold(xt, (g.Ky, g.Kx), padding=(g.pady, g.padx), stride=(g.sy, g.sx))   # (N, K, M)
        return torch.bmm(U.permute(2, 0, 1), wt)

    for _ in range(2):
        torch_fprop()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        torch_fprop()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    tm = statistics.median(ts)
    res["torch_unfold_bmm_fprop_fp32"] = {"ms": round(tm, 4), "tflops": round(g.flops() / (tm * 1e-3) / 1e12, 2)}
    return res


def bench_cifar_local(steps=20, warmup=3):
    import torch
    from convnet_amd import _lib, models
    from test_net_gpu import build
    _lib.lib.convnet_hip_set_matrix_path(1)
    net = build(models.cifar_local(), 128, fused=True)
    for _ in range(warmup):
        net.TrainOneBatch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.TrainOneBatch()
    _lib.lib.cuda_sync_threads()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    _lib.profile_report()
    _lib.profile_enable(True)
    for _ in range(3):
        net.TrainOneBatch()
    _lib.profile_enable(False)
    rows = _lib.profile_report()
    tot = sum(r["ms"] for r in rows)
    loc = sum(r["ms"] for r in rows if r["kernel"].startswith("lc_kernel"))
    return {"batch": 128, "step_ms": round(dt * 1e3, 3), "images_per_s": round(128 / dt, 1),
            "local_share_of_kernel_time": round(loc / tot, 3) if tot else None,
            "local_ms_per_step": round(loc / 3, 4), "kernel_ms_per_step": round(tot / 3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    from local_ref import LocalGeom
    assert torch.cuda.is_available()
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(42)
    line = {"tool": "local_bench", "device": torch.cuda.get_device_name(0), "peaks_tflops": {"path1": 416.7, "path0": 157.3},
            "hbm_tbs": 6.3, "layers": {}}
    for name, kw in GEOMS.items():
        line["layers"][name] = bench_geometry(LocalGeom(**kw), a.reps)
    line["cifar_local_step"] = bench_cifar_local()
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
