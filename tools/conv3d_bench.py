"""Spatio-temporal (3-D) convolution and pooling on one MI355X (csrc/conv3d.hip): prints ONE JSON line.

Per geometry, direction (fprop, dgrad, wgrad) and matrix path: the kernel time of ONE call on the chip (HIP events around every launch,
the library's per-launch timer, summed over the call's launches; median of `--reps`) of
  * the 3-D entry of this library as it ships, and the same entry with its batched forms off (CONVNET_CONV3D_BATCH=0: no filter-bank
    preparation shared between frames, dW accumulated frame by frame), and
  * the reference's form — the loop of 2-D entries over frame slices, with its Scale pass for dgrad (cudamat_conv3d_gemm.cu) — on ANOTHER
    build of the library, given by --baseline-lib (a file name under convnet_amd/lib or a path; python -m convnet_amd.build --rev REV builds the
    parent commit's).  Each leg runs in a child process of this call (the library is chosen at import, CONVNET_HIP_LIB), so both are measured on
    the same GPU minutes apart; boxes differ by +-4 %, so only pairs of one call compare.
Then the pooling kernels over time (bytes needed / time against 6.3 TB/s) and the video_small training step at batch 32 on path 1
(images/s, share of kernel time per kernel family).

    python tools/conv3d_bench.py --baseline-lib libconvnet_hip_prev.so [--reps 7] [--out profiles/conv3d_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM = 6.3e12

GEOMS = {
    "c3d_56_c64_f128": dict(N=32, C=64, H=56, W=56, T=16, F=128, Ky=3, Kx=3, Kt=3, pady=1, padx=1),
    "c3d_56_c64_f128_st2": dict(N=32, C=64, H=56, W=56, T=16, F=128, Ky=3, Kx=3, Kt=3, st=2, pady=1, padx=1),
    "c3d_112_c3_f64": dict(N=32, C=3, H=112, W=112, T=16, F=64, Ky=3, Kx=3, Kt=3, pady=1, padx=1),
    "c3d_112_c3_f64_st2": dict(N=32, C=3, H=112, W=112, T=16, F=64, Ky=3, Kx=3, Kt=3, st=2, pady=1, padx=1),
}
POOLS = {
    "pool_56_c128_k3x3x2_s2": dict(N=32, C=128, H=56, W=56, T=14, F=128, Ky=3, Kx=3, Kt=2, sy=2, sx=2, st=2),
    "pool_28_c256_k2x2x2_s2": dict(N=32, C=256, H=28, W=28, T=8, F=256, Ky=2, Kx=2, Kt=2, sy=2, sx=2, st=2),
}


def _time_call(fn, reps):
    from convnet_amd import _lib
    fn()   # warm
    _lib.profile_report()
    ms, kernels = [], {}
    for _ in range(reps):
        _lib.profile_enable(True)
        fn()
        _lib.profile_enable(False)
        rows = _lib.profile_report()
        ms.append(sum(r["ms"] for r in rows))
        kernels = {}
        for r in rows:
            kernels[r["kernel"]] = kernels.get(r["kernel"], 0) + r["launches"]
    return round(statistics.median(ms), 4), kernels


def _setup():
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available()
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(42)


def leg(which, reps):
    """which = 'entry' (the 3-D entries of the loaded library) or 'loop' (the loop of its 2-D entries over frame slices)."""
    from conv3d_ref import Geom3D
    from convnet_amd import _lib
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _w, _x, _y
    from test_conv3d_gpu import _loop_2d
    _setup()
    out = {}
    rng = np.random.default_rng(0)
    for name, kw in GEOMS.items():
        g = Geom3D(**kw)
        X, W, DY = (_x(g, rng.standard_normal(g.in_shape(), np.float32)), _w(g, rng.standard_normal(g.filt_shape(), np.float32)),
                                   _y(g, rng.standard_normal(g.out_shape(), np.float32)))
        T, DX, DW = _y(g, np.zeros(g.out_shape(), np.float32)), _x(g, np.zeros(g.in_shape(), np.float32)), _w(g, np.zeros(g.filt_shape(), np.float32))
        d = _desc(g)
        if which == "entry":
            calls = {"fprop": lambda: Matrix.Conv3DUp(X, W, T, d, 0.0), "dgrad": lambda: Matrix.Conv3DDown(DY, W, DX, d, 0.0),
                     "wgrad": lambda: Matrix.Conv3DOutp(X, DY, DW, d, 0.0, 1.0 / g.N)}
        else:
            calls = {"fprop": lambda: _loop_2d(g, X, W, DY, "up", T, 0.0), "dgrad": lambda: _loop_2d(g, X, W, DY, "down", DX, 0.0),
                     "wgrad": lambda: _loop_2d(g, X, W, DY, "outp", DW, 0.0, 1.0 / g.N)}
        res = {}
        for path in (1, 0):
            _lib.lib.convnet_hip_set_matrix_path(path)
            for k, fn in calls.items():
                ms, kernels = _time_call(fn, reps)
                res[f"{k}_p{path}"] = {"ms": ms, "launches": kernels}
        _lib.lib.convnet_hip_set_matrix_path(1)
        out[name] = res
        del X, W, DY, T, DX, DW
    return out


def pools(reps):
    from conv3d_ref import Geom3D
    from convnet_amd.matrix import Matrix
    from hip_adapter import _desc, _x, _y
    rng = np.random.default_rng(1)
    out = {}
    for name, kw in POOLS.items():
        g = Geom3D(**kw)
        d = _desc(g, pool=True)
        X, DY = _x(g, rng.standard_normal(g.in_shape(), np.float32)), _y(g, rng.standard_normal(g.pooled_shape(), np.float32), pool=True)
        Y, DX = _y(g, np.zeros(g.pooled_shape(), np.float32), pool=True), _x(g, np.zeros(g.in_shape(), np.float32))
        Matrix.ConvMaxPool(X, Y, d)
        a, p = 4.0 * X.GetNumEls(), 4.0 * Y.GetNumEls()
        calls = {"max_fwd": (lambda: Matrix.ConvMaxPool(X, Y, d), a + p), "avg_fwd": (lambda: Matrix.ConvAvgPool(X, Y, d), a + p),
                 "max_undo": (lambda: Matrix.ConvMaxPoolUndo(X, DY, Y, DX, d, 0.0), 2 * a + 2 * p),
                 "avg_undo": (lambda: Matrix.ConvAvgPoolUndo(DY, DX, d, 0.0), a + p)}
        res = {}
        for k, (fn, need) in calls.items():
            ms, _ = _time_call(fn, reps)
            res[k] = {"ms": ms, "bytes": need, "tbs": round(need / (ms * 1e-3) / 1e12, 3), "frac_of_hbm": round(need / (ms * 1e-3) / HBM, 3)}
        out[name] = res
    return out


def video_small_step(steps=10, warmup=3):
    import torch
    from convnet_amd import _lib, models
    from test_conv3d_gpu import _build
    _lib.lib.convnet_hip_set_matrix_path(1)
    net = _build(models.video_small(), 32, fused=True)
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
    fam = {}
    for r in rows:
        fam[r["op"]] = fam.get(r["op"], 0.0) + r["ms"]
    return {"batch": 32, "step_ms": round(dt * 1e3, 3), "images_per_s": round(32 / dt, 1), "kernel_ms_per_step": round(tot / 3, 4),
            "share_of_kernel_time": {k: round(v / tot, 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])} if tot else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-lib", default=None, help="the library build that runs the loop-of-2-D-entries leg (CONVNET_HIP_LIB)")
    ap.add_argument("--leg", default=None, choices=["entry", "loop", "rest"], help="(internal) run one leg in this process and print its JSON")
    a = ap.parse_args()
    if a.leg in ("entry", "loop"):
        print("LEG " + json.dumps(leg(a.leg, a.reps)))
        return
    if a.leg == "rest":
        _setup()
        print("LEG " + json.dumps({"pooling_over_time": pools(a.reps), "video_small_step": video_small_step()}))
        return

    def child(which, lib=None, batch=None):
        env = dict(os.environ)
        env.pop("CONVNET_HIP_LIB", None)
        env.pop("CONVNET_CONV3D_BATCH", None)
        if lib:
            env["CONVNET_HIP_LIB"] = lib
        if batch is not None:
            env["CONVNET_CONV3D_BATCH"] = str(batch)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(a.reps)], env=env, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"leg {which} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][-1][4:])

    line = {"tool": "conv3d_bench", "hbm_tbs": 6.3, "baseline_lib": a.baseline_lib, "geoms": GEOMS, "pool_geoms": POOLS}
    entry = child("entry")
    unbatched = child("entry", batch=0)   # this library's entries as plain frame loops: no shared bank preparation, dW accumulated per frame
    loop = child("loop", a.baseline_lib) if a.baseline_lib else None
    line["conv3d"] = {}
    for name in GEOMS:
        line["conv3d"][name] = {}
        for k, v in entry[name].items():
            row = {"entry_ms": v["ms"], "entry_launches": v["launches"], "entry_unbatched_ms": unbatched[name][k]["ms"]}
            if loop:
                row["loop_on_baseline_ms"] = loop[name][k]["ms"]
                row["entry_over_loop"] = round(v["ms"] / loop[name][k]["ms"], 3)
            line["conv3d"][name][k] = row
    line.update(child("rest"))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
