"""The optimizer steps on one MI355X (csrc/elementwise.hip): prints ONE JSON line and writes it to --out.

On the AlexNet parameter set — the weight and bias tensors of every edge of models.alexnet(), 13 + 3 tensors, as slices of flat
buffers laid out like the trainer's — the time of one whole step over all tensors (HIP events around it, median and spread of --reps):
  sgd             : sgd_momentum_step_multi, the yardstick                 (20 bytes per parameter)
  adagrad         : adagrad_momentum_step_multi                            (28 bytes per parameter: four reads, three needed writes)
  rmsprop         : rmsprop_momentum_step_multi                            (28 bytes per parameter)
  adagrad_unfused : the reference's call sequence, one library call each   (AdagradSGDOptimizer::Optimize, 9 passes per tensor)
  rmsprop_unfused : the reference's call sequence                          (RMSPropSGDOptimizer::Optimize, 8 passes per tensor)
with GB/s by the fused entry's own byte count (the unfused rows are priced by the same bytes: what the step NEEDS, not what they move).

    python tools/opt_bench.py [--reps 30] [--out profiles/opt_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

L2, CLIP, EPS, MOM = 0.0005, 0.0, 0.01, 0.9


def _tensors():
    """[(weights, bias) sizes] of the AlexNet edges and the flat total with the 128-float slice alignment."""
    from convnet_amd import models
    from convnet_amd.convnet import ConvNet
    from convnet_amd.edge import EdgeWithWeight
    net = ConvNet(models.alexnet())
    out, total = [], 0
    for e in net.edges_:
        if isinstance(e, EdgeWithWeight):
            n = e.GetParameterMemoryRequirement()
            rows, bias_cols, _ = e._param_layout()
            out.append((total, n - rows * bias_cols, rows * bias_cols))
            total += (n + 127) // 128 * 128
    return out, total


def _time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opt_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    layout, total = _tensors()
    rng = np.random.default_rng(0)
    flats = []
    for k in range(4):      # gradient, parameter, momentum history, second-moment history
        m = Matrix()
        m.AllocateGPUMemory(1, total)
        m.FromNumpy((1.0 + rng.random(total)).astype(np.float32) if k == 3 else rng.standard_normal(total).astype(np.float32) * 0.01)
        flats.append(m)
    tensors = []
    for off, nw, nb in layout:
        for start, n in ((off, nw), (off + nw, nb)):
            views = []
            for f in flats:
                v = Matrix()
                f.GetSlice(v, start, start + n)
                views.append(v)
            tensors.append(views)
    params = sum(t[0].GetNumEls() for t in tensors)
    G, W, H, A = range(4)

    def adagrad_unfused():
        for t in tensors:
            Matrix.AdagradUpdate(t[A], t[G], 1.0)
            t[G].Divide(t[A])
            t[G].Mult(2.0)
            t[G].Add(t[W], L2)
            t[G].Mult(EPS)
            t[H].Mult(MOM)
            t[H].Add(t[G])
            t[W].Add(t[H], -1)

    def rmsprop_unfused():
        for t in tensors:
            t[H].Mult(MOM)
            t[G].Add(t[W], L2)
            Matrix.RMSPropUpdate(t[A], t[G], 0.9)
            t[G].Divide(t[A])
            t[H].Add(t[G], EPS)
            t[W].Add(t[H], -1)

    sgd_items = [(t[G], t[W], t[H], L2, CLIP, EPS, MOM) for t in tensors]
    ada_items = [(t[G], t[W], t[H], t[A], 1.0, 2.0, L2, CLIP, EPS, MOM) for t in tensors]
    rms_items = [(t[G], t[W], t[H], t[A], 0.9, L2, CLIP, EPS, MOM) for t in tensors]
    legs = (("sgd", lambda: Matrix.SGDMomentumStepMulti(sgd_items), 20), ("adagrad", lambda: Matrix.AdagradMomentumStepMulti(ada_items), 28),
            ("rmsprop", lambda: Matrix.RMSPropMomentumStepMulti(rms_items), 28), ("adagrad_unfused", adagrad_unfused, 28),
            ("rmsprop_unfused", rmsprop_unfused, 28), ("sgd_again", lambda: Matrix.SGDMomentumStepMulti(sgd_items), 20))
    out = {"tool": "opt_bench", "device": torch.cuda.get_device_name(0), "tensors": len(tensors), "parameters": params, "reps": args.reps, "legs": {}}
    for name, fn, bytes_per in legs:
        med, lo, hi = _time(fn, args.reps)
        gbs = lambda us: round(bytes_per * params / us / 1e3, 1)   # noqa: E731
        out["legs"][name] = {"us": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1), "bytes_per_parameter": bytes_per,
                             "GBps": gbs(med), "GBps_min": gbs(hi), "GBps_max": gbs(lo)}
    L = out["legs"]
    out["adagrad_unfused_over_fused"] = round(L["adagrad_unfused"]["us"] / L["adagrad"]["us"], 2)
    out["rmsprop_unfused_over_fused"] = round(L["rmsprop_unfused"]["us"] / L["rmsprop"]["us"], 2)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
