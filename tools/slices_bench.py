"""Grouped convolutions through layer slices on one MI355X: prints ONE JSON line and writes it to --out.

models.alexnet_grouped() (conv2, conv4 and conv5 as two groups each, written with layer_slice / source_slice / dest_slice) beside
models.alexnet() at --batch images, fused host, same process:
  * the whole training step of either: ms/step and images/s;
  * per convolution edge of conv2..conv5 of either model — for the grouped model one row per group — which kernel its forward pass,
    its input gradient and its weight gradient went to and at what rate: the edge's own ComputeUp / ComputeDown / ComputeOuter on the
    net's (slice) matrices under the library's kernel timers (the mechanism of tests/gemm_launch_trace.py), --reps times; per pass the
    rows of the report {kernel, launches per call, us per call}, and the algorithmic TFLOP/s of the call over the sum of its kernels.
The per-group shapes (C = 48 / F = 128, C = 192 / F = 192, C = 192 / F = 128) may land on narrower kernels than the 256- and
384-filter layers of the ungrouped model do; this tool records what they land on, it tunes nothing.

    python tools/slices_bench.py [--batch 256] [--steps 10] [--reps 5] [--out profiles/slices_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)

LAYERS = ("hidden2_conv", "hidden3_conv", "hidden4_conv", "hidden5_conv")


def _build(text, batch):
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import SyntheticDataHandler
    net = ConvNet(text, fused=True)
    net.SetBatchsize(batch)
    net.SetupDataset(SyntheticDataHandler(net, batch, seed=5, num_batches=1))
    net.AllocateMemory(False)
    return net


def _step_ms(net, steps):
    import torch
    for _ in range(3):
        net.TrainOneBatch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.TrainOneBatch()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _profiled(fn, reps):
    """fn() reps times under the kernel timers: ([{kernel, launches, us}] per call, the call's algorithmic flops)."""
    import torch
    from convnet_amd import _lib
    fn()
    torch.cuda.synchronize()
    _lib.profile_report()
    _lib.profile_enable(True)
    try:
        for _ in range(reps):
            fn()
        rows = _lib.profile_report()
    finally:
        _lib.profile_enable(False)
    out = [dict(kernel=r["kernel"], launches=r["launches"] / reps, us=round(r["ms"] * 1e3 / reps, 1)) for r in rows]
    return out, sum(r["flops"] for r in rows) / reps


def _edge_passes(net, e, reps):
    src, dst = e.GetSource(), e.GetDest()
    s, d = e.GetSourceSliceName(), e.GetDestSliceName()
    relu = net.plan_[dst].fuse_relu

    def wgrad():
        e.ComputeOuter(src.GetState(s), dst.GetDeriv(d))
        e.num_grads_received_ = 0
    passes = {"fprop": lambda: e.ComputeUp(src.GetState(s), dst.GetState(d), True, True, fuse_relu=relu),
              "dgrad": lambda: e.ComputeDown(dst.GetDeriv(d), src.GetState(s), dst.GetState(d), src.GetDeriv(s), True,
                                             fuse_mask=net.plan_[src].down_scale),
              "wgrad": wgrad}
    c = e.conv_desc_
    row = dict(edge=e.GetName(), C=c.num_input_channels, F=c.num_output_channels, K=c.kernel_size_y, pixels=e.num_modules_y_ * e.num_modules_x_)
    for name, fn in passes.items():
        kernels, flops = _profiled(fn, reps)
        us = sum(k["us"] for k in kernels)
        row[name] = dict(kernels=kernels, us=round(us, 1), tflops=round(flops / (us * 1e-6) / 1e12, 1) if us > 0 else None)
    return row


def _model(text, batch, steps, reps):
    import torch
    from convnet_amd import models
    from convnet_amd.edge import ConvEdge
    net = _build(text, batch)
    ms = _step_ms(net, steps)
    edges = [_edge_passes(net, e, reps) for e in net.edges_ if isinstance(e, ConvEdge) and e.GetDest().GetName() in LAYERS]
    out = dict(ms_per_step=round(ms, 2), images_per_s=round(batch / ms * 1e3, 1), train_gmacs_per_image=round(models.count_macs(net)[1] / 1e9, 3),
               parameters=net.NumParameters(), conv_edges=edges)
    del net
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slices_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "slices_bench needs an MI355X"
    from convnet_amd import models
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    line = dict(tool="slices_bench", device=torch.cuda.get_device_name(0), batch=a.batch, steps=a.steps, reps=a.reps,
                alexnet=_model(models.alexnet(), a.batch, a.steps, a.reps),
                alexnet_grouped=_model(models.alexnet_grouped(), a.batch, a.steps, a.reps))
    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
