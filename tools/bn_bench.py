"""Batch-normalisation kernels on one MI355X (csrc/batch_norm.hip): prints ONE JSON line and writes it to --out.

Per layer shape — every VGG-16-BN conv output at N = 128, the AlexNet conv1 / conv2 outputs at N = 256, an FC layer of 4096 units
at N = 32 / 128 / 256 — the time (HIP events around
the call, median of --reps) of
  fwd_stats : bn_fprop_act(train) minus bn_fprop_act(test)   (the statistics read and the finish launch)
  fwd_apply : bn_fprop_act(test), ReLU on                     (one read, one write)
  bwd       : bn_bprop_fused                                  (two reads for the sums, two reads and one write for the apply)
with the bytes each needs (4 per float per pass) and the fraction of 8 TB/s nominal HBM, and of the 6.3 TB/s a copy measures.
Then the whole training step of vgg_bn() against vgg() at N = 128, fused host, same call: ms/step and images/s.

    python tools/bn_bench.py [--reps 20] [--steps 5] [--out profiles/bn_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

NOMINAL, COPY = 8.0e12, 6.3e12


def _shapes():
    from convnet_amd import models
    from convnet_amd.convnet import ConvNet
    out = []
    for model, n, pick in ((models.vgg_bn(), 128, lambda l: l.UseBatchNormalization()),
                           (models.alexnet(), 256, lambda l: l.GetName() in ("hidden1_conv", "hidden2_conv"))):
        net = ConvNet(model)
        for l in net.layers_:
            if pick(l):
                out.append((f"{net.model_name_}:{l.GetName()}@N{n}", l.GetNumChannels(), n * l.GetSizeY() * l.GetSizeX()))
    # FC-shaped BN (short columns: one wave per column, 8-64 of its lanes busy)
    out += [(f"fc4096@N{n}", 4096, n) for n in (32, 128, 256)]
    return out


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
    return statistics.median(ts)


def _kernels(reps):
    import torch
    from convnet_amd.matrix import Matrix
    rows = []
    for name, C, H in _shapes():
        n = C * H
        x = Matrix()
        x.AllocateGPUMemory(H, C)
        d = Matrix()
        d.AllocateGPUMemory(H, C)
        g = torch.Generator(device="cuda").manual_seed(1)
        x.tensor().normal_(generator=g)
        d.tensor().normal_(generator=g)
        vec = []
        for v in (1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0):   # gamma beta mu sigma batch_mu batch_sigma dgamma dbeta
            m = Matrix()
            m.AllocateGPUMemory(1, C)
            m.Set(v)
            vec.append(m)
        gm, bt, mu, sg, bm, bs, dg, db = vec
        # the state is normalised again on every call: the forward stays on BN outputs (mean 0, std 1), never drifts
        t_train = _time(lambda: Matrix.BNFpropAct(x, gm, bt, mu, sg, bm, bs, 0.9, 1e-5, True, True), reps)
        t_test = _time(lambda: Matrix.BNFpropAct(x, gm, bt, mu, sg, bm, bs, 0.9, 1e-5, False, True), reps)
        t_bwd = _time(lambda: Matrix.BNBpropFused(d, x, gm, bt, bs, dg, db), reps)
        r = dict(layer=name, C=C, H=H, MB=round(4 * n / 2**20, 1))
        for k, t, passes in (("fwd_stats", t_train - t_test, 1), ("fwd_apply", t_test, 2), ("fwd", t_train, 3), ("bwd", t_bwd, 5)):
            b = 4.0 * n * passes
            r[k] = dict(us=round(t, 1), bytes=int(b), of_nominal=round(b / (t * 1e-6) / NOMINAL, 3) if t > 0 else None,
                        of_copy=round(b / (t * 1e-6) / COPY, 3) if t > 0 else None)
        rows.append(r)
        del x, d, vec
        torch.cuda.empty_cache()
    return rows


def _step(text, batch, steps):
    import torch
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import SyntheticDataHandler
    net = ConvNet(text, fused=True)
    net.SetBatchsize(batch)
    net.SetupDataset(SyntheticDataHandler(net, batch, seed=5, num_batches=1))
    net.AllocateMemory(False)
    for _ in range(2):
        net.TrainOneBatch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.TrainOneBatch()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    bn_bytes = sum(4.0 * batch * l.GetSizeY() * l.GetSizeX() * l.GetNumChannels() * 8 for l in net.layers_ if l.UseBatchNormalization())
    del net
    torch.cuda.empty_cache()
    return ms, bn_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bn_bench needs an MI355X"
    from convnet_amd import models
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    rows = _kernels(a.reps)
    big = [r for r in rows if r["MB"] >= 64]
    ms_bn, bn_bytes = _step(models.vgg_bn(), a.batch, a.steps)
    ms_plain, _ = _step(models.vgg(), a.batch, a.steps)
    bound_ms = bn_bytes / NOMINAL * 1e3
    line = dict(
        tool="bn_bench", device=torch.cuda.get_device_name(0), layers=rows,
        min_of_nominal_ge_64MB={k: min(r[k]["of_nominal"] for r in big) for k in ("fwd_stats", "fwd_apply", "bwd")} if big else None,
        vgg_step=dict(batch=a.batch, steps=a.steps, vgg_ms=round(ms_plain, 2), vgg_bn_ms=round(ms_bn, 2),
                      vgg_img_s=round(a.batch / ms_plain * 1e3, 1), vgg_bn_img_s=round(a.batch / ms_bn * 1e3, 1),
                      bn_overhead_ms=round(ms_bn - ms_plain, 2), bn_8pass_bound_ms=round(bound_ms, 2),
                      overhead_over_bound=round((ms_bn - ms_plain) / bound_ms, 2)))
    s = json.dumps(line)
    print(s)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
