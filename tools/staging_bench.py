"""Input staging from a byte chunk on one MI355X: prints ONE JSON line and writes it to --out.  All legs run in this one process, timed
with HIP events (a host clock around a device synchronise for the training windows), legs that are compared alternate inside every rep.

  (a) one batch of AlexNet's input (N = 256, 3 x 256 x 256 -> 224 x 224, random crop + flip) out of a resident chunk of --chunk cases:
        stage_u8_norm    stage_patches_u8 with mean / std                  (1 B read + 4 B written per patch pixel, + mean / std reads)
        stage_u8         stage_patches_u8, both NULL                       (5 B per patch pixel)
        extract_f32      extract_patches on the float chunk, the yardstick  (8 B per patch pixel; its normalisation was paid at load)
        extract_f32_again  the same leg once more: the spread of repeating one leg
      every rep takes the next 256 columns of the chunk, so no leg re-reads what the one before it left in the caches
  (b) upload of the whole chunk from pinned host memory, as bytes and as float
  (c) models.alexnet() training steps (bench.py's configuration of the net) fed by
        hdf5             DataHandler on an HDF5 file of 2 x --chunk synthetic byte images written to a temporary directory:
                         chunk_size --chunk, pipeline_loads, randomize_gpu, crop + flip, mean / std, bytes form
        hdf5_float       the same handler with raw_chunks=False: the reference's float chunk
        synthetic        SyntheticDataHandler (pre-staged batches: no input work inside the step)
      in alternating windows of --steps steps; "disk_ms_per_chunk" is the host time of the preload thread's DiskAccess for one chunk.

    python tools/staging_bench.py [--reps 20] [--steps 40] [--rounds 3] [--chunk 1280] [--out profiles/staging_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N, COLORS, S, CROP = 256, 3, 256, 224
DIMS = COLORS * S * S


def _stat(ts, nd=3):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd), "n": len(ts)}


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def leg_a(args, out):
    import torch
    from convnet_amd.matrix import Matrix
    cases = args.chunk
    gen = torch.Generator(device="cuda").manual_seed(1)
    chunk_u8 = torch.randint(0, 256, (cases * DIMS,), dtype=torch.uint8, device="cuda", generator=gen)
    chunk_f32 = Matrix()
    chunk_f32.AllocateGPUMemory(DIMS, cases)
    chunk_f32._t[:cases * DIMS].copy_(chunk_u8)          # the reference's cast (its Preprocess is paid once per chunk, not here)
    rng = np.random.default_rng(2)
    mean, std = Matrix(), Matrix()
    for m, v in ((mean, rng.random(DIMS) * 255), (std, (rng.random(DIMS) + 0.5) * 60)):
        m.AllocateGPUMemory(DIMS, 1)
        m.FromNumpy(v.astype(np.float32))
    index = Matrix()
    index.AllocateGPUMemory(1, cases)
    index.FromNumpy(np.arange(cases, dtype=np.float32))
    wo, ho, fl, dst = Matrix(), Matrix(), Matrix(), Matrix()
    for m in (wo, ho, fl):
        m.AllocateGPUMemory(1, N)
        m.FillWithRand()
    wo.Mult(S - CROP + 1)
    ho.Mult(S - CROP + 1)
    dst.AllocateGPUMemory(N, COLORS * CROP * CROP)
    idx_slice, img_slice = Matrix(), Matrix()

    def u8(norm):
        def run(start):
            index.GetSlice(idx_slice, start, start + N)
            Matrix.StagePatchesU8(chunk_u8, DIMS, cases, idx_slice, mean if norm else None, std if norm else None, dst, wo, ho, fl, S, S, CROP, CROP)
        return run

    def f32(start):
        chunk_f32.GetSlice(img_slice, start, start + N)
        Matrix.ExtractPatches(img_slice, dst, wo, ho, fl, S, S, CROP, CROP)

    legs = [("stage_u8_norm", u8(True), 5), ("stage_u8", u8(False), 5), ("extract_f32", f32, 8), ("extract_f32_again", f32, 8)]
    times = {name: [] for name, _, _ in legs}
    pos = 0
    for rep in range(args.reps + 2):
        for name, fn, _ in legs:
            start = (pos * N) % (cases - N + 1)
            pos += 1
            ms = _event_ms(lambda: fn(start))
            if rep >= 2:                                  # two warm-up reps of every leg
                times[name].append(ms * 1e3)
    pixels = N * COLORS * CROP * CROP
    out["a_one_batch"] = {"N": N, "image": [COLORS, S, S], "patch": [CROP, CROP], "chunk_cases": cases, "unit": "us", "legs": {}}
    for name, _, bytes_per in legs:
        st = _stat(times[name], 1)
        st["bytes_per_pixel"] = bytes_per
        st["GBps_by_needed_bytes"] = round(bytes_per * pixels / st["median"] / 1e3, 1)
        out["a_one_batch"]["legs"][name] = st
    del chunk_u8, chunk_f32
    torch.cuda.empty_cache()


def leg_b(args, out):
    import torch
    cases = args.chunk
    host_u8 = torch.empty(cases * DIMS, dtype=torch.uint8, pin_memory=True)
    host_f32 = torch.empty(cases * DIMS, dtype=torch.float32, pin_memory=True)
    host_u8.random_(0, 256)
    host_f32.copy_(host_u8)
    dev_u8 = torch.empty(cases * DIMS, dtype=torch.uint8, device="cuda")
    dev_f32 = torch.empty(cases * DIMS, dtype=torch.float32, device="cuda")
    times = {"bytes": [], "float": []}
    for rep in range(args.upload_reps + 1):
        for name, d, h in (("bytes", dev_u8, host_u8), ("float", dev_f32, host_f32)):
            ms = _event_ms(lambda: d.copy_(h, non_blocking=True))
            if rep >= 1:
                times[name].append(ms)
    out["b_chunk_upload"] = {"chunk_cases": cases, "unit": "ms", "legs": {}}
    for name, nbytes in (("bytes", cases * DIMS), ("float", 4 * cases * DIMS)):
        st = _stat(times[name])
        st["MB"] = round(nbytes / 1e6, 1)
        st["GBps"] = round(nbytes / st["median"] / 1e6, 1)
        out["b_chunk_upload"]["legs"][name] = st
    del dev_u8, dev_f32, host_u8, host_f32
    torch.cuda.empty_cache()


def _write_dataset(args, d):
    from convnet_amd import hdf5io
    rng = np.random.default_rng(3)
    total = 2 * args.chunk
    path, mean_path = os.path.join(d, "images.h5"), os.path.join(d, "mean.h5")
    images = rng.integers(0, 256, (total, DIMS), dtype=np.uint8)
    with hdf5io.File(path, "w") as f:
        f.WriteDataset("images", images)
        f.WriteDataset("labels", rng.integers(0, 1000, total).astype(np.int32))
    del images
    with hdf5io.File(mean_path, "w") as f:
        f.WriteHDF5CPU((rng.random(DIMS) * 255).astype(np.float32), 1, DIMS, "mean")
        f.WriteHDF5CPU(((rng.random(DIMS) + 0.5) * 60).astype(np.float32), 1, DIMS, "std")
    cfg = os.path.join(d, "train_data.pbtxt")
    with open(cfg, "w") as f:
        f.write(f'data_config {{\n  file_pattern: "{path}"\n  layer_name: "input"\n  dataset_name: "images"\n  image_size: {S}\n'
                f'  gpu_image_size_y: {CROP}\n  gpu_image_size_x: {CROP}\n  can_translate: true\n  can_flip: true\n  normalize: true\n'
                f'  mean_file: "{mean_path}"\n}}\ndata_config {{\n  file_pattern: "{path}"\n  layer_name: "output"\n  dataset_name: "labels"\n}}\n'
                f'batch_size: {N}\nchunk_size: {args.chunk}\npipeline_loads: true\nrandomize_gpu: true\n')
    return cfg


def leg_c(args, out):
    import torch
    from convnet_amd import models, pbtxt
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import DataHandler, SyntheticDataHandler
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        cfg = _write_dataset(args, d)
        write_s = time.perf_counter() - t0
        nets = {}
        for name in ("hdf5", "hdf5_float", "synthetic"):
            net = ConvNet(models.alexnet(), fused=True, overlap_wgrad=True)
            if name == "hdf5":
                net.SetupDataset(cfg)
            elif name == "hdf5_float":
                net.SetupDataset(DataHandler(pbtxt.read(cfg, pbtxt.DatasetConfig), raw_chunks=False))
            else:
                net.SetBatchsize(N)
                net.SetupDataset(SyntheticDataHandler(net, N, seed=1000, num_batches=2))
            net.AllocateMemory(False)
            nets[name] = net
        dh = nets["hdf5"].train_dataset_
        disk_ms = {}
        for name in ("hdf5", "hdf5_float"):
            def timed_disk_access(buf, inner=nets[name].train_dataset_.disk_.DiskAccess, log=disk_ms.setdefault(name, [])):
                t = time.perf_counter()                   # runs on the preload thread: host clock only
                r = inner(buf)
                log.append((time.perf_counter() - t) * 1e3)
                return r
            nets[name].train_dataset_.disk_.DiskAccess = timed_disk_access
        for net in nets.values():
            for _ in range(args.warmup):
                net.TrainOneBatch()
        torch.cuda.synchronize()
        times = {name: [] for name in nets}
        for _ in range(args.rounds):
            for name, net in nets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    net.TrainOneBatch()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        assert dh.streams_["input"].raw_ and not nets["hdf5_float"].train_dataset_.streams_["input"].raw_
        dh.close()
        nets["hdf5_float"].train_dataset_.close()
    leg = {"model": "alexnet", "batch": N, "steps_per_window": args.steps, "windows": args.rounds, "unit": "ms per step",
           "dataset": {"cases": 2 * args.chunk, "chunk_size": args.chunk, "batches_per_chunk": args.chunk // N, "write_s": round(write_s, 1)}, "legs": {}}
    for name in nets:
        st = _stat(times[name])
        st["images_per_s"] = round(N / st["median"] * 1e3)
        leg["legs"][name] = st
    leg["disk_ms_per_chunk"] = {name: _stat(ms, 1) for name, ms in disk_ms.items() if ms}
    for name in ("hdf5", "hdf5_float"):
        leg[name + "_over_synthetic"] = round(leg["legs"][name]["median"] / leg["legs"]["synthetic"]["median"], 3)
    out["c_training"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--upload-reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--chunk", type=int, default=1280)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. 'c'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "staging_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "staging_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(7)
    out = {"tool": "staging_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    for name, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
        if name not in args.skip:
            leg(args, out)
            print(f"leg {name} done", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
