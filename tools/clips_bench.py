"""Clip staging from a frame dataset on one MI355X: prints ONE JSON line and writes it to --out.  All legs run in this one process, timed
with HIP events (a host clock for the preload thread's work and, around a device synchronise, for the training windows); legs that are
compared alternate inside every rep.

  (a) one batch of N = 32 clips of T = 16 frames, 3 x 128 x 128 -> 112 x 112, random crop + flip, mean / std, out of a resident chunk of
      --chunk consecutive clips:
        clips_u8             stage_clips_u8 on the frames-once buffer, a block stages all 16 planes of its tile  (5 + 8/T B per patch pixel)
        clips_u8_plane       the same entry with one plane per block                                              (13 B)
        patches_u8_mat       stage_patches_u8 on the MATERIALISED byte clips: frames as colours, mean / std tiled (13 B)
        extract_f32_mat      extract_patches on the materialised float clips, the reference's form                (8 B; normalised at load)
        patches_u8_mat_again the third leg once more: the spread of repeating one leg
      every rep takes the next 32 clips of the chunk
  (b) per chunk of --chunk clips: the upload from pinned host memory of the frames-once bytes, the materialised bytes and the
      materialised floats (the device holds the same bytes), and the host time of DiskAccess — what the preload thread does — for the
      frames-once form against the float form's materialised host cast, from an HDF5 file
  (c) models.video_small(image_size=112) training steps at batch 32 from an HDF5 frame file (chunk_size --chunk, pipeline_loads,
      randomize_gpu, crop + flip, mean / std): the frames-once form, the float form (raw_chunks=False) and SyntheticDataHandler in
      alternating windows of --steps steps

    python tools/clips_bench.py [--reps 20] [--steps 40] [--rounds 5] [--chunk 640] [--out profiles/clips_bench.json]
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

N, T, COLORS, S, CROP = 32, 16, 3, 128, 112
FS = COLORS * S * S


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


def _colvec(Matrix, v):
    m = Matrix()
    m.AllocateGPUMemory(v.size, 1)
    m.FromNumpy(v.astype(np.float32))
    return m


def leg_a(args, out):
    import torch
    from convnet_amd._lib import lib
    from convnet_amd.matrix import Matrix
    clips, frames = args.chunk, args.chunk + T - 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    once = torch.randint(0, 256, (frames, FS), dtype=torch.uint8, device="cuda", generator=gen)
    mat_u8 = torch.empty((clips, T * FS), dtype=torch.uint8, device="cuda")        # clip i = frames i .. i + T - 1, concatenated
    for t in range(T):
        mat_u8[:, t * FS:(t + 1) * FS] = once[t:t + clips]
    rng = np.random.default_rng(2)
    mean_v, std_v = rng.random(FS) * 255, (rng.random(FS) + 0.5) * 60
    mean, std = _colvec(Matrix, mean_v), _colvec(Matrix, std_v)
    mean_t, std_t = _colvec(Matrix, np.tile(mean_v, T)), _colvec(Matrix, np.tile(std_v, T))
    mat_f32 = Matrix()
    mat_f32.AllocateGPUMemory(T * FS, clips)
    mat_f32._t[:clips * T * FS].copy_(mat_u8.view(-1))       # the reference's cast and its Preprocess, paid once per chunk
    mat_f32.AddColVec(mean_t, -1)
    mat_f32.DivideByColVec(std_t)
    index = Matrix()
    index.AllocateGPUMemory(1, clips)
    index.FromNumpy(np.arange(clips, dtype=np.float32))       # clip i starts at buffer column i, and is column i of the materialised chunks
    wo, ho, fl, dst = Matrix(), Matrix(), Matrix(), Matrix()
    for m in (wo, ho, fl):
        m.AllocateGPUMemory(1, N)
        m.FillWithRand()
    wo.Mult(S - CROP + 1)
    ho.Mult(S - CROP + 1)
    dst.AllocateGPUMemory(N, T * COLORS * CROP * CROP)
    idx_slice, img_slice = Matrix(), Matrix()

    def clips_u8(grid):
        def run(start):
            lib.convnet_hip_set_stage_clips_grid(grid)
            index.GetSlice(idx_slice, start, start + N)
            Matrix.StageClipsU8(once.view(-1), FS, frames, idx_slice, T, mean, std, dst, wo, ho, fl, S, S, CROP, CROP)
            lib.convnet_hip_set_stage_clips_grid(0)
        return run

    def patches_u8(start):
        index.GetSlice(idx_slice, start, start + N)
        Matrix.StagePatchesU8(mat_u8.view(-1), T * FS, clips, idx_slice, mean_t, std_t, dst, wo, ho, fl, S, S, CROP, CROP)

    def extract_f32(start):
        mat_f32.GetSlice(img_slice, start, start + N)
        Matrix.ExtractPatches(img_slice, dst, wo, ho, fl, S, S, CROP, CROP)

    # the results first: the legs that are timed against each other leave the same batch, bit for bit
    results = []
    for fn in (clips_u8(1), clips_u8(2), patches_u8, extract_f32):
        fn(N)
        results.append(dst._t[:N * T * COLORS * CROP * CROP].clone())
    same = [bool(torch.equal(results[0].view(torch.int32), r.view(torch.int32))) for r in results[1:]]
    assert all(same), same

    legs = [("clips_u8", clips_u8(1), 5 + 8 / T), ("clips_u8_plane", clips_u8(2), 13), ("patches_u8_mat", patches_u8, 13),
            ("extract_f32_mat", extract_f32, 8), ("patches_u8_mat_again", patches_u8, 13)]
    times = {name: [] for name, _, _ in legs}
    pos = 0
    for rep in range(args.reps + 2):
        for name, fn, _ in legs:
            start = (pos * N) % (clips - N + 1)
            pos += 1
            ms = _event_ms(lambda: fn(start))
            if rep >= 2:                                  # two warm-up reps of every leg
                times[name].append(ms * 1e3)
    pixels = N * T * COLORS * CROP * CROP
    out["a_one_batch"] = {"N": N, "clip_frames": T, "frame": [COLORS, S, S], "patch": [CROP, CROP], "chunk_clips": clips, "unit": "us",
                          "legs_leave_the_same_bits": True, "legs": {}}
    for name, _, bytes_per in legs:
        st = _stat(times[name], 1)
        st["bytes_per_pixel"] = bytes_per
        st["GBps_by_needed_bytes"] = round(bytes_per * pixels / st["median"] / 1e3, 1)
        out["a_one_batch"]["legs"][name] = st
    del once, mat_u8, mat_f32, results
    torch.cuda.empty_cache()


def _write_dataset(args, d, sequences=2):
    """``sequences`` sequences of chunk + T - 1 frames: ``sequences * chunk`` clips."""
    from convnet_amd import hdf5io
    rng = np.random.default_rng(3)
    per = args.chunk + T - 1
    total = sequences * per
    path, mean_path, bounds = os.path.join(d, "frames.h5"), os.path.join(d, "mean.h5"), os.path.join(d, "bounds.txt")
    with hdf5io.File(path, "w") as f:
        f.WriteDataset("frames", rng.integers(0, 256, (total, FS), dtype=np.uint8))
        f.WriteDataset("labels", rng.integers(0, 10, total).astype(np.int32))
    with hdf5io.File(mean_path, "w") as f:
        f.WriteHDF5CPU((rng.random(FS) * 255).astype(np.float32), 1, FS, "mean")
        f.WriteHDF5CPU(((rng.random(FS) + 0.5) * 60).astype(np.float32), 1, FS, "std")
    with open(bounds, "w") as f:
        f.write("\n".join([str(per)] * sequences) + "\n")
    cfg = os.path.join(d, "clips.pbtxt")
    seq = f'is_sequence: true\n  seq_length: {T}\n  boundary_file: "{bounds}"'
    with open(cfg, "w") as f:
        f.write(f'data_config {{\n  file_pattern: "{path}"\n  layer_name: "input"\n  dataset_name: "frames"\n  image_size: {S}\n'
                f'  gpu_image_size_y: {CROP}\n  gpu_image_size_x: {CROP}\n  can_translate: true\n  can_flip: true\n  normalize: true\n'
                f'  mean_file: "{mean_path}"\n  {seq}\n}}\ndata_config {{\n  file_pattern: "{path}"\n  layer_name: "output"\n'
                f'  dataset_name: "labels"\n  {seq}\n  pick_first: true\n}}\n'
                f'batch_size: {N}\nchunk_size: {args.chunk}\npipeline_loads: true\nrandomize_gpu: true\n')
    return cfg


def leg_b(args, out):
    import torch
    from convnet_amd import pbtxt
    from convnet_amd.datahandler import DataHandler
    clips, frames = args.chunk, args.chunk + T - 1
    forms = (("frames_once_bytes", frames * FS, torch.uint8), ("materialised_bytes", clips * T * FS, torch.uint8),
             ("materialised_float", clips * T * FS, torch.float32))
    leg = {"chunk_clips": clips, "unit": "ms", "upload": {}, "disk_access": {}}
    for name, count, dtype in forms:                       # one form at a time: the float one is 4 T times the first
        host = torch.empty(count, dtype=dtype, pin_memory=True)
        host.random_(0, 256)
        dev = torch.empty(count, dtype=dtype, device="cuda")
        ts = [_event_ms(lambda: dev.copy_(host, non_blocking=True)) for _ in range(args.upload_reps + 1)][1:]
        st = _stat(ts)
        nbytes = count * host.element_size()
        st["MB_uploaded_and_held"] = round(nbytes / 1e6, 1)
        st["GBps"] = round(nbytes / st["median"] / 1e6, 1)
        leg["upload"][name] = st
        del host, dev
        torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as d:
        cfg = pbtxt.read(_write_dataset(args, d), pbtxt.DatasetConfig)
        cfg.pipeline_loads = False
        for name, raw in (("frames_once_bytes", True), ("materialised_float", False)):
            dh = DataHandler(cfg, raw_chunks=raw)
            dh.SetInputLayers(["input"])
            dh.AllocateHostMemory(pinned=False)
            assert dh.streams_["input"].frames_once_ is raw
            ts = []
            for rep in range(args.disk_reps + 1):
                t0 = time.perf_counter()
                dh.DiskAccess()
                ts.append((time.perf_counter() - t0) * 1e3)
            st = _stat(ts[1:], 1)
            st["host_buffer_MB"] = round(dh.host_[0]["input"].nbytes / 1e6, 1)
            st["reads_per_chunk"] = dh.streams_["input"].reader_.num_reads_ // (args.disk_reps + 1)
            leg["disk_access"][name] = st
            dh.close()
            del dh
    out["b_per_chunk"] = leg


def leg_c(args, out):
    import torch
    from convnet_amd import models, pbtxt
    from convnet_amd.convnet import ConvNet
    from convnet_amd.datahandler import DataHandler, SyntheticDataHandler
    with tempfile.TemporaryDirectory() as d:
        cfg = _write_dataset(args, d)
        nets = {}
        for name in ("hdf5_frames_once", "hdf5_float", "synthetic"):
            net = ConvNet(models.video_small(image_size=CROP, frames=T), fused=True)
            if name == "hdf5_frames_once":
                net.SetupDataset(cfg)
            elif name == "hdf5_float":
                net.SetupDataset(DataHandler(pbtxt.read(cfg, pbtxt.DatasetConfig), raw_chunks=False))
                net.train_dataset_.SetInputLayers(["input"])
            else:
                net.SetBatchsize(N)
                net.SetupDataset(SyntheticDataHandler(net, N, seed=1000, num_batches=2))
            net.AllocateMemory(False)
            nets[name] = net
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
        assert nets["hdf5_frames_once"].train_dataset_.streams_["input"].frames_once_
        assert not nets["hdf5_float"].train_dataset_.streams_["input"].raw_
        for name in ("hdf5_frames_once", "hdf5_float"):
            nets[name].train_dataset_.close()
    leg = {"model": "video_small(image_size=112)", "batch": N, "clip_frames": T, "steps_per_window": args.steps, "windows": args.rounds,
           "unit": "ms per step", "dataset": {"clips": 2 * args.chunk, "chunk_size": args.chunk, "batches_per_chunk": args.chunk // N},
           "legs": {}}
    for name in nets:
        st = _stat(times[name])
        st["clips_per_s"] = round(N / st["median"] * 1e3)
        leg["legs"][name] = st
    for name in ("hdf5_frames_once", "hdf5_float"):
        leg[name + "_over_synthetic"] = round(leg["legs"][name]["median"] / leg["legs"]["synthetic"]["median"], 3)
    out["c_training"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--upload-reps", type=int, default=5)
    ap.add_argument("--disk-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=640)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. 'c'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clips_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "clips_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(7)
    out = {"tool": "clips_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    for name, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
        if name not in args.skip:
            leg(args, out)
            print(f"leg {name} done", file=sys.stderr, flush=True)
            with open(args.out, "w") as f:                # (kept after every leg: a later leg that fails loses nothing)
                f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
