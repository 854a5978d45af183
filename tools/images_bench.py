"""IMAGE_RAW streams on one MI355X: prints ONE JSON line and writes it to --out.  All legs run in this one process; kernels are timed with
HIP events, host work with a host clock (around a device synchronise where the device takes part); legs that are compared alternate
inside every rep.  The image files are synthetic PPMs of mixed sizes around 500 x 375, written into a temporary directory from a seed.

  (a) one AlexNet batch: N = 256 cases, raw_image_size 256, image_size 256, random 224 x 224 patch + flip, mean / std:
        images_u8     stage_images_u8 out of the decoded files at their original sizes: resample + crop + normalise + transpose
        patches_u8    stage_patches_u8 on the same crops resized on the host and kept as bytes (what an HDF5 byte dataset holds)
      both leave the same bits (checked first)
  (b) per chunk of --chunk files, on the host: DiskAccess of the images-once form (decode, copy, taps) against the float form's (decode,
      resize, crop, cast) — the chunk load with and without the host resize
  (c) bytes uploaded per chunk in both forms, with and without avg10_full_image (ten rows per file), counted from the handler's buffers
  (d) models.alexnet extraction (output layer, batch 256) in images/s from the PPM files — images-once and float form — beside the same
      from an HDF5 byte dataset of the 256 x 256 crops

    python tools/images_bench.py [--reps 20] [--chunk 256] [--files 512] [--out profiles/images_bench.json]
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

N, RAW, S, CROP = 256, 256, 256, 224
DIMS = 3 * S * S


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


def write_files(d, count, seed=1):
    """``count`` PPM files of mixed sizes and orientations around 500 x 375, the list file, a mean file; paths by name."""
    from convnet_amd import hdf5io
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(count):
        w, h = int(rng.integers(420, 581)), int(rng.integers(320, 431))
        if i % 4 == 3:
            w, h = h, w                                        # a portrait one in four
        # smooth content with some noise, so that the resample has something to average
        y, x = np.mgrid[0:h, 0:w]
        image = np.stack([(x * (3 + k) + y * (5 - k) + i * 17) % 256 for k in range(3)], axis=2) + rng.integers(0, 32, (h, w, 3))
        paths.append(os.path.join(d, f"im{i:05d}.ppm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h))
            f.write(np.clip(image, 0, 255).astype(np.uint8).tobytes())
    f = {"list": os.path.join(d, "list.txt"), "mean": os.path.join(d, "mean.h5"), "paths": paths}
    with open(f["list"], "w") as h:
        h.write("\n".join(paths) + "\n")
    with hdf5io.File(f["mean"], "w") as h:
        h.WriteHDF5CPU((rng.random(DIMS) * 255).astype(np.float32), 1, DIMS, "mean")
        h.WriteHDF5CPU(((rng.random(DIMS) + 0.5) * 60).astype(np.float32), 1, DIMS, "std")
    return f


def config(f, chunk, stream="", extra="", batch=N):
    from convnet_amd import pbtxt
    return pbtxt.parse(f'data_config {{ file_pattern: "{f["list"]}" layer_name: "input" data_type: IMAGE_RAW raw_image_size: {RAW} '
                       f'image_size: {S} gpu_image_size_y: {CROP} gpu_image_size_x: {CROP} {stream} }}\n'
                       f'batch_size: {batch}\nchunk_size: {chunk}\n{extra}\n', pbtxt.DatasetConfig)


def leg_a(args, f, out):
    import torch
    from convnet_amd import hdf5io
    from convnet_amd.datahandler import DataHandler
    from convnet_amd.matrix import Matrix
    dh = DataHandler(config(f, N))
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    dh.DiskAccess()
    half = dh.disk_.halves_["input"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    data, table, taps, cases = (dev(a) for a in half.Used(0))
    source_pixels = int(sum(int(w) * int(h) for _, w, h, _, _, _ in half.image_table_[0][:N].tolist()))
    dh.close()
    floats = DataHandler(config(f, N), raw_chunks=False)                # the same crops, resized on the host: kept as bytes
    crops = dev(np.asarray(floats.DiskAccess()["input"]).astype(np.uint8))
    floats.close()
    with hdf5io.File(f["mean"]) as h:
        mean_v, std_v = h.ReadHDF5CPU(DIMS, "mean"), h.ReadHDF5CPU(DIMS, "std")
    mean, std, index, wo, ho, fl, dst = (Matrix() for _ in range(7))
    for m, v in ((mean, mean_v), (std, std_v)):
        m.AllocateGPUMemory(DIMS, 1)
        m.FromNumpy(v)
    index.AllocateGPUMemory(1, N)
    index.FromNumpy(np.arange(N, dtype=np.float32))
    for m in (wo, ho, fl):
        m.AllocateGPUMemory(1, N)
        m.FillWithRand()
    wo.Mult(S - CROP + 1)
    ho.Mult(S - CROP + 1)
    dst.AllocateGPUMemory(N, 3 * CROP * CROP)

    def images_u8():
        Matrix.StageImagesU8(data, table, taps, cases, mean, std, dst, wo, ho, fl, S, S, CROP, CROP)

    def patches_u8():
        Matrix.StagePatchesU8(crops.view(-1), DIMS, N, index, mean, std, dst, wo, ho, fl, S, S, CROP, CROP)

    results = []
    for fn in (images_u8, patches_u8):
        fn()
        results.append(dst._t[:N * 3 * CROP * CROP].clone())
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32)), "the two legs leave different batches"
    legs = [("images_u8", images_u8), ("patches_u8", patches_u8), ("images_u8_again", images_u8)]
    times = {name: [] for name, _ in legs}
    for rep in range(args.reps + 2):
        for name, fn in legs:
            ms = _event_ms(fn)
            if rep >= 2:                                        # two warm-up reps of every leg
                times[name].append(ms * 1e3)
    pixels = N * 3 * CROP * CROP
    out["a_one_batch"] = {"N": N, "raw_image_size": RAW, "image_size": S, "patch": [CROP, CROP], "unit": "us", "legs_leave_the_same_bits": True,
                          "source_MB_of_the_batch": round(3 * source_pixels / 1e6, 1), "written_MB": round(4 * pixels / 1e6, 1),
                          "legs": {name: _stat(times[name], 1) for name, _ in legs}}
    # bytes the kernel cannot avoid: 4 B written and 8 B of mean / std per patch value; every source byte of the patch's footprint once
    for name in ("images_u8", "patches_u8"):
        leg = out["a_one_batch"]["legs"][name]
        leg["GBps_written_plus_mean_std"] = round(12 * pixels / leg["median"] / 1e3, 1)


def leg_b_c(args, f, out):
    from convnet_amd.datahandler import DataHandler
    leg = {"chunk_files": args.chunk, "unit": "ms", "disk_access": {}, "uploaded_MB_per_chunk": {}}
    for avg10 in (False, True):
        stream = "avg10_full_image: true" if avg10 else ""
        chunk = args.chunk * (10 if avg10 else 1)               # the same files either way: ten rows per file
        for name, raw in (("images_once", True), ("float", False)):
            dh = DataHandler(config(f, chunk, stream, batch=min(N, chunk)), raw_chunks=raw)
            dh.SetInputLayers(["input"])
            dh.AllocateHostMemory(pinned=False)
            ts = []
            for rep in range(args.disk_reps + 1):
                t0 = time.perf_counter()
                dh.DiskAccess()
                ts.append((time.perf_counter() - t0) * 1e3)
            half = dh.disk_.halves_["input"]
            if raw:
                nbytes = sum(a.nbytes for a in half.Used(0))
            else:
                nbytes = dh.host_[0]["input"].nbytes
            key = name + ("_avg10" if avg10 else "")
            leg["uploaded_MB_per_chunk"][key] = round(nbytes / 1e6, 2)
            leg["disk_access"][key] = _stat(ts[1:], 1)
            dh.close()
    out["b_c_per_chunk"] = leg


def leg_d(args, f, d, out):
    import torch
    from convnet_amd import hdf5io, models, pbtxt
    from convnet_amd import datahandler
    from convnet_amd.convnet import ConvNet
    files = len(f["paths"])
    # the HDF5 twin: the 256 x 256 crops as a byte dataset
    floats = datahandler.DataHandler(config(f, 0), raw_chunks=False)
    h5 = os.path.join(d, "crops.h5")
    with hdf5io.File(h5, "w") as h:
        h.WriteDataset("images", np.asarray(floats.DiskAccess()["input"]).astype(np.uint8))
    floats.close()
    image_input = f'data_config {{ file_pattern: "{f["list"]}" layer_name: "input" data_type: IMAGE_RAW raw_image_size: {RAW} image_size: {S} ' \
                  f'gpu_image_size_y: {CROP} gpu_image_size_x: {CROP} }}'
    h5_input = f'data_config {{ file_pattern: "{h5}" layer_name: "input" dataset_name: "images" image_size: {S} ' \
               f'gpu_image_size_y: {CROP} gpu_image_size_x: {CROP} }}'
    plain = datahandler.DataHandler
    legs = (("ppm_images_once", image_input, True), ("ppm_float", image_input, False), ("hdf5_bytes", h5_input, True))
    times = {name: [] for name, _, _ in legs}
    for rep in range(args.extract_reps + 1):
        for name, stream, raw in legs:
            cfg = pbtxt.parse(f'output_file: "{os.path.join(d, name + ".h5")}"\nfeature {{ layer: "output" }}\ninput {{\n{stream}\n'
                              f'batch_size: {N}\nchunk_size: {args.chunk}\npipeline_loads: true\n}}\n', pbtxt.FeatureExtractorConfig)
            net = ConvNet(models.alexnet(image_size=CROP), fused=True)
            datahandler.DataHandler = (lambda c, **kw: plain(c, **dict(kw, raw_chunks=raw)))
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                net.ExtractFeatures(cfg)
                torch.cuda.synchronize()
                if rep:                                         # the first round of every leg warms up
                    times[name].append(time.perf_counter() - t0)
            finally:
                datahandler.DataHandler = plain
            del net
    leg = {"model": "alexnet(image_size=224)", "batch": N, "files": files, "chunk_size": args.chunk, "unit": "s per pass (allocation included)",
           "legs": {}}
    for name, _, _ in legs:
        st = _stat(times[name])
        st["images_per_s"] = round(files / st["median"])
        leg["legs"][name] = st
    out["d_extraction"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--disk-reps", type=int, default=2)
    ap.add_argument("--extract-reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. 'd'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "images_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "images_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(7)
    out = {"tool": "images_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    with tempfile.TemporaryDirectory() as d:
        f = write_files(d, max(args.files, N))
        for name, leg in (("a", lambda: leg_a(args, f, out)), ("b", lambda: leg_b_c(args, f, out)), ("d", lambda: leg_d(args, f, d, out))):
            if name not in args.skip:
                leg()
                print(f"leg {name} done", file=sys.stderr, flush=True)
                with open(args.out, "w") as h:                  # (kept after every leg: a later leg that fails loses nothing)
                    h.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
