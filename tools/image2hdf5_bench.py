"""image2hdf5 on one MI355X: prints ONE JSON line and writes it to --out.  All legs run in this one process; kernels are timed with HIP
events, host work with a host clock (around work that ends in a device synchronise or a closed file); legs that are compared alternate
inside every rep.  The image files are tools/images_bench.py's: synthetic PPMs of mixed sizes around 500 x 375, written into a temporary
directory from a seed.

  (a) one chunk: N = 256 cases, resize 256, crop 256, out of the decoded files at their original sizes:
        crop_images_u8    resample + crop + planar split into 256 x 196 608 stored bytes
        stage_images_u8   the same buffers into a normalised float batch of random 224 x 224 patches (what a training step stages)
        device_copy       a device-to-device copy of the output's size: what moving those bytes costs with nothing else to do
      crop_images_u8's bytes are checked first against the host's numpy resize of the same files
  (b) the whole tool over --files files, in images/s: the GPU path and --host, which must write the same dataset (checked)
  (c) the GPU path's decode: the host time of the chunk loads alone (DiskAccess of the images-once form, every chunk of the list once)
      over the GPU path's whole time, beside the time the tool itself spent waiting for its preload thread

    python tools/image2hdf5_bench.py [--reps 20] [--tool-reps 3] [--chunk 256] [--files 512] [--out profiles/image2hdf5_bench.json]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from images_bench import CROP, DIMS, N, RAW, S, _event_ms, _stat, config, write_files  # noqa: E402


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
    dh.close()
    floats = DataHandler(config(f, N), raw_chunks=False)                # the same crops, resized on the host
    want = np.asarray(floats.DiskAccess()["input"]).astype(np.uint8)
    floats.close()
    rows, copy = torch.empty(N * DIMS, dtype=torch.uint8, device="cuda"), torch.empty(N * DIMS, dtype=torch.uint8, device="cuda")
    Matrix.CropImagesU8(data, table, taps, cases, rows, S, S)
    assert np.array_equal(rows.cpu().numpy().reshape(N, DIMS), want), "crop_images_u8 and the host resize leave different bytes"
    with hdf5io.File(f["mean"]) as h:
        mean_v, std_v = h.ReadHDF5CPU(DIMS, "mean"), h.ReadHDF5CPU(DIMS, "std")
    mean, std, wo, ho, fl, dst = (Matrix() for _ in range(6))
    for m, v in ((mean, mean_v), (std, std_v)):
        m.AllocateGPUMemory(DIMS, 1)
        m.FromNumpy(v)
    for m in (wo, ho, fl):
        m.AllocateGPUMemory(1, N)
        m.FillWithRand()
    wo.Mult(S - CROP + 1)
    ho.Mult(S - CROP + 1)
    dst.AllocateGPUMemory(N, 3 * CROP * CROP)
    legs = [("crop_images_u8", lambda: Matrix.CropImagesU8(data, table, taps, cases, rows, S, S)),
            ("stage_images_u8", lambda: Matrix.StageImagesU8(data, table, taps, cases, mean, std, dst, wo, ho, fl, S, S, CROP, CROP)),
            ("device_copy", lambda: copy.copy_(rows)),
            ("crop_images_u8_again", lambda: Matrix.CropImagesU8(data, table, taps, cases, rows, S, S))]
    times = {name: [] for name, _ in legs}
    for rep in range(args.reps + 2):
        for name, fn in legs:
            ms = _event_ms(fn)
            if rep >= 2:                                        # two warm-up reps of every leg
                times[name].append(ms * 1e3)
    leg = {"N": N, "resize": RAW, "crop": S, "stage_images_u8_patch": [CROP, CROP], "unit": "us", "bytes_equal_the_host_resize": True,
           "written_MB": round(N * DIMS / 1e6, 1), "legs": {name: _stat(times[name], 1) for name, _ in legs}}
    for name in ("crop_images_u8", "device_copy"):
        leg["legs"][name]["GBps_written"] = round(N * DIMS / leg["legs"][name]["median"] / 1e3, 1)
    out["a_one_chunk"] = leg


def _dataset(path):
    from convnet_amd import hdf5io
    with hdf5io.File(path) as h:
        r = h.RowReader("data")
        rows = np.empty((r.GetDataSetSize(), r.GetDims()), np.uint8)
        r.Get(rows, 0, len(rows))
        r.close()
    return rows


def leg_b_c(args, f, d, out):
    import torch
    from convnet_amd import image2hdf5
    from convnet_amd.datahandler import DataHandler
    files = len(f["paths"])
    paths = {"gpu": os.path.join(d, "gpu.h5"), "host": os.path.join(d, "host.h5")}
    times, waits = {"gpu": [], "host": []}, []
    for rep in range(args.tool_reps + 1):
        for name in ("gpu", "host"):
            if name == "host" and rep > args.host_reps:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = image2hdf5.Image2HDF5(f["list"], paths[name], S, RAW, chunk=args.chunk, host=name == "host", out=io.StringIO())
            torch.cuda.synchronize()
            if rep:                                             # the first round of every leg warms up
                times[name].append(time.perf_counter() - t0)
                if name == "gpu":
                    waits.append(info["load_wait_seconds"])
        if rep == 0:
            assert np.array_equal(_dataset(paths["gpu"]), _dataset(paths["host"])), "the GPU path and --host wrote different datasets"
    leg = {"files": files, "chunk": args.chunk, "resize": RAW, "crop": S, "unit": "s per run (allocation and file creation included)",
           "datasets_equal": True, "legs": {}}
    for name in ("gpu", "host"):
        st = _stat(times[name])
        st["images_per_s"] = round(files / st["median"])
        leg["legs"][name] = st
    out["b_whole_tool"] = leg
    # (c) the chunk loads alone, as the preload thread runs them
    dh = DataHandler(image2hdf5.ImageStreamConfig(f["list"], S, RAW, args.chunk))
    dh.SetInputLayers([image2hdf5.LAYER])
    dh.AllocateHostMemory(pinned=False)
    chunks = -(-files // args.chunk)
    ts = []
    for rep in range(args.disk_reps + 1):
        dh.Seek(0)
        t0 = time.perf_counter()
        for _ in range(chunks):
            dh.DiskAccess()
        ts.append(time.perf_counter() - t0)
    dh.close()
    decode, whole = _stat(ts[1:]), leg["legs"]["gpu"]["median"]
    out["c_decode_share"] = {"unit": "s", "chunk_loads_alone": decode, "tool_wait_for_preload": _stat(waits),
                             "decode_over_whole_gpu_run": round(decode["median"] / whole, 3),
                             "wait_over_whole_gpu_run": round(_stat(waits)["median"] / whole, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tool-reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--disk-reps", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. 'b'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image2hdf5_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "image2hdf5_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(7)
    out = {"tool": "image2hdf5_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    with tempfile.TemporaryDirectory() as d:
        f = write_files(d, max(args.files, N))
        for name, leg in (("a", lambda: leg_a(args, f, out)), ("b", lambda: leg_b_c(args, f, d, out))):
            if name not in args.skip:
                leg()
                print(f"leg {name} done", file=sys.stderr, flush=True)
                with open(args.out, "w") as h:                  # (kept after every leg: a later leg that fails loses nothing)
                    h.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
