"""jitter_raw_image on one MI355X: prints ONE JSON line and writes it to --out.  All legs run in this one process; kernels are timed with
HIP events after warm-up reps, host work with a host clock; legs that are compared alternate inside every rep; medians with their
ranges.  The image files are tools/images_bench.py's synthetic PPMs of mixed sizes around 500 x 375.

  (a) one AlexNet batch: N = 256 cases, raw_image_size 256, image_size 256, random 224 x 224 patch + flip, mean / std:
        jitter_rotated    stage_images_jitter_u8 under random_rotate_max_angle 15, min_scale 1.5: every image cropped, zoomed and rotated
        jitter_unrotated  the same entry's arm without the blend, under min_scale 1.5 alone: cropped and zoomed
        images_u8         stage_images_u8 on the same decoded buffers, no jitter_raw_image
  (b) per chunk of --chunk files, on the host: DiskAccess with and without jitter_raw_image in the images-once form (decode, copy, taps
      and rotation rows) and in the float form (decode, Transform / Resize, crop, cast)

    python tools/jitter_bench.py [--reps 20] [--chunk 256] [--out profiles/jitter_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
from images_bench import CROP, DIMS, N, S, _event_ms, _stat, config, write_files  # noqa: E402

ROTATED = "jitter_raw_image: true random_rotate_max_angle: 15 min_scale: 1.5"
UNROTATED = "jitter_raw_image: true min_scale: 1.5"


def leg_a(args, f, out):
    import torch
    from convnet_amd import hdf5io
    from convnet_amd.datahandler import DataHandler
    from convnet_amd.matrix import Matrix
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    tables = {}
    for name, stream in (("jitter_rotated", ROTATED), ("jitter_unrotated", UNROTATED), ("images_u8", "")):
        dh = DataHandler(config(f, N, stream))
        dh.SetInputLayers(["input"])
        dh.AllocateHostMemory(pinned=False)
        dh.DiskAccess()
        used = dh.disk_.halves_["input"].Used(0)
        tables[name] = [dev(a) for a in used]
        if name == "jitter_rotated":
            assert used[1][:, 7].all(), "every image of the rotated leg is rotated"
            out_sizes = used[1][:, 3:5]
        dh.close()
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
    tail = (mean, std, dst, wo, ho, fl, S, S, CROP, CROP)
    legs = [("jitter_rotated", lambda: Matrix.StageImagesJitterU8(*tables["jitter_rotated"], True, *tail)),
            ("images_u8", lambda: Matrix.StageImagesU8(*tables["images_u8"], *tail)),
            ("jitter_unrotated", lambda: Matrix.StageImagesJitterU8(*tables["jitter_unrotated"], False, *tail)),
            ("jitter_rotated_again", lambda: Matrix.StageImagesJitterU8(*tables["jitter_rotated"], True, *tail))]
    times = {name: [] for name, _ in legs}
    for rep in range(args.reps + 2):
        for name, fn in legs:
            ms = _event_ms(fn)
            if rep >= 2:                                        # two warm-up reps of every leg
                times[name].append(ms * 1e3)
    assert np.isfinite(dst.ToNumpy()).all()
    out["a_one_batch"] = {"N": N, "raw_image_size": S, "image_size": S, "patch": [CROP, CROP], "max_angle": 15, "min_scale": 1.5, "unit": "us",
                          "rotated_sizes": {"min": int(out_sizes.min()), "max": int(out_sizes.max())},
                          "legs": {name: _stat(times[name], 1) for name, _ in legs}}
    base = out["a_one_batch"]["legs"]["images_u8"]["median"]
    for name in ("jitter_rotated", "jitter_unrotated"):
        out["a_one_batch"]["legs"][name]["times_images_u8"] = round(out["a_one_batch"]["legs"][name]["median"] / base, 2)


def leg_b(args, f, out):
    from convnet_amd.datahandler import DataHandler
    leg = {"chunk_files": args.chunk, "unit": "ms", "disk_access": {}}
    for form, raw in (("images_once", True), ("float", False)):
        for name, stream in (("plain", ""), ("jitter", ROTATED)):
            dh = DataHandler(config(f, args.chunk, stream, batch=min(N, args.chunk)), raw_chunks=raw)
            dh.SetInputLayers(["input"])
            dh.AllocateHostMemory(pinned=False)
            ts = []
            for rep in range(args.disk_reps + 1):
                t0 = time.perf_counter()
                dh.DiskAccess()
                ts.append((time.perf_counter() - t0) * 1e3)
            leg["disk_access"][f"{form}_{name}"] = _stat(ts[1:], 1)           # the first load warms the file cache
            dh.close()
    out["b_per_chunk"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--disk-reps", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. 'b'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jitter_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "jitter_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(7)
    out = {"tool": "jitter_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    with tempfile.TemporaryDirectory() as d:
        f = write_files(d, max(args.chunk, N))
        for name, leg in (("a", lambda: leg_a(args, f, out)), ("b", lambda: leg_b(args, f, out))):
            if name not in args.skip:
                leg()
                print(f"leg {name} done", file=sys.stderr, flush=True)
                with open(args.out, "w") as h:                  # (kept after every leg: a later leg that fails loses nothing)
                    h.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
