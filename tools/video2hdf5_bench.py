"""video2hdf5 on one MI355X: prints ONE JSON line and writes it to --out.  All legs run in this one process; kernels are timed with HIP
events, host work with a host clock (around work that ends in a device synchronise or a closed file); legs that are compared alternate
inside every rep, after two warm-up reps of every leg.

  (a)  one chunk: 256 seeded random frames of 320 x 240 -> 256 x 256 (a mild resize: adjacent output rows share source rows), mirrored:
         resize_frames_u8   the frames of one geometry, taps and source rows staged in LDS
         crop_images_u8     the route that existed: a per-frame image table whose rows all point at one shared tap block, cases
                            {n, 0, 0, mirrored}
         device_copy        a device-to-device copy of the output's size: what moving those bytes costs with nothing else to do
       the two resize legs must leave the same bytes (checked before anything is timed)
  (a') the same legs from 640 x 480: downsizing by about 2x, where no source row is shared
  (b)  the whole tool on 16 directories of 32 binary PPM frames of 320 x 240, written into a temporary directory from a seed: the GPU
       path beside --host, which must write the same dataset (checked), and the share of the GPU path's time that its main thread
       spent waiting for the decode thread (load_wait_seconds)

    python tools/video2hdf5_bench.py [--reps 20] [--tool-reps 3] [--skip b] [--out profiles/video2hdf5_bench.json]
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

from images_bench import _event_ms, _stat  # noqa: E402

N, W, H = 256, 256, 256
DIMS = 3 * H * W


def leg_a(args, w, h, out, key):
    import torch
    from convnet_amd import image_iterators
    from convnet_amd.matrix import Matrix
    g = torch.Generator(device="cuda").manual_seed(11 + w)
    frames = torch.randint(0, 256, (N * h * w * 3,), dtype=torch.uint8, device="cuda", generator=g)
    taps = torch.from_numpy(np.concatenate(image_iterators.ImageTaps(w, h, W, H))).cuda()
    table = torch.tensor([[n * w * h * 3, w, h, W, H, 0] for n in range(N)], dtype=torch.int64, device="cuda")
    cases = torch.tensor([[n, 0, 0, 1] for n in range(N)], dtype=torch.int32, device="cuda")
    rows, other, copy = (torch.empty(N * DIMS, dtype=torch.uint8, device="cuda") for _ in range(3))
    resize = lambda: Matrix.ResizeFramesU8(frames, N, h, w, taps, rows, H, W, True)          # noqa: E731
    crop = lambda: Matrix.CropImagesU8(frames, table, taps, cases, other, H, W)              # noqa: E731
    resize()
    crop()
    torch.cuda.synchronize()
    assert torch.equal(rows, other), "resize_frames_u8 and crop_images_u8 leave different bytes"
    first = np.ascontiguousarray(frames[:h * w * 3].cpu().numpy().reshape(h, w, 3))
    want = image_iterators.PlanarCrop(image_iterators.ResizeTo(first, H, W), 0, 0, H, W, True)
    assert np.array_equal(rows[:DIMS].cpu().numpy(), want), "resize_frames_u8 and the host's ResizeTo leave different bytes"
    legs = [("resize_frames_u8", resize), ("crop_images_u8", crop), ("device_copy", lambda: copy.copy_(rows))]
    times = {name: [] for name, _ in legs}
    for rep in range(args.reps + 2):
        for name, fn in legs:
            ms = _event_ms(fn)
            if rep >= 2:                                        # two warm-up reps of every leg
                times[name].append(ms * 1e3)
    leg = {"frames": N, "from": [w, h], "to": [W, H], "mirrored": True, "unit": "us, kernel time by HIP events", "bytes_equal": True,
           "read_MB": round(N * w * h * 3 / 1e6, 1), "written_MB": round(N * DIMS / 1e6, 1),
           "legs": {name: _stat(times[name], 1) for name, _ in legs}}
    new, old = leg["legs"]["resize_frames_u8"], leg["legs"]["crop_images_u8"]
    leg["crop_over_resize"] = round(old["median"] / new["median"], 2)
    leg["resize_below_crop_by_more_than_crops_spread"] = bool(old["median"] - new["median"] > old["max"] - old["min"])
    out[key] = leg


def write_videos(d, videos=16, frames=32, w=320, h=240, seed=5):
    rng = np.random.default_rng(seed)
    names = []
    for v in range(videos):
        names.append(os.path.join(d, f"video_{v}"))
        os.mkdir(names[-1])
        for i in range(frames):
            with open(os.path.join(names[-1], f"frame_{i + 1}.ppm"), "wb") as f:
                f.write(b"P6\n%d %d\n255\n" % (w, h))
                f.write(rng.integers(0, 256, h * w * 3, dtype=np.uint8).tobytes())
    listing = os.path.join(d, "videos.txt")
    with open(listing, "w") as f:
        f.write("\n".join(names) + "\n")
    return listing, videos * frames


def _dataset(path):
    from convnet_amd import hdf5io
    with hdf5io.File(path) as h:
        r = h.RowReader("data")
        rows = np.empty((r.GetDataSetSize(), r.GetDims()), np.uint8)
        r.Get(rows, 0, len(rows))
        r.close()
    return rows


def leg_b(args, d, out):
    import torch
    from convnet_amd import video2hdf5
    listing, frames = write_videos(d)
    paths = {"gpu": os.path.join(d, "gpu.h5"), "host": os.path.join(d, "host.h5")}
    times, waits, launches = {"gpu": [], "host": []}, [], 0
    for rep in range(args.tool_reps + 1):
        for name in ("gpu", "host"):
            if name == "host" and rep > args.host_reps:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = video2hdf5.Video2HDF5(listing, paths[name], W, H, chunk=args.chunk, host=name == "host", out=io.StringIO())
            torch.cuda.synchronize()
            if rep:                                             # the first round of every leg warms up
                times[name].append(time.perf_counter() - t0)
                if name == "gpu":
                    waits.append(info["load_wait_seconds"])
                    launches = info["launches"]
        if rep == 0:
            assert np.array_equal(_dataset(paths["gpu"]), _dataset(paths["host"])), "the GPU path and --host wrote different datasets"
    leg = {"videos": 16, "frames": frames, "chunk": args.chunk, "from": [320, 240], "to": [W, H], "launches": launches,
           "unit": "s per run, tool wall time (allocation and file creation included)", "datasets_equal": True, "legs": {}}
    for name in ("gpu", "host"):
        st = _stat(times[name])
        st["frames_per_s"] = round(frames / st["median"])
        leg["legs"][name] = st
    leg["wait_for_decode"] = _stat(waits)
    leg["decode_share_of_gpu_run"] = round(_stat(waits)["median"] / leg["legs"]["gpu"]["median"], 3)
    out["b_whole_tool"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tool-reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. 'b'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video2hdf5_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "video2hdf5_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    out = {"tool": "video2hdf5_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps}
    with tempfile.TemporaryDirectory() as d:
        for name, leg in (("a", lambda: leg_a(args, 320, 240, out, "a_mild_resize")), ("a'", lambda: leg_a(args, 640, 480, out, "a_prime_downsize")),
                          ("b", lambda: leg_b(args, d, out))):
            if name not in args.skip.split(","):
                leg()
                print(f"leg {name} done", file=sys.stderr, flush=True)
                with open(args.out, "w") as h:                  # (kept after every leg: a later leg that fails loses nothing)
                    h.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
