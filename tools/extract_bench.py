"""Feature extraction on one MI355X: prints ONE JSON line and writes it to --out.  All legs run in this one process; legs that are
compared alternate inside every rep.

  (a) models.alexnet() at batch 256 over an HDF5 file of --cases synthetic byte images (3 x 256 x 256, centre crop 224) written to a
      temporary directory, one feature stream per run: "hidden7" (4 096 dims) and "hidden5_conv" (43 264 dims).  Per stream:
        config_pipelined   ConvNet.ExtractFeatures(FeatureExtractorConfig): feature_rows + async copy + writer thread
        config_sync        the same with pipelined=False: every batch waited for and written on the main thread
        three_arg          the older ExtractFeatures(dataset, layer_names, output_file): synchronous copy of the whole state, host
                           transpose, every row held until the end
      Each is the WHOLE call on a host clock — handler construction, AllocateMemory(True) and the file's close included, the same
      set-up on every leg — so the images/s are end-to-end figures, not kernel rates.
  (b) feature_rows alone at (256, 4 096) and (256, 43 264), HIP events, --reps calls per leg cycling over enough distinct states that
      a 44 MB state is not served from the 256 MiB Infinity Cache (the 4 MB one is, whatever the cycle):
        passes1            group 1: state read, rows written                (8 B per element)
        passes10_add       a middle pass of ten: sum += state               (12 B per element)
        passes10_last      the last pass of ten: (sum + state) / 10 -> rows (12 B per element)
        group3             passes 1, average_online 3                       (4 B + 4/3 B per element)
      GB/s are those needed bytes over the event time.

    python tools/extract_bench.py [--cases 2048] [--rounds 3] [--reps 30] [--out profiles/extract_bench.json]
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
STREAMS = (("hidden7", 4096), ("hidden5_conv", 43264))


def _stat(ts, nd=3):
    return {"median": round(statistics.median(ts), nd), "min": round(min(ts), nd), "max": round(max(ts), nd), "n": len(ts)}


def _write_dataset(args, d):
    from convnet_amd import hdf5io
    rng = np.random.default_rng(3)
    path = os.path.join(d, "images.h5")
    with hdf5io.File(path, "w") as f:
        f.WriteDataset("images", rng.integers(0, 256, (args.cases, DIMS), dtype=np.uint8))
        f.WriteDataset("labels", rng.integers(0, 1000, args.cases).astype(np.int32))
    return (f'data_config {{\n  file_pattern: "{path}"\n  layer_name: "input"\n  dataset_name: "images"\n  image_size: {S}\n'
            f'  gpu_image_size_y: {CROP}\n  gpu_image_size_x: {CROP}\n}}\ndata_config {{\n  file_pattern: "{path}"\n  layer_name: "output"\n'
            f'  dataset_name: "labels"\n}}\nbatch_size: {N}\nchunk_size: {min(args.cases, 1024)}\npipeline_loads: true\n')


def leg_a(args, out):
    import torch
    from convnet_amd import models, pbtxt
    from convnet_amd.convnet import ConvNet
    with tempfile.TemporaryDirectory() as d:
        dataset_text = _write_dataset(args, d)

        def config(layer, path):
            return pbtxt.parse(f'output_file: "{path}"\nfeature {{ layer: "{layer}" }}\ninput {{\n{dataset_text}}}\n', pbtxt.FeatureExtractorConfig)

        def run(kind, layer, path):
            net = ConvNet(models.alexnet(), fused=True)
            if kind == "three_arg":
                dh = net._build_data_handler(pbtxt.parse(dataset_text, pbtxt.DatasetConfig))
                net.SetBatchsize(N)
                net.AllocateMemory(True)
                net.ExtractFeatures(dh, [layer], path)
                dh.close()
            else:
                net.ExtractFeatures(config(layer, path), pipelined=kind == "config_pipelined")

        kinds = ("config_pipelined", "config_sync", "three_arg")
        leg = {"model": "alexnet", "batch": N, "cases": args.cases, "unit": "s per whole call (set-up included)", "streams": {}}
        for layer, dims in STREAMS:
            times = {k: [] for k in kinds}
            for rep in range(args.rounds + 1):
                for k in kinds:
                    path = os.path.join(d, f"{layer}_{k}.h5")
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(k, layer, path)
                    torch.cuda.synchronize()
                    if rep >= 1:                          # one warm-up call of every leg
                        times[k].append(time.perf_counter() - t0)
                    os.remove(path)
            legs = {}
            for k in kinds:
                st = _stat(times[k])
                st["images_per_s"] = round(args.cases / st["median"])
                legs[k] = st
            leg["streams"][layer] = {"dims": dims, "file_MB": round(4e-6 * args.cases * dims, 1), "legs": legs}
        out["a_extraction"] = leg


def leg_b(args, out):
    import torch
    from convnet_amd.matrix import Matrix

    def event_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    leg = {"N": N, "unit": "us", "shapes": {}}
    for layer, D in STREAMS:
        count = max(2, -(-(300 << 20) // (4 * N * D)))       # distinct states: > 256 MiB in all where one state is big enough to matter
        count = min(count, 8)
        states = []
        for _ in range(count):
            m = Matrix()
            m.AllocateGPUMemory(N, D)
            m.FillWithRandn()
            states.append(m)
        sum_, rows, rows3, carry = Matrix(), Matrix(), Matrix(), Matrix()
        sum_.AllocateGPUMemory(N, D)
        sum_.Set(0.0)
        rows.AllocateGPUMemory(D, N)
        rows3.AllocateGPUMemory(D, (N + 2) // 3)
        carry.AllocateGPUMemory(D, 1)
        carry.Set(0.0)
        legs = [("passes1", lambda m: Matrix.FeatureRows(m, None, 0, 1, N, None, 0, 1, rows), 8.0),
                ("passes10_add", lambda m: Matrix.FeatureRows(m, sum_, 4, 10, N, None, 0, 1, rows), 12.0),
                ("passes10_last", lambda m: Matrix.FeatureRows(m, sum_, 9, 10, N, None, 0, 1, rows), 12.0),
                ("group3", lambda m: Matrix.FeatureRows(m, None, 0, 1, N, carry, 0, 3, rows3), 4.0 + 4.0 / 3)]
        times = {name: [] for name, _, _ in legs}
        for rep in range(args.reps + 3):
            for name, fn, _ in legs:
                us = event_us(lambda: fn(states[rep % count]))
                if rep >= 3:
                    times[name].append(us)
        shape = {"D": D, "distinct_states": count, "legs": {}}
        for name, _, bytes_per in legs:
            st = _stat(times[name], 1)
            st["bytes_per_element"] = round(bytes_per, 2)
            st["GBps_by_needed_bytes"] = round(bytes_per * N * D / st["median"] / 1e3, 1)
            shape["legs"][name] = st
        leg["shapes"][layer] = shape
        del states, sum_, rows, rows3, carry
        torch.cuda.empty_cache()
    out["b_feature_rows"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. 'a'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "extract_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    Matrix.InitRandom(7)
    out = {"tool": "extract_bench", "device": torch.cuda.get_device_name(0)}
    for name, leg in (("b", leg_b), ("a", leg_a)):
        if name not in args.skip:
            leg(args, out)
            print(f"leg {name} done", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
