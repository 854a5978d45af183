"""Dataset moments of one AlexNet-shaped byte chunk (3 x 256 x 256, --chunk cases: staging_bench's chunk) on one MI355X: prints ONE JSON
line and writes it to --out.  All legs run in this one process and alternate inside every rep, timed with HIP events:

  kernel        chunk_moments_u8 on the resident byte chunk, the whole chunk in one call (what compute_mean does per chunk)
  copy          a device-to-device copy of the same bytes (bytes copied per second: the yardstick the kernel's rate stands beside)
  float_upload  the float form of the chunk from pinned host memory to the device (4 x the bytes; the byte path never pays it)
  float_seq     the reference's op sequence on the resident float chunk, in pieces of 256 cases: transpose, Add, Reshape + Dot, Mult, Add
  byte_upload   the byte chunk from pinned host memory, for scale: a pass over a dataset cannot run faster than it is uploaded

    python tools/moments_bench.py [--reps 10] [--chunk 1280] [--out profiles/moments_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)

N, COLORS, S = 256, 3, 256
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=1280)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_bench.json"))
    args = ap.parse_args()
    import torch
    from convnet_amd.compute_mean import _FloatSums
    from convnet_amd.matrix import Matrix
    assert torch.cuda.is_available(), "moments_bench needs the GPU: nothing here is measured without one"
    Matrix.SetupCUDADevice(0)
    cases, nbytes = args.chunk, args.chunk * DIMS
    host_u8 = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    host_u8.random_(0, 256)
    host_f32 = torch.empty(nbytes, dtype=torch.float32, pin_memory=True)
    host_f32.copy_(host_u8)
    chunk_u8 = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    other_u8 = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    chunk_f32 = Matrix()
    chunk_f32.AllocateGPUMemory(DIMS, cases)
    acc = torch.zeros(2 * DIMS + COLORS * COLORS, dtype=torch.int64, device="cuda")
    sums = _FloatSums(Matrix, DIMS, COLORS, cases)
    piece = Matrix()

    def stage(start, end, state):
        chunk_f32.GetSlice(piece, start, end)
        piece.CopyTranspose(state)

    def float_seq():
        for start in range(0, cases, N):
            sums.Add(stage, start, min(start + N, cases))

    legs = [("byte_upload", lambda: chunk_u8.copy_(host_u8, non_blocking=True)),
            ("kernel", lambda: Matrix.ChunkMomentsU8(chunk_u8, DIMS, cases, 0, cases, COLORS, acc)),
            ("copy", lambda: other_u8.copy_(chunk_u8)),
            ("float_upload", lambda: chunk_f32._t[:nbytes].copy_(host_f32, non_blocking=True)),
            ("float_seq", float_seq)]
    times = {name: [] for name, _ in legs}
    for rep in range(args.reps + 2):
        for name, fn in legs:
            ms = _event_ms(fn)
            if rep >= 2:                                  # two warm-up reps of every leg
                times[name].append(ms)
    # the kernel's sums after reps + 2 calls are (reps + 2) x the chunk's: check one of them against torch on the device
    want = int(chunk_u8.view(cases, DIMS)[:, 0].to(torch.int64).sum().item()) * (args.reps + 2)
    assert int(acc[0].item()) == want, (int(acc[0].item()), want)
    out = {"tool": "moments_bench", "device": torch.cuda.get_device_name(0), "reps": args.reps, "chunk_cases": cases,
           "image": [COLORS, S, S], "chunk_MB": round(nbytes / 1e6, 1), "unit": "ms", "legs": {}}
    for name, _ in legs:
        st = _stat(times[name])
        moved = 4 * nbytes if name == "float_upload" else nbytes
        st["GBps_of_chunk_bytes" if name != "float_upload" else "GBps"] = round(moved / st["median"] / 1e6, 1)
        out["legs"][name] = st
    med = {name: out["legs"][name]["median"] for name, _ in legs}
    out["kernel_over_copy"] = round(med["kernel"] / med["copy"], 3)
    out["float_seq_over_kernel"] = round(med["float_seq"] / med["kernel"], 2)
    out["float_path_over_byte_path_with_uploads"] = round((med["float_seq"] + med["float_upload"]) / (med["kernel"] + med["byte_upload"]), 2)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
