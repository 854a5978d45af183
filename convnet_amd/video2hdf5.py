"""``python -m convnet_amd.video2hdf5 --input LIST --output OUT.h5 [--width 256] [--height 256] [--boundary FILE] [--labels FILE]
[--mean-file MEAN.h5] [--no-mirror] [--board 0] [--chunk 256] [--host]`` — apps/video2hdf5.cc over RawVideoFileIterator
(src/video_iterators.cc): a list of videos becomes the HDF5 dataset ``data`` of unsigned bytes, (frames, 3 * height * width): every frame
of every listed video, in list order and frame order, stretched to ``width`` x ``height`` (``image_iterators.ResizeTo``: resizeOCV
unconditionally, no aspect ratio kept, no crop) as planar R, G, B — the dataset a sequence stream (``is_sequence``, ``seq_length``,
``boundary_file``) trains from.  A video is a directory of frame files or a multi-frame image file (convnet_amd/video_iterators.py);
compressed video is refused by name.

The reference mirrors every frame (``flip_(true)``, :83,161), so the default does too and a dataset made here matches one made by the
reference's tool; ``--no-mirror`` writes the frames as they are (NOTES.md).  ``--boundary FILE`` writes one frame count per listed video,
one per line: the reference's ``num_frames_file`` (:100-118; its own tool passes no name and writes none) and the ``boundary_file`` a
sequence stream reads.  ``--labels FILE``: whitespace-separated integers, one per listed VIDEO, written as dataset ``labels``, int32
(frames, 1), every frame carrying its video's label: the row a ``pick_first`` label stream reads.

Two paths that write the same bytes.  The GPU path (the default): a chunk is ``--chunk`` frames and may span videos; a decode thread
decodes chunk k + 1 at the frames' original sizes into a pinned buffer while chunk k is on the GPU.  Per chunk: one upload, one
``resize_frames_u8`` per run of consecutive frames of equal (w, h) — normally one per chunk; the taps are built once per geometry —
an asynchronous copy into one of two pinned host buffers, and a writer thread that puts the rows into ``data`` under the libhdf5 lock.
``--mean-file MEAN.h5`` (GPU path): one ``chunk_moments_u8`` per chunk on the device-resident rows, then ``FinishMoments`` /
``WriteMeanFile``: bit for bit the file ``compute_mean`` computes from OUT.h5.  ``--host`` is the reference's loop with ``ResizeTo`` in
numpy: no GPU call."""
import argparse
import queue
import sys
import threading
import time

import numpy as np

from . import hdf5io, image_iterators, video_iterators
from .image2hdf5 import ReadLabels, SetupBoard, _Slot

NUM_COLORS = image_iterators.NUM_COLORS


def _progress(done, total, out):
    print(f"\rFrame {done} / {total}", end="", file=out, flush=True)


def _host_rows(reader, width, height, mirrored, chunk, data, out):
    """The reference's loop: decode, ResizeTo, mirror, planar — ``chunk`` rows per write."""
    size, dims = reader.GetDataSetSize(), NUM_COLORS * height * width
    rows = np.empty((min(chunk, size), dims), np.uint8)
    for start in range(0, size, chunk):
        frames = reader.Get(start, min(start + chunk, size))
        for i, frame in enumerate(frames):
            rows[i] = image_iterators.PlanarCrop(image_iterators.ResizeTo(frame, height, width), 0, 0, height, width, mirrored)
        data.WriteRows(rows[:len(frames)], start)
        _progress(start + len(frames), size, out)


def GeometryRuns(frames):
    """[(w, h, count)] of the runs of consecutive frames of equal size."""
    runs = []
    for f in frames:
        h, w = f.shape[:2]
        if runs and runs[-1][:2] == (w, h):
            runs[-1] = (w, h, runs[-1][2] + 1)
        else:
            runs.append((w, h, 1))
    return runs


class _DecodeSide:
    """All the decode thread touches: the reader, two pinned byte buffers that grow on demand, which of them the main thread has let go
    of, and a queue of (chunk, buffer number, bytes, runs) that ends with None or with the exception that stopped it."""

    def __init__(self, torch, reader, chunk):
        self.torch_, self.reader_, self.chunk_ = torch, reader, chunk
        self.buffers_ = [None, None]
        self.free_ = [threading.Event(), threading.Event()]
        for e in self.free_:
            e.set()
        self.stop_ = threading.Event()
        self.chunks_ = queue.Queue()

    def Run(self):
        try:
            size = self.reader_.GetDataSetSize()
            for k, start in enumerate(range(0, size, self.chunk_)):
                frames = self.reader_.Get(start, min(start + self.chunk_, size))
                num_bytes = sum(f.size for f in frames)
                while not self.free_[k % 2].wait(0.05):           # the upload out of this buffer is behind us
                    if self.stop_.is_set():
                        return
                self.free_[k % 2].clear()
                if self.buffers_[k % 2] is None or self.buffers_[k % 2].numel() < num_bytes:
                    self.buffers_[k % 2] = self.torch_.empty(num_bytes + num_bytes // 4, dtype=self.torch_.uint8, pin_memory=True)
                host, at = self.buffers_[k % 2].numpy(), 0
                for f in frames:
                    host[at:at + f.size] = f.reshape(-1)
                    at += f.size
                self.chunks_.put((k, k % 2, num_bytes, GeometryRuns(frames)))
            self.chunks_.put(None)
        except BaseException as e:                                # handed to the main thread
            self.chunks_.put(e)


def _gpu_rows(reader, width, height, mirrored, chunk, data, mean_file, out, info):
    import torch
    from .compute_mean import FinishMoments, WriteMeanFile
    from .datawriter import _WriterSide
    from .matrix import Matrix
    size, dims = reader.GetDataSetSize(), NUM_COLORS * height * width
    chunk = min(chunk, size)
    side, decode = _WriterSide(), _DecodeSide(torch, reader, chunk)
    writer = threading.Thread(target=side.Run, name="video2hdf5 writer", daemon=True)
    decoder = threading.Thread(target=decode.Run, name="video2hdf5 decoder", daemon=True)
    writer.start()
    decoder.start()

    def wait_free(slot):
        while not slot.free_.wait(0.05):
            if not writer.is_alive():
                raise RuntimeError("video2hdf5: the writer thread is gone while it holds a buffer")
        if side.error_ is not None:
            raise side.error_

    try:
        dev = Matrix()._dev()
        rows = torch.empty(chunk * dims, dtype=torch.uint8, device=dev)
        slots = [_Slot(torch, chunk, dims) for _ in range(2)]
        acc = torch.zeros(2 * dims + NUM_COLORS * NUM_COLORS, dtype=torch.int64, device=dev) if mean_file else None
        source, taps = None, {}
        while True:
            t0 = time.perf_counter()
            job = decode.chunks_.get()                            # (waits for this chunk's decode; the next one's starts behind it)
            info["load_wait_seconds"] += time.perf_counter() - t0
            if job is None:
                break
            if isinstance(job, BaseException):
                raise job
            k, which, num_bytes, runs = job
            if source is None or source.numel() < num_bytes:
                source = torch.empty(num_bytes + num_bytes // 4, dtype=torch.uint8, device=dev)
            source[:num_bytes].copy_(decode.buffers_[which][:num_bytes], non_blocking=True)
            at = valid = 0
            for w, h, count in runs:                              # one launch per run of equal geometry
                if (w, h) not in taps:
                    taps[w, h] = torch.from_numpy(np.concatenate(image_iterators.ImageTaps(w, h, width, height))).to(dev)
                Matrix.ResizeFramesU8(source[at:at + count * w * h * 3], count, h, w, taps[w, h],
                                      rows[valid * dims:(valid + count) * dims], height, width, mirrored)
                at += count * w * h * 3
                valid += count
                info["launches"] += 1
            frames = rows[:valid * dims]
            if acc is not None:
                Matrix.ChunkMomentsU8(frames, dims, valid, 0, valid, NUM_COLORS, acc)
            slot = slots[k % 2]
            wait_free(slot)                                       # the writer thread has let go of this host buffer
            slot.host_tensor_[:valid].copy_(frames.view(valid, dims), non_blocking=True)
            slot.copied_.record(torch.cuda.current_stream())
            slot.copied_.synchronize()                            # (the next chunk's decode is already running beside this)
            decode.free_[which].set()                             # the upload is behind that event too
            slot.free_.clear()
            side.jobs_.put((data, slot.host_[:valid], k * chunk, slot.free_))
            _progress(k * chunk + valid, size, out)
        for slot in slots:
            wait_free(slot)
        if acc is not None:
            stats = FinishMoments(acc.cpu().numpy().view(np.uint64), size, dims, NUM_COLORS)
            WriteMeanFile(mean_file, stats)
    finally:
        decode.stop_.set()
        side.jobs_.put(None)
        writer.join()
        decoder.join()
    if side.error_ is not None:
        raise side.error_


def Video2HDF5(input, output, width=256, height=256, boundary=None, labels=None, mean_file=None, mirror=True, board=None, chunk=256,
               host=False, out=None):
    """The command line as a function.  ``board=None``: the device is the caller's (``Matrix.SetupCUDADevice``); ``--host`` never looks at
    it.  Returns what the run did: ``videos``, ``frames``, ``dims``, ``path`` ("kernel" or "host"), ``chunks``, ``launches`` (GPU path:
    the resize launches, one per run of equal geometry inside a chunk), ``seconds`` and — GPU path — ``load_wait_seconds``, the time the
    main thread spent waiting for the decode thread."""
    out = out if out is not None else sys.stdout
    width, height, chunk = int(width), int(height), int(chunk)
    if width < 1:
        raise SystemExit(f"--width {width} is not a frame width.")
    if height < 1:
        raise SystemExit(f"--height {height} is not a frame height.")
    if chunk < 1:
        raise SystemExit(f"--chunk {chunk} is not a number of frames.")
    if host and mean_file:
        raise SystemExit("--mean-file is computed on the GPU path, beside the crops; with --host, run convnet_amd.compute_mean on the "
                         "output file instead.")
    videos = video_iterators.ReadVideoList(input)
    if not videos:
        raise SystemExit(f"{input} lists no video.")
    label_rows = ReadLabels(labels, len(videos)) if labels else None     # (before anything is written)
    reader = video_iterators.VideoReader(videos)                         # (the first pass: every refusal of a listed path)
    if board is not None and not host:
        SetupBoard(board, out)
    frames, dims = reader.GetDataSetSize(), NUM_COLORS * height * width
    info = {"videos": len(videos), "frames": frames, "dims": dims, "path": "host" if host else "kernel", "chunks": -(-frames // chunk),
            "launches": 0, "load_wait_seconds": 0.0, "mirrored": bool(mirror)}
    start = time.perf_counter()
    if boundary:
        with open(boundary, "w") as f:
            f.write("".join(f"{c}\n" for c in reader.counts_))
    with hdf5io.File(output, "w") as f:
        data = f.CreateRows("data", frames, dims, np.uint8)
        try:
            if host:
                _host_rows(reader, width, height, bool(mirror), chunk, data, out)
            else:
                _gpu_rows(reader, width, height, bool(mirror), chunk, data, mean_file, out, info)
        finally:
            print(file=out, flush=True)
            data.close()
        if label_rows is not None:
            f.WriteDataset("labels", np.repeat(label_rows, reader.counts_, axis=0))
    info["seconds"] = time.perf_counter() - start
    return info


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m convnet_amd.video2hdf5", description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", "-i", default="", help="File containing list of videos: frame directories or multi-frame image files.")
    ap.add_argument("--output", "-o", default="", help="Output hdf5 file.")
    ap.add_argument("--width", type=int, default=256, help="Every frame is stretched to this width.")
    ap.add_argument("--height", type=int, default=256, help="Every frame is stretched to this height.")
    ap.add_argument("--boundary", default="", help="also write the frame count of every video, one per line: a stream's boundary_file")
    ap.add_argument("--labels", default="", help="whitespace-separated integers, one per listed video: written per frame as dataset labels")
    ap.add_argument("--mean-file", default="", help="also write the statistics file of the dataset (GPU path)")
    ap.add_argument("--no-mirror", action="store_true", help="write the frames as they are (the reference's tool mirrors every frame)")
    ap.add_argument("--board", "-b", default="0", help="GPU board: 0, 1, ...")
    ap.add_argument("--chunk", type=int, default=256, help="frames decoded, resized and written together")
    ap.add_argument("--host", action="store_true", help="resize on the host with numpy: no GPU call")
    args = ap.parse_args(argv)
    if not args.input or not args.output:
        ap.print_help()
        return 1
    info = Video2HDF5(args.input, args.output, args.width, args.height, args.boundary or None, args.labels or None, args.mean_file or None,
                      not args.no_mirror, args.board, args.chunk, args.host)
    print(f"{info['frames']} frames of {info['videos']} videos, {info['dims']} bytes each, in {info['chunks']} chunks, "
          + ("mirrored as the reference's tool writes them" if info["mirrored"] else "not mirrored") + ": "
          + (f"{info['launches']} resize_frames_u8 launches on decoded frames" if info["path"] == "kernel" else "numpy resize on the host"))
    print(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
