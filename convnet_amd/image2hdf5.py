"""``python -m convnet_amd.image2hdf5 --input LIST --output OUT.h5 [--crop 256] [--resize 256] [--board 0] [--chunk 256] [--labels FILE]
[--mean-file MEAN.h5] [--host]`` — apps/image2hdf5.cc: a list of image files becomes the HDF5 dataset ``data`` of unsigned bytes,
(files, 3 * crop * crop), in file order: every image resized so that it covers ``resize`` x ``resize`` (``Resize``) and its centre
``crop`` x ``crop`` patch as planar R, G, B — the dataset the byte form of the data handler trains from.

Two paths that write the same bytes.  The GPU path (the default) is a ``DataHandler`` client, as ``compute_mean`` is: an ``IMAGE_RAW``
stream built here (``image_size`` crop, ``raw_image_size`` resize, ``chunk_size`` chunk, ``parallel_disk_access``, nothing randomised)
takes the images-once form, so the preload thread decodes every file of a chunk once at its original size and the bytes and tables go
up together.  Per chunk: ONE ``crop_images_u8`` over the chunk's valid cases into a device byte buffer (resize, crop and planar split),
an asynchronous copy into one of two pinned host buffers, and a writer thread that puts the rows into ``data`` under the libhdf5 lock;
chunk k's download and write run beside chunk k + 1's decode.  A last chunk wraps to the first files behind its valid part: those cases
are not counted.  ``--host`` is the reference's loop with the package's numpy resize (``image_iterators.Resize``, ``PlanarCrop``): no
GPU call; the comparison leg, and the way on a machine without a GPU.

``--labels FILE``: whitespace-separated integers, one per listed file, written as dataset ``labels``, int32 (files, 1) (the reference
writes none — NOTES.md).  ``--mean-file MEAN.h5`` (GPU path): one ``chunk_moments_u8`` per chunk on the device-resident rows, then
``FinishMoments`` / ``WriteMeanFile``: bit for bit the file ``compute_mean`` computes from OUT.h5, whose moments are the same exact
integers."""
import argparse
import sys
import threading
import time

import numpy as np

from . import hdf5io, image_iterators, pbtxt

LAYER = "input"
NUM_COLORS = image_iterators.NUM_COLORS


def ReadLabels(path, num_files):
    """One integer per listed file, as int32 (files, 1)."""
    try:
        with open(path) as f:
            labels = [int(w) for w in f.read().split()]
    except (OSError, UnicodeDecodeError, ValueError) as e:
        raise SystemExit(f"Could not read labels file : {path} ({e})")
    if len(labels) != num_files:
        raise SystemExit(f"{path} holds {len(labels)} labels for {num_files} listed files.")
    return np.asarray(labels, np.int32).reshape(-1, 1)


def ImageStreamConfig(file_list, crop, resize, chunk):
    """The DatasetConfig the GPU path reads through: one IMAGE_RAW stream, rows in file order."""
    dsc = pbtxt.DataStreamConfig()
    dsc.file_pattern, dsc.layer_name, dsc.data_type = file_list, LAYER, "IMAGE_RAW"
    dsc.image_size, dsc.raw_image_size, dsc.num_colors = int(crop), int(resize), NUM_COLORS
    dsc.parallel_disk_access = True
    cfg = pbtxt.DatasetConfig()
    cfg.data_config.append(dsc)
    cfg.batch_size, cfg.chunk_size, cfg.pipeline_loads = 1, int(chunk), True
    return cfg


def _progress(done, total, out):
    print(f"\rImage {done} / {total}", end="", file=out, flush=True)


def _host_rows(files, crop, resize, chunk, data, out):
    """The reference's loop: decode, Resize, the centre crop, planar — ``chunk`` rows per write."""
    dims = NUM_COLORS * crop * crop
    rows = np.empty((min(chunk, len(files)), dims), np.uint8)
    for i, name in enumerate(files):
        _progress(i + 1, len(files), out)
        image = image_iterators.Resize(image_iterators.ReadImage(name), resize, resize)
        left, top, mirrored = image_iterators.Coordinates(image.shape[1], image.shape[0], 0, crop, crop)
        at = i % len(rows)
        rows[at] = image_iterators.PlanarCrop(image, left, top, crop, crop, mirrored)
        if at + 1 == len(rows) or i + 1 == len(files):
            data.WriteRows(rows[:at + 1], i - at)


class _Slot:
    """One of the two pinned host buffers, the event behind the copy into it, and whether the writer thread has let go of it."""

    def __init__(self, torch, max_rows, dims):
        self.host_tensor_ = torch.empty((max_rows, dims), dtype=torch.uint8, pin_memory=True)
        self.host_ = self.host_tensor_.numpy()
        self.copied_ = torch.cuda.Event()
        self.free_ = threading.Event()
        self.free_.set()


def _gpu_rows(file_list, crop, resize, chunk, data, mean_file, out, info):
    import torch
    from .compute_mean import FinishMoments, WriteMeanFile
    from .datahandler import DataHandler
    from .datawriter import _WriterSide
    from .matrix import Matrix
    dims = NUM_COLORS * crop * crop
    dh = DataHandler(ImageStreamConfig(file_list, crop, resize, chunk))
    side = _WriterSide()
    thread = threading.Thread(target=side.Run, name="image2hdf5 writer", daemon=True)
    thread.start()

    def wait_free(slot):
        while not slot.free_.wait(0.05):
            if not thread.is_alive():
                raise RuntimeError("image2hdf5: the writer thread is gone while it holds a buffer")
        if side.error_ is not None:
            raise side.error_

    try:
        st = dh.streams_[LAYER]
        size, chunk = dh.GetDataSetSize(), dh.chunk_size_
        dh.SetInputLayers([LAYER])
        dh.AllocateMemory()
        form = st.form_
        dev = Matrix()._dev()
        rows = torch.empty(chunk * dims, dtype=torch.uint8, device=dev)
        slots = [_Slot(torch, chunk, dims) for _ in range(2)]
        acc = torch.zeros(2 * dims + NUM_COLORS * NUM_COLORS, dtype=torch.int64, device=dev) if mean_file else None
        for k, valid in dh.ChunkPass():                # (waits for this chunk's decode, starts the next one's)
            info["load_wait_seconds"] = dh.pass_wait_seconds_
            crops = rows[:valid * dims]
            Matrix.CropImagesU8(*form.Cases(0, valid), crops, crop, crop)
            if acc is not None:
                Matrix.ChunkMomentsU8(crops, dims, valid, 0, valid, NUM_COLORS, acc)
            slot = slots[k % 2]
            wait_free(slot)                            # the writer thread has let go of this host buffer
            slot.host_tensor_[:valid].copy_(crops.view(valid, dims), non_blocking=True)
            slot.copied_.record(torch.cuda.current_stream())
            slot.copied_.synchronize()                 # (the next chunk's decode is already running beside this)
            slot.free_.clear()
            side.jobs_.put((data, slot.host_[:valid], k * chunk, slot.free_))
            _progress(k * chunk + valid, size, out)
        for slot in slots:
            wait_free(slot)
        if acc is not None:
            stats = FinishMoments(acc.cpu().numpy().view(np.uint64), size, dims, NUM_COLORS)
            WriteMeanFile(mean_file, stats)
    finally:
        side.jobs_.put(None)
        thread.join()
        dh.close()
    if side.error_ is not None:
        raise side.error_


def SetupBoard(board, out=None):
    """``--board`` as the other tools take it: one board digit; several boards are refused in their words."""
    from .train_convnet import ParseBoardIds
    boards = ParseBoardIds(str(board))
    if len(boards) > 1:
        raise SystemExit(f"--board {board}: {len(boards)} boards ask for a model-parallel net, which is not built; name one board.")
    from .matrix import Matrix
    Matrix.SetupCUDADevice(boards[0])
    print(f"Using board {boards[0]}", file=out if out is not None else sys.stdout)


def Image2HDF5(input, output, crop=256, resize=256, board=None, chunk=256, labels=None, mean_file=None, host=False, out=None):
    """The command line as a function.  ``board=None``: the device is the caller's (``Matrix.SetupCUDADevice``); ``--host`` never looks at
    it.  Returns what the run did: ``files``, ``dims``, ``path`` ("kernel" or "host"), ``chunks``, ``seconds`` and — GPU path —
    ``load_wait_seconds``, the time the main thread spent waiting for the preload thread's decode and queueing the upload."""
    out = out if out is not None else sys.stdout
    crop, resize, chunk = int(crop), int(resize), int(chunk)
    if crop > resize:
        raise SystemExit("Crop size cannot be bigger than the resized image.")
    if crop < 1:
        raise SystemExit(f"--crop {crop} is not an image size.")
    if chunk < 1:
        raise SystemExit(f"--chunk {chunk} is not a number of images.")
    if host and mean_file:
        raise SystemExit("--mean-file is computed on the GPU path, beside the crops; with --host, run convnet_amd.compute_mean on the "
                         "output file instead.")
    files = image_iterators.ReadFileList(input)
    if not files:
        raise SystemExit(f"{input} lists no image file.")
    label_rows = ReadLabels(labels, len(files)) if labels else None      # (before anything is written)
    if board is not None and not host:
        SetupBoard(board, out)
    dims = NUM_COLORS * crop * crop
    info = {"files": len(files), "dims": dims, "path": "host" if host else "kernel", "chunks": -(-len(files) // chunk),
            "load_wait_seconds": 0.0}
    start = time.perf_counter()
    with hdf5io.File(output, "w") as f:
        data = f.CreateRows("data", len(files), dims, np.uint8)
        try:
            if host:
                _host_rows(files, crop, resize, chunk, data, out)
            else:
                _gpu_rows(input, crop, resize, chunk, data, mean_file, out, info)
        finally:
            print(file=out, flush=True)
            data.close()
        if label_rows is not None:
            f.WriteDataset("labels", label_rows)
    info["seconds"] = time.perf_counter() - start
    return info


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m convnet_amd.image2hdf5", description=__doc__.split("\n\n")[0])
    ap.add_argument("--input", "-i", default="", help="File containing list of images.")
    ap.add_argument("--output", "-o", default="", help="Output hdf5 file.")
    ap.add_argument("--crop", "-c", type=int, default=256, help="After resize, crop a central patch of this size.")
    ap.add_argument("--resize", "-s", type=int, default=256, help="Resize each image so that the shorter side is equal to this size.")
    ap.add_argument("--board", "-b", default="0", help="GPU board: 0, 1, ...")
    ap.add_argument("--chunk", type=int, default=256, help="images decoded, cropped and written together")
    ap.add_argument("--labels", default="", help="whitespace-separated integers, one per listed file: written as dataset labels")
    ap.add_argument("--mean-file", default="", help="also write the statistics file of the dataset (GPU path)")
    ap.add_argument("--host", action="store_true", help="resize and crop on the host with numpy: no GPU call")
    args = ap.parse_args(argv)
    if not args.input or not args.output:
        ap.print_help()
        return 1
    info = Image2HDF5(args.input, args.output, args.crop, args.resize, args.board, args.chunk, args.labels or None, args.mean_file or None,
                      args.host)
    print(f"{info['files']} images of {info['dims']} bytes in {info['chunks']} chunks: "
          + ("crop_images_u8 on decoded files" if info["path"] == "kernel" else "numpy resize on the host"))
    print(args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
