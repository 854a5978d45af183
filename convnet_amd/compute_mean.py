"""``python -m convnet_amd.compute_mean --board B --data D --layer L --output O`` — apps/compute_mean.cc: one pass over an HDF5 data
stream writes the statistics file that the stream's ``mean_file`` names: ``mean`` / ``std`` (1, dims) for ``normalize``, ``pixel_mean`` /
``pixel_std`` (1, C) for ``pixelwise_normalize``, ``pixel_cov`` (C, C), and ``S`` (1, C) / ``U`` (C, C) for ``pca_noise_stddev``.

The pass walks every stored row once, in file order, chunk by chunk through the data handler's own machinery (row reader, pinned host
buffers, the preload thread): the next chunk is read while the current one is summed.  It runs on a COPY of the config with everything
that changes a row on its way to the layer cleared (normalisation, jitter, shuffling), so a training config works as it stands before
its ``mean_file`` exists, and the statistics are those of the stored rows — all of them, a tail shorter than a batch included.

Two paths.  A stream stored as unsigned bytes with at most 4 colours keeps its chunk as bytes and takes ``chunk_moments_u8``: exact
integer sums of x, x^2 and the colour products, one read of the chunk, finished on the host from the integers (numerators in exact
integer arithmetic, then float64, then float32).  Everything else — and ``raw_chunks=False`` — takes the reference's op sequence on the
float chunk: Add, Reshape + Dot, Mult, Add per batch-sized piece, then SumRows / Subtract / Sqrt (apps/compute_mean.cc:70-127).

``pixel_cov`` is what the reference writes: the CORRELATION matrix of the colours, (E[x_c x_c'] - m_c m_c') / (s_c s_c').  ``S`` / ``U``
are ours (the reference has no program that writes them): the eigen-decomposition of ``pixel_cov`` in the form AddPCANoise consumes —
``S`` = sqrt(eigenvalues), descending, clamped at 0; ROW k of the matrix ``U`` is eigenvector k (largest component positive), so that
U^T diag(S^2) U = pixel_cov and the noise randn(n, C) * S . U, which is added AFTER normalisation, has the colours' correlation.  A
stream with a constant colour channel (``pixel_std`` 0) has a 0/0 in ``pixel_cov`` and gets no ``S`` / ``U``."""
import argparse
import sys

import numpy as np

from . import hdf5io, pbtxt

_STREAM_CLEARED = ("normalize", "pixelwise_normalize", "normalize_local", "pca_noise_stddev", "mean_file", "can_translate", "can_flip",
                   "gpu_image_size_y", "gpu_image_size_x")
_DATASET_CLEARED = ("randomize_cpu", "randomize_gpu")
DATASETS = ("mean", "pixel_mean", "std", "pixel_std", "pixel_cov", "S", "U")      # in the order they are written


def StoredRowsConfig(data_config, layer_name):
    """The copy of a DatasetConfig a statistics pass runs on: ``layer_name``'s stream alone, rows as stored."""
    if isinstance(data_config, str):
        data_config = pbtxt.read(data_config, pbtxt.DatasetConfig)
    streams = [d for d in data_config.data_config if d.layer_name == layer_name]
    if not streams:
        raise SystemExit(f"Layer name {layer_name} not found.")
    dsc = streams[0].copy()
    if dsc.is_sequence:
        raise SystemExit(f"Data stream for layer {layer_name}: compute_mean does not take a sequence stream (is_sequence): the statistics "
                         "are per frame, so point the config at the base frame stream.")
    for field in _STREAM_CLEARED:
        dsc._set.pop(field, None)
    cfg = data_config.copy()
    cfg._set["data_config"] = [dsc]
    for field in _DATASET_CLEARED:
        cfg._set.pop(field, None)
    cfg.pipeline_loads = True            # the next chunk's read runs beside this chunk's sums
    return cfg


def EigenNoise(pixel_cov):
    """(S, U) of a correlation matrix, float64, in the module docstring's convention."""
    w, v = np.linalg.eigh(np.asarray(pixel_cov, np.float64))
    order = np.argsort(w)[::-1]
    U = v[:, order].T.copy()
    for u in U:
        if u[np.argmax(np.abs(u))] < 0:
            u *= -1
    return np.sqrt(np.maximum(w[order], 0.0)), U


def _with_noise(stats):
    if np.all(stats["pixel_std"] > 0) and np.all(np.isfinite(stats["pixel_cov"])):
        S, U = EigenNoise(stats["pixel_cov"])
        stats["S"], stats["U"] = S.astype(np.float32), U.astype(np.float32)
    return stats


def FinishMoments(acc, num_cases, dims, num_colors):
    """The statistics from chunk_moments_u8's sums over ``num_cases`` cases.  Every numerator — N * sum(x^2) - sum(x)^2 and its colour
    counterparts — is formed in exact (Python) integers; it becomes float64 once, and the result float32."""
    C, N = int(num_colors), int(num_cases)
    P = dims // C
    sums = [int(v) for v in acc]
    s, q, x = sums[:dims], sums[dims:2 * dims], sums[2 * dims:]
    f64 = lambda ints: np.array([float(v) for v in ints], np.float64)
    mean = f64(s) / N
    std = np.sqrt(f64(N * b - a * a for a, b in zip(s, q))) / N
    K = N * P
    cs = [sum(s[c * P:(c + 1) * P]) for c in range(C)]
    num = [[K * x[c * C + d] - cs[c] * cs[d] for d in range(C)] for c in range(C)]       # K^2 * covariance
    root = np.sqrt(f64(num[c][c] for c in range(C)))
    with np.errstate(divide="ignore", invalid="ignore"):
        pixel_cov = f64(v for r in num for v in r).reshape(C, C) / np.outer(root, root)
    f = np.float32
    stats = {"mean": mean.astype(f), "std": std.astype(f), "pixel_mean": (f64(cs) / K).astype(f), "pixel_std": (root / K).astype(f)}
    if np.all(root > 0):
        S, U = EigenNoise(pixel_cov)                 # from the float64 matrix
        stats["S"], stats["U"] = S.astype(f), U.astype(f)
    stats["pixel_cov"] = pixel_cov.astype(f)
    return stats


class _FloatSums:
    """The reference's accumulators (apps/compute_mean.cc:53-80) on float pieces of up to ``batch`` cases: per (position in the piece,
    dim) the sums of x and of x^2, and the C x C product scaled per piece.  A piece shorter than a batch has accumulators of its own
    shape, so every piece enters with its true case count."""

    def __init__(self, Matrix, dims, num_colors, num_cases):
        self.Matrix_, self.dims_, self.C_, self.N_ = Matrix, dims, num_colors, num_cases
        self.P_ = dims // num_colors
        self.sets_ = {}                    # cases in a piece -> (state, mean_batch, var_batch)
        self.pixel_cov_ = Matrix()
        self.pixel_cov_.AllocateGPUMemory(num_colors, num_colors)
        self.pixel_cov_.Set(0)

    def Add(self, stage, start, end):
        """``stage(start, end, state)`` leaves cases start:end of the resident chunk in ``state`` (cases, dims), as a batch is staged."""
        n = end - start
        if n not in self.sets_:
            ms = self.sets_[n] = tuple(self.Matrix_() for _ in range(3))
            for m in ms:
                m.AllocateGPUMemory(n, self.dims_)
                m.Set(0)
        state, mean_batch, var_batch = self.sets_[n]
        stage(start, end, state)
        mean_batch.Add(state)
        state.Reshape(-1, self.C_)
        self.Matrix_.Dot(state, state, self.pixel_cov_, 1, 1.0 / (self.N_ * self.P_), True, False)
        state.Reshape(n, -1)
        state.Mult(state)
        var_batch.Add(state)

    def Finish(self):
        Matrix, C, dims = self.Matrix_, self.C_, self.dims_
        mean_image, var_image, mean_pixel, var_pixel, out_p = (Matrix() for _ in range(5))
        for m, shape in ((mean_image, (1, dims)), (var_image, (1, dims)), (mean_pixel, (1, C)), (var_pixel, (1, C)), (out_p, (C, C))):
            m.AllocateGPUMemory(*shape)
        for i, (_, mean_batch, var_batch) in enumerate(self.sets_.values()):
            mean_batch.SumRows(mean_image, min(i, 1), 1.0 / self.N_)
            var_batch.SumRows(var_image, min(i, 1), 1.0 / self.N_)           # (E[x^2] so far)
        for image, pixel in ((mean_image, mean_pixel), (var_image, var_pixel)):
            image.Reshape(-1, C)
            image.SumRows(pixel, 0, 1.0 / self.P_)
            image.Reshape(1, -1)
        Matrix.Dot(mean_pixel, mean_pixel, out_p, 0, 1, True, False)
        self.pixel_cov_.Subtract(out_p, self.pixel_cov_)
        stats = {"mean": mean_image.ToNumpy().reshape(-1), "pixel_mean": mean_pixel.ToNumpy().reshape(-1)}
        mean_image.Mult(mean_image)
        mean_pixel.Mult(mean_pixel)
        var_image.Subtract(mean_image, var_image)
        var_pixel.Subtract(mean_pixel, var_pixel)
        var_image.Sqrt()
        var_pixel.Sqrt()
        stats["std"], stats["pixel_std"] = var_image.ToNumpy().reshape(-1), var_pixel.ToNumpy().reshape(-1)
        Matrix.Dot(var_pixel, var_pixel, out_p, 0, 1, True, False)
        self.pixel_cov_.Divide(out_p)
        stats["pixel_cov"] = self.pixel_cov_.ToNumpy().reshape(C, C)          # (symmetric: either order)
        return _with_noise(stats)


def ComputeMean(data_config, layer_name, num_colors, *, raw_chunks=True):
    """The statistics of ``layer_name``'s stream of ``data_config`` (a pbtxt.DatasetConfig or the path of one) as float32 arrays by
    dataset name (``DATASETS``; no S / U for a constant channel), and under ``"info"`` what the pass did: ``path`` ("kernel" or
    "float"), ``dataset_size``, ``dims``, ``image_size`` (y, x) and ``chunks``."""
    import torch
    from .datahandler import DataHandler, size_yx
    from .matrix import Matrix
    C = int(num_colors)
    cfg = StoredRowsConfig(data_config, layer_name)
    if C < 1:
        raise SystemExit(f"Data stream for layer {layer_name}: num_colors {C} is not a colour count.")
    cfg.data_config[0].num_colors = C
    dh = DataHandler(cfg, raw_chunks=bool(raw_chunks) and C <= 4)
    try:
        st = dh.streams_[layer_name]
        if st.is_images_:
            raise SystemExit(f"Data stream for layer {layer_name}: compute_mean does not take an IMAGE_RAW stream: the statistics pass "
                             "reads stored rows, and a list of image files stores none.")
        dims, size, chunk, batch = st.GetDims(), dh.GetDataSetSize(), dh.chunk_size_, dh.GetBatchSize()
        if dims % C:
            raise SystemExit(f"Data stream for layer {layer_name}: rows of {dims} values are not {C} colours of whole images.")
        dh.SetInputLayers([layer_name])
        dh.AllocateMemory()
        kernel = st.raw_
        if kernel:
            acc = torch.zeros(2 * dims + C * C, dtype=torch.int64, device=Matrix()._dev())
        else:
            sums = _FloatSums(Matrix, dims, C, size)
            stage = lambda start, end, state: st.form_.Stage(st, start, end, state)
        for _, valid in dh.ChunkPass():                # (what a last chunk holds behind its valid part is not counted)
            if kernel:
                Matrix.ChunkMomentsU8(st.form_.data_, dims, chunk, 0, valid, C, acc)
            else:
                for start in range(0, valid, batch):
                    sums.Add(stage, start, min(start + batch, valid))
        if kernel:
            stats = FinishMoments(acc.cpu().numpy().view(np.uint64), size, dims, C)
        else:
            stats = sums.Finish()
        stats["info"] = {"path": "kernel" if kernel else "float", "dataset_size": size, "dims": dims,
                         "image_size": size_yx(cfg.data_config[0], "image_size"), "chunks": -(-size // chunk)}
        return stats
    finally:
        dh.close()


def WriteMeanFile(path, stats):
    """The datasets of ``stats`` under the reference's names.  ``mean``, ``pixel_mean``, ``std``, ``pixel_std`` and ``pixel_cov`` are the
    reference's own WriteHDF5CPU calls (apps/compute_mean.cc:98-129): datasets (1, dims), (1, C) and (C, C), which LoadMeans reads flat.
    ``S`` and ``U`` are read as MATRICES (Matrix.AllocateAndReadHDF5), and a column-major matrix (rows, cols) is the row-major dataset
    (cols, rows): the matrix ``S`` (1, C) goes out as the dataset (C, 1) and ``U`` transposed, so the loader gets back the row vector and
    the matrix whose rows are the eigenvectors — the shapes the reference's examples/imagenet/pixel_mean.h5 reads as."""
    C = int(np.size(stats["pixel_mean"]))
    dims = int(np.size(stats["mean"]))
    shapes = {"mean": (1, dims), "pixel_mean": (1, C), "std": (1, dims), "pixel_std": (1, C), "pixel_cov": (C, C), "S": (C, 1), "U": (C, C)}
    with hdf5io.File(path, "w") as f:
        for name in DATASETS:
            if name in stats:
                a = np.asarray(stats[name], np.float32)
                f.WriteHDF5CPU(a.reshape(C, C).T if name == "U" else a, *shapes[name], name)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m convnet_amd.compute_mean", description=__doc__.split("\n\n")[0])
    ap.add_argument("--board", "-b", default="", help="GPU board: 0, 1, ...")
    ap.add_argument("--data", "-d", default="", help="Data pbtxt file")
    ap.add_argument("--layer", "-l", default="", help="Layer pbtxt file: its name and num_channels are used")
    ap.add_argument("--layer-name", default="", help="in place of --layer: the layer whose stream is read")
    ap.add_argument("--num-colors", type=int, default=0, help="in place of --layer: the layer's number of channels")
    ap.add_argument("--output", "-o", default="", help="Output hdf5 file")
    ap.add_argument("--float-chunks", action="store_true", help="take the float op sequence where the byte kernel would serve")
    args = ap.parse_args(argv)
    if not args.board or not args.data or not args.output or not (args.layer or (args.layer_name and args.num_colors > 0)):
        ap.print_help()
        return 1
    from .matrix import Matrix
    from .train_convnet import ParseBoardIds
    boards = ParseBoardIds(args.board)
    Matrix.SetupCUDADevice(boards[0])
    print(f"Using board {boards[0]}")
    if args.layer:
        layer = pbtxt.read(args.layer, pbtxt.Layer)
        name, colors = layer.name, layer.num_channels
    else:
        name, colors = args.layer_name, args.num_colors
    stats = ComputeMean(args.data, name, colors, raw_chunks=not args.float_chunks)
    info = stats["info"]
    print(f"Data set size {info['dataset_size']}")
    if info["image_size"][0] > 0 and info["image_size"][1] > 0:
        print(f"Image size {info['image_size'][0]}x{info['image_size'][1]}")
    else:
        print(f"Image size {info['dims'] // colors} pixels of {colors} colours")
    print("Path: " + ("chunk_moments_u8 on byte chunks (exact integer moments)" if info["path"] == "kernel"
                      else "float op sequence on float chunks") + f", {info['chunks']} chunks")
    if "S" not in stats:
        print("A colour channel is constant: pixel_cov is undefined there, no S / U written.")
    print(args.output)
    WriteMeanFile(args.output, stats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
