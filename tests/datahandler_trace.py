"""The data handlers' call trace, recorded without a GPU.

``DataHandler`` and ``ChunkDataHandler`` (convnet_amd/datahandler.py) reach the device through ``Matrix`` alone, so "a refactor of the data
handler leaves behaviour as it was" can be checked exactly, like the host's (tests/host_trace.py, whose ``Recorder`` this uses).  A trace
holds every library call as the recorder writes it; for every ``Matrix.FromNumpy`` the SHA-256 of the array (the recorder does not carry
the copy out, so the column index, the first-frame tables, the permutations and the means are pinned here); and after every ``GetBatch``,
behind a ``Sync()``, every reader's ``num_reads_`` and ``Tell()`` and the SHA-256 of every host buffer in ``host_``.

Stand-ins, all of them here and none in the package: ``Matrix._device`` is the CPU; ``torch.empty(pin_memory=True)`` gives zeroed unpinned
memory; ``torch.cuda.Event`` / ``current_stream`` do nothing; ``Matrix.StagePatchesU8`` / ``StageClipsU8`` — whose ``is_cuda`` guard cannot
pass — are recorded at the ``Matrix`` level with every argument and the SHA-256 of the byte tensor they were handed.

Per config: build, ``SetInputLayers``, 12 ``GetBatch`` on stand-in layers, ``Seek(0)``, 3 more, ``close``.  The files are written into a
temporary directory from a seeded generator: 40 rows of 3 x 8 x 8 bytes with a float32 twin, a second byte dataset, 28 frames with a
boundary file that has one too-short sequence, labels, and a mean file with mean / std and pixel_mean / pixel_std / S / U.

tests/test_datahandler_trace_cpu.py compares the traces with tests/golden/datahandler_trace.json.  Only names that convnet.py, the tools
and the tests read are used, so the same file runs on another checkout:  python tests/datahandler_trace.py CONFIG  dumps a trace for
diffing,  --list  names the configs,  --golden  prints the JSON."""
import contextlib
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from convnet_amd import hdf5io, matrix, pbtxt  # noqa: E402
from convnet_amd.datahandler import ChunkDataHandler, DataHandler  # noqa: E402
from convnet_amd.matrix import Matrix  # noqa: E402
from host_trace import Recorder, digest  # noqa: E402,F401

ROWS, COLORS, SIZE, CROP, FRAMES, T, BATCH = 40, 3, 8, 6, 28, 4, 4
DIMS = COLORS * SIZE * SIZE
BOUNDS = [9, 2, 17]                      # 6 clips of 4, a sequence too short for one, 14 clips: 20 rows


def write_files(d):
    """The dataset files, in directory ``d``; the paths by name."""
    rng = np.random.default_rng(1234)
    f = {k: os.path.join(d, v) for k, v in (("rows", "rows.h5"), ("frames", "frames.h5"), ("mean", "mean.h5"), ("bounds", "bounds.txt"))}
    x = rng.integers(0, 256, (ROWS, DIMS), dtype=np.uint8)
    with hdf5io.File(f["rows"], "w") as h:
        h.WriteDataset("x", x)
        h.WriteDataset("xf", x.astype(np.float32))
        h.WriteDataset("x2", rng.integers(0, 256, (ROWS, 12), dtype=np.uint8))
        h.WriteDataset("y", (np.arange(ROWS) % 10).astype(np.float32))
    with hdf5io.File(f["frames"], "w") as h:
        h.WriteDataset("x", rng.integers(0, 256, (FRAMES, DIMS), dtype=np.uint8))
        h.WriteDataset("y", np.arange(FRAMES, dtype=np.float32))
    with open(f["bounds"], "w") as h:
        h.write(" ".join(map(str, BOUNDS)) + "\n")
    with hdf5io.File(f["mean"], "w") as h:          # a (dims, 1) column-major matrix is a (1, dims) dataset
        h.WriteHDF5CPU((rng.random(DIMS) * 255).astype(np.float32), 1, DIMS, "mean")
        h.WriteHDF5CPU(((rng.random(DIMS) + 0.5) * 60).astype(np.float32), 1, DIMS, "std")
        h.WriteHDF5CPU(np.array([120.5, 113.25, 99.0], np.float32), 1, COLORS, "pixel_mean")
        h.WriteHDF5CPU(np.array([61.0, 58.5, 64.75], np.float32), 1, COLORS, "pixel_std")
        h.WriteHDF5CPU(np.array([0.3, 0.2, 0.1], np.float32), COLORS, 1, "S")
        h.WriteHDF5CPU(rng.standard_normal((COLORS, COLORS)).astype(np.float32), COLORS, COLORS, "U")
    f["images"], f["labels"] = x[:18].astype(np.float32), (np.arange(18) % 10).astype(np.float32)
    f["mean_v"], f["std_v"] = (rng.random(DIMS) * 255).astype(np.float32), ((rng.random(DIMS) + 0.5) * 60).astype(np.float32)
    return f


ACCESS = {"sequential": "", "randomize_gpu": "randomize_gpu: true", "randomize_cpu": "randomize_cpu: true random_access_chunk_size: 4",
          "pipeline_loads": "pipeline_loads: true",
          "all_three": "randomize_gpu: true randomize_cpu: true random_access_chunk_size: 4 pipeline_loads: true"}
GEOM = f"image_size: {SIZE} num_colors: {COLORS}"
CROPPED = f"{GEOM} gpu_image_size_y: {CROP} gpu_image_size_x: {CROP}"


def _jitter(f):
    return f'{CROPPED} can_translate: true can_flip: true normalize: true mean_file: "{f["mean"]}"'


def _rows(f, stream="", extra="", dataset="x", second=False):
    text = f'data_config {{ file_pattern: "{f["rows"]}" layer_name: "input" dataset_name: "{dataset}" {stream} }}\n'
    if second:
        text += f'data_config {{ file_pattern: "{f["rows"]}" layer_name: "input2" dataset_name: "x2" }}\n'
    text += f'data_config {{ file_pattern: "{f["rows"]}" layer_name: "output" dataset_name: "y" }}\nbatch_size: {BATCH}\n{extra}\n'
    return text, ["input", "input2"] if second else ["input"]


def _clips(f, stream="", extra=""):
    seq = f'is_sequence: true seq_length: {T} boundary_file: "{f["bounds"]}"'
    return (f'data_config {{ file_pattern: "{f["frames"]}" layer_name: "input" dataset_name: "x" {seq} {stream} }}\n'
            f'data_config {{ file_pattern: "{f["frames"]}" layer_name: "output" dataset_name: "y" {seq} pick_first: true }}\n'
            f'batch_size: {BATCH}\n{extra}\n'), ["input"]


def configs(f):
    """name -> ("handler", dataset text, input layer names, raw_chunks) or ("chunk", ChunkDataHandler keywords)."""
    named = {}
    for access, flags in ACCESS.items():     # chunk 6: a batch and a dropped tail of 2 per chunk, the last random run cut; 16: four batches
        named[f"rows_{access}"] = _rows(f, extra=f"chunk_size: 6 {flags}")
        named[f"rows_{access}_jitter"] = _rows(f, _jitter(f), f"chunk_size: 16 {flags}")
        named[f"clips_{access}"] = _clips(f, extra=f"chunk_size: 16 {flags}")
        named[f"clips_{access}_jitter"] = _clips(f, _jitter(f), f"chunk_size: 6 {flags}")
    named["multiplicity_corners"] = _rows(f, f"{CROPPED} can_translate: false can_flip: false", "chunk_size: 16 multiplicity: 10")
    named["pixelwise_pca"] = _rows(f, f'{CROPPED} can_translate: true can_flip: true pixelwise_normalize: true pca_noise_stddev: 0.1 '
                                      f'mean_file: "{f["mean"]}"', "chunk_size: 16 randomize_gpu: true")
    named["normalize_local"] = _rows(f, f'{GEOM} normalize_local: true normalize: true mean_file: "{f["mean"]}"', "chunk_size: 6")
    named["max_reuse_count"] = _rows(f, _jitter(f), "chunk_size: 6 max_reuse_count: 2 randomize_gpu: true")
    named["fits_on_gpu"] = _rows(f, _jitter(f), "chunk_size: 0 randomize_gpu: true")
    named["float32_dataset"] = _rows(f, _jitter(f), "chunk_size: 16 randomize_gpu: true", dataset="xf")
    named["two_byte_streams"] = _rows(f, _jitter(f), "chunk_size: 16 randomize_gpu: true", second=True)
    named["pick_first"] = _clips(f, f"{CROPPED} can_translate: true can_flip: true pick_first: true", "chunk_size: 6 randomize_gpu: true")
    out = {f"{name} {'bytes' if raw else 'float'}": ("handler", text, inputs, raw) for name, (text, inputs) in named.items()
           for raw in (True, False)}
    common = dict(images=f["images"], labels=f["labels"], batch_size=BATCH, image_size=SIZE, colors=COLORS)
    out["chunk_jitter_reshuffle"] = ("chunk", dict(common, crop_size=CROP, mean=f["mean_v"], std=f["std_v"], randomize=True, seed=5))
    out["chunk_corners"] = ("chunk", dict(common, crop_size=CROP, translate=False, flip=False, randomize=True, seed=6))
    out["chunk_sequential_wrap"] = ("chunk", dict(common, translate=False, flip=False, randomize=False))
    return out


class _Layer:
    """What GetBatch asks of a data layer."""

    def __init__(self, name, is_input, dims):
        self.name_, self.is_input_ = name, is_input
        self.m_ = Matrix()
        self.m_.AllocateGPUMemory(BATCH, dims)

    def GetName(self):
        return self.name_

    def IsInput(self):
        return self.is_input_

    def GetState(self):
        assert self.is_input_
        return self.m_

    def GetData(self):
        assert not self.is_input_
        return self.m_


class _Event:
    def record(self, stream=None):
        pass

    def synchronize(self):
        pass


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def trace(config):
    """The canonical lines of one config of ``configs()``."""
    rec = Recorder()
    saved = (matrix.lib, Matrix._device, Matrix.AllocateGPUMemory, Matrix.FromNumpy, Matrix.__dict__["StagePatchesU8"],
             Matrix.__dict__["StageClipsU8"], Matrix._temp,
             Matrix._temp_size, Matrix._ones, Matrix._ones_size, Matrix._rnd, torch.empty, torch.cuda.Event, torch.cuda.current_stream)
    allocate, from_numpy, empty = Matrix.AllocateGPUMemory, Matrix.FromNumpy, torch.empty

    def allocate_and_register(self, rows, cols, name=""):
        allocate(self, rows, cols, name)
        rec.register(self)

    def from_numpy_hashed(self, arr):
        rec.lines.append("# FromNumpy " + _sha(np.ascontiguousarray(arr, np.float32)))
        from_numpy(self, arr)

    def unpinned(*args, pin_memory=False, **kw):
        return torch.zeros(*args, **kw) if pin_memory else empty(*args, **kw)

    def staging(entry):
        def record(chunk, *args):
            assert chunk.dtype == torch.uint8
            rec.lines.append(f"{entry} {_sha(chunk.numpy())} " + " ".join(rec._mat(a.mat_) if isinstance(a, Matrix) else rec._arg(a) for a in args))
        return staticmethod(record)

    matrix.lib = rec
    Matrix._device = torch.device("cpu")
    Matrix.AllocateGPUMemory, Matrix.FromNumpy = allocate_and_register, from_numpy_hashed
    Matrix.StagePatchesU8, Matrix.StageClipsU8 = staging("StagePatchesU8"), staging("StageClipsU8")
    Matrix._temp = Matrix._ones = None
    Matrix._temp_size = Matrix._ones_size = 0
    torch.empty, torch.cuda.Event, torch.cuda.current_stream = unpinned, _Event, lambda: None
    try:
        Matrix.InitRandom(42)
        if config[0] == "chunk":
            dh = ChunkDataHandler(**config[1])
            crop = config[1].get("crop_size") or SIZE
            layers = [_Layer("input", True, COLORS * crop * crop), _Layer("output", False, 1)]
        else:
            _, text, inputs, raw = config
            dh = DataHandler(pbtxt.parse(text, pbtxt.DatasetConfig), raw_chunks=raw, seed=7)
            dh.SetInputLayers(inputs)
            layers = [_Layer(name, name in inputs, st.StagedDims()) for name, st in dh.streams_.items()]

        def batches(count):
            for _ in range(count):
                rec.lines.append("# GetBatch")
                dh.GetBatch(layers)
                dh.Sync()
                for name, st in getattr(dh, "streams_", {}).items():
                    rec.lines.append(f"# reader {name} reads {st.reader_.num_reads_} tell {st.reader_.Tell()}")
                for i, buffers in enumerate(getattr(dh, "host_", None) or ()):
                    for name, a in buffers.items():
                        rec.lines.append(f"# host {i} {name} {a.dtype} {a.shape} {_sha(a)}")

        batches(12)
        rec.lines.append("# Seek(0)")
        dh.Seek(0)
        batches(3)
        if hasattr(dh, "close"):
            dh.close()
    finally:
        (matrix.lib, Matrix._device, Matrix.AllocateGPUMemory, Matrix.FromNumpy, Matrix.StagePatchesU8, Matrix.StageClipsU8, Matrix._temp,
         Matrix._temp_size, Matrix._ones, Matrix._ones_size, Matrix._rnd, torch.empty, torch.cuda.Event, torch.cuda.current_stream) = saved
    return rec.lines


def traces(names=None):
    """name -> lines, for ``names`` or every config; the files live only while this runs."""
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(sys.stderr):     # (a sequence reader warns on stdout)
        cfgs = configs(write_files(d))
        return {n: trace(cfgs[n]) for n in (names or cfgs)}


def names():
    with tempfile.TemporaryDirectory() as d:
        return list(configs(write_files(d)))


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--list" in args:
        print("\n".join(names()))
    elif "--golden" in args:
        print(json.dumps({n: digest(lines) for n, lines in traces().items()}, indent=0))
    else:
        print("\n".join(traces([" ".join(args)])[" ".join(args)]))
