"""CPU: the disk side of the data pipeline — DatasetConfig pbtxt, HDF5 row reader, DataHandler::DiskAccess on plain host buffers and
the refused stream kinds.  No GPU call is made: a DataHandler touches the device only from AllocateMemory / GetBatch on."""
import json
import os

import numpy as np
import pytest

from convnet_amd import hdf5io, pbtxt
from convnet_amd.datahandler import DataHandler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW_TYPES = ["int8", "int32", "int64", "uint8", "uint32", "uint64", "float32", "float64"]


# ---- config ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dataset,flags", [("train_data.pbtxt", "train", (True, True)), ("val_data.pbtxt", "validation", (False, False))])
def test_the_mnist_conv_dataset_files_parse(name, dataset, flags):
    c = pbtxt.read(os.path.join(GOLDEN, "dataset_pbtxt", name), cls=pbtxt.DatasetConfig)
    assert [(d.file_pattern, d.layer_name, d.dataset_name, d.data_type) for d in c.data_config] == [
        ("../data/mnist.h5", "input", dataset, "HDF5"), ("../data/mnist.h5", "output", dataset + "_labels", "HDF5")]
    assert c.batch_size == 100 and (c.randomize_cpu, c.randomize_gpu) == flags
    # everything the files leave out reads as the proto's default
    assert (c.chunk_size, c.max_reuse_count, c.pipeline_loads, c.random_access_chunk_size, c.max_dataset_size, c.multiplicity) == (0, 0, False, 1, 0, 1)
    d = c.data_config[0]
    assert not d.has_image_size() and not d.has_gpu_image_size_y() and d.has_data_type()
    assert (d.num_colors, d.can_flip, d.can_translate, d.normalize, d.gpu_id, d.context_factor, d.stride) == (3, False, False, False, 0, 1.0, 1)
    assert pbtxt.parse(pbtxt.dump(c), pbtxt.DatasetConfig)._set.keys() == c._set.keys()


def test_dataset_schema_matches_the_reference_proto_field_for_field():
    """DataStreamConfig / DatasetConfig against proto/convnet_config.proto:289-382 as stored in tests/golden/ref_dataset_schema.json
    (tests/golden/make_dataset_fixtures.py), every field and every default."""
    with open(os.path.join(GOLDEN, "ref_dataset_schema.json")) as f:
        schema = json.load(f)
    ints = {"int32", "int64", "uint32", "uint64"}
    for name, cls in (("DataStreamConfig", pbtxt.DataStreamConfig), ("DatasetConfig", pbtxt.DatasetConfig)):
        proto = {f["name"]: f for f in schema["messages"][name]}
        assert set(proto) == set(cls.FIELDS), name
        for key, mine in cls.FIELDS.items():
            f, d = proto[key], proto[key]["default"]
            if f["label"] == "repeated":
                assert mine == (list, pbtxt.DataStreamConfig), key
            elif f["type"] == "string":
                assert mine == ("" if d is None else d.strip('"')), key
            elif f["type"] == "bool":
                assert mine is (d == "true"), key
            elif f["type"] == "float":
                assert type(mine) is float and mine == (0.0 if d is None else float(d)), key
            elif f["type"] in ints:
                assert type(mine) is int and mine == (0 if d is None else int(d)), key
            else:
                assert f["type"] == "DataType" and mine == d == "HDF5", key
    assert schema["enums"]["DataType"] == ["DUMMY", "HDF5", "IMAGE_RAW", "SLIDING_WINDOW", "TXT", "BOUNDING_BOX", "CROPS", "VIDEO_RAW"]


# ---- HDF5 rows --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def typed_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rows") / "typed.h5")
    rng = np.random.default_rng(0)
    arrays = {}
    for t in ROW_TYPES:
        info = np.iinfo(t) if np.dtype(t).kind in "iu" else None
        a = (rng.integers(info.min, info.max, (23, 5), dtype=t, endpoint=True) if info is not None
             else (rng.standard_normal((23, 5)) * 1e3).astype(t))
        arrays[t] = a
    arrays["labels"] = np.arange(23, dtype=np.int32)                 # 1-D
    arrays["shorts"] = np.arange(12, dtype=np.int16).reshape(4, 3)
    with hdf5io.File(path, "w") as f:
        for name, a in arrays.items():
            if a.dtype == np.int16:                                   # WriteDataset refuses it too: written as a checkpoint-style matrix
                continue
            f.WriteDataset(name, a)
        with pytest.raises(ValueError, match="int16"):
            f.WriteDataset("shorts", arrays["shorts"])
        with pytest.raises(ValueError):
            f.WriteDataset("cube", np.zeros((2, 2, 2), np.float32))
    return path, arrays


def test_row_reader_reads_every_type_as_the_reference_cast(typed_file):
    path, arrays = typed_file
    with hdf5io.File(path) as f:
        for t in ROW_TYPES:
            r = f.RowReader(t)
            assert (r.GetDataSetSize(), r.GetDims(), r.GetStoredType()) == (23, 5, np.dtype(t))
            for a, b in ((0, 23), (0, 1), (22, 23), (3, 11), (17, 20)):
                out = np.full((b - a + 1, 5), -7.0, np.float32)       # one row more than asked for: it must stay
                r.Get(out, a, b)
                assert np.array_equal(out[:b - a], arrays[t][a:b].astype(np.float32)), (t, a, b)
                assert np.all(out[b - a:] == -7.0)
            with pytest.raises(IndexError):
                r.Get(np.zeros((2, 5), np.float32), 22, 24)
            with pytest.raises(IndexError):
                r.Get(np.zeros((2, 5), np.float32), 5, 5)
            r.close()
        r = f.RowReader("labels")                                     # a 1-D dataset has 1 dim
        assert (r.GetDataSetSize(), r.GetDims()) == (23, 1)
        out = np.zeros((6, 1), np.float32)
        r.Get(out, 4, 10)
        assert out.reshape(-1).tolist() == [4, 5, 6, 7, 8, 9]


def test_row_reader_as_stored_is_for_unsigned_bytes_only(typed_file):
    path, arrays = typed_file
    with hdf5io.File(path) as f:
        r = f.RowReader("uint8")
        out = np.zeros((9, 5), np.uint8)
        r.Get(out, 14, 23)
        assert np.array_equal(out, arrays["uint8"][14:23])
        for t in ROW_TYPES:
            if t != "uint8":
                with pytest.raises(TypeError, match=t):
                    f.RowReader(t).Get(out, 0, 2)
        with pytest.raises(ValueError):
            r.Get(np.zeros((9, 5), np.int32), 0, 2)                   # neither read mode


def test_row_reader_get_next_seek_tell_and_the_wrap(typed_file):
    path, arrays = typed_file
    with hdf5io.File(path) as f:
        r = f.RowReader("int32")
        r.Seek(21)
        row, seen = np.zeros(5, np.float32), []
        for _ in range(4):
            seen.append(r.Tell())
            r.GetNext(row)
            assert np.array_equal(row, arrays["int32"][seen[-1]].astype(np.float32))
        assert seen == [21, 22, 0, 1] and r.Tell() == 2
        r.SetMaxDataSetSize(20)                                       # max_dataset_size: the wrap moves with it
        r.Seek(19)
        r.GetNext(row)
        assert r.Tell() == 0 and r.GetDataSetSize() == 20


def test_row_reader_refuses_other_types_by_name(tmp_path):
    # no writer here makes a 16-bit dataset, so one comes from libhdf5 directly
    import ctypes
    path = str(tmp_path / "short.h5")
    with hdf5io.File(path, "w") as f:
        L = hdf5io._lib()
        t16 = ctypes.c_int64.in_dll(L, "H5T_NATIVE_INT16_g").value
        a = np.arange(12, dtype=np.int16)
        space = L.H5Screate_simple(2, (ctypes.c_uint64 * 2)(4, 3), None)
        ds = L.H5Dcreate2(f.id, b"shorts", t16, space, 0, 0, 0)
        assert ds >= 0 and L.H5Dwrite(ds, t16, 0, 0, 0, a.ctypes.data_as(ctypes.c_void_p)) >= 0
        L.H5Sclose(space)
        L.H5Dclose(ds)
    with hdf5io.File(path) as f:
        with pytest.raises(TypeError, match=r"shorts.*integer of 2 bytes"):
            f.RowReader("shorts")
        with pytest.raises(KeyError, match="nothing_here"):
            f.RowReader("nothing_here")


def test_existing_matrix_io_is_unchanged(tmp_path):
    path = str(tmp_path / "m.h5")
    with hdf5io.File(path, "w") as f:
        f.WriteHDF5CPU(np.arange(6, dtype=np.float32), 2, 3, "m")
        f.WriteHDF5IntAttr("k", 5)
    with hdf5io.File(path) as f:
        assert f.ReadHDF5Shape("m") == (3, 2) and f.ReadHDF5CPU(6, "m").tolist() == [0, 1, 2, 3, 4, 5] and f.ReadHDF5IntAttr("k", 0) == 5
        r = f.RowReader("m")                                          # and a checkpoint matrix is a float dataset of rows
        assert (r.GetDataSetSize(), r.GetDims()) == (2, 3)


# ---- DiskAccess on host buffers ---------------------------------------------------------------------------------------------------------
DIMS, ROWS = 6, 23


@pytest.fixture(scope="module")
def rows_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("disk") / "rows.h5")
    data = ((7 * np.arange(ROWS)[:, None] + np.arange(DIMS)) % 251).astype(np.uint8)      # every row is recognisable
    with hdf5io.File(path, "w") as f:
        f.WriteDataset("x", data)
        f.WriteDataset("y", np.arange(ROWS, dtype=np.float32))
        f.WriteDataset("short", np.arange(ROWS - 1, dtype=np.float32))
    return path, data


def _config(path, extra="", stream=""):
    return pbtxt.parse(f'data_config {{ file_pattern: "{path}" layer_name: "input" dataset_name: "x" {stream} }}\n'
                       f'data_config {{ file_pattern: "{path}" layer_name: "output" dataset_name: "y" }}\nbatch_size: 2\n{extra}', pbtxt.DatasetConfig)


def _rows_of(chunk, data):
    """The dataset row each case of a host chunk is (and the label stream must agree)."""
    x = np.asarray(chunk["input"])
    rows = [int(np.flatnonzero((data == x[i].astype(np.uint8)).all(axis=1))[0]) for i in range(x.shape[0])]
    assert np.asarray(chunk["output"]).reshape(-1).tolist() == rows
    return rows


@pytest.mark.parametrize("raw", [True, False])
def test_sequential_disk_access_walks_the_file_and_wraps(rows_file, raw):
    path, data = rows_file
    dh = DataHandler(_config(path, "chunk_size: 10"), raw_chunks=raw)
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    assert dh.host_[0]["input"].dtype == (np.uint8 if raw else np.float32) and dh.host_[0]["output"].dtype == np.float32
    assert (dh.GetDataSetSize(), dh.GetBatchSize(), dh.chunk_size_, dh.fits_on_gpu_) == (23, 2, 10, False)
    want = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [10, 11, 12, 13, 14, 15, 16, 17, 18, 19], [20, 21, 22, 0, 1, 2, 3, 4, 5, 6],
            [7, 8, 9, 10, 11, 12, 13, 14, 15, 16]]
    for chunk in want:
        assert _rows_of(dh.DiskAccess(), data) == chunk
    dh.Seek(21)
    assert _rows_of(dh.DiskAccess(), data) == [21, 22, 0, 1, 2, 3, 4, 5, 6, 7]
    dh.close()


def test_chunk_size_rule_and_max_dataset_size(rows_file):
    path, data = rows_file
    for extra, chunk, fits, size in (("", 23, True, 23), ("chunk_size: 23", 23, False, 23), ("chunk_size: 24", 23, True, 23),
                                     ("max_dataset_size: 9 chunk_size: 10", 9, True, 9), ("max_dataset_size: 40", 23, True, 23)):
        dh = DataHandler(_config(path, extra))
        assert (dh.chunk_size_, dh.fits_on_gpu_, dh.GetDataSetSize()) == (chunk, fits, size), extra
        dh.close()
    dh = DataHandler(_config(path, "max_dataset_size: 9 chunk_size: 6"))
    assert _rows_of(dh.DiskAccess(), data) == [0, 1, 2, 3, 4, 5] and _rows_of(dh.DiskAccess(), data) == [6, 7, 8, 0, 1, 2]
    dh.close()
    with pytest.raises(SystemExit, match="All data streams must have the same size."):
        DataHandler(pbtxt.parse(f'data_config {{ file_pattern: "{path}" layer_name: "input" dataset_name: "x" }}\n'
                                f'data_config {{ file_pattern: "{path}" layer_name: "output" dataset_name: "short" }}', pbtxt.DatasetConfig))


def test_randomize_cpu_reads_runs_of_consecutive_rows(rows_file):
    path, data = rows_file
    dh = DataHandler(_config(path, "chunk_size: 10 randomize_cpu: true random_access_chunk_size: 4"), seed=11)
    starts = []
    for _ in range(9):
        rows = _rows_of(dh.DiskAccess(), data)
        for at in (0, 4, 8):                       # runs of 4 (the last one cut at the chunk's end), consecutive modulo 23
            run = rows[at:at + 4]
            assert run == [(run[0] + k) % ROWS for k in range(len(run))]
            starts.append(run[0])
    # three starts per chunk out of a shuffled list of 23: seven chunks use 21 of them without a repeat, the eighth reshuffles
    assert len(set(starts[:21])) == 21 and len(set(starts[21:])) == 6
    dh.close()
    other = DataHandler(_config(path, "chunk_size: 10 randomize_cpu: true random_access_chunk_size: 4"), seed=12)
    assert _rows_of(other.DiskAccess(), data)[::4] != starts[:3]          # the seed is the constructor's
    other.close()


def test_randomize_cpu_single_rows_over_the_whole_dataset_is_a_permutation(rows_file):
    path, data = rows_file
    dh = DataHandler(_config(path, "randomize_cpu: true random_access_chunk_size: 1"), seed=5)
    first, second = _rows_of(dh.DiskAccess(), data), _rows_of(dh.DiskAccess(), data)
    assert sorted(first) == list(range(ROWS)) and sorted(second) == list(range(ROWS))
    assert first != list(range(ROWS)) and first != second
    dh.close()


def test_preload_thread_fills_the_other_host_buffer_and_is_joined(rows_file):
    import threading
    path, data = rows_file
    before = threading.active_count()
    dh = DataHandler(_config(path, "chunk_size: 10 pipeline_loads: true"))
    dh.AllocateHostMemory(pinned=False)
    assert len(dh.host_) == 2
    dh.StartPreload()
    with pytest.raises(SystemExit, match="previous one is still running"):
        dh.StartPreload()
    dh.Sync()
    assert threading.active_count() == before and _rows_of(dh.host_[dh.pending_], data) == list(range(10))
    dh.StartPreload()
    dh.close()
    assert threading.active_count() == before
    dh = DataHandler(_config(path, "chunk_size: 10 pipeline_loads: true"))
    dh.StartPreload()
    del dh                                          # a collected handler joins its thread
    import gc
    gc.collect()
    assert threading.active_count() == before


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream,message", [
    ("data_type: DUMMY", "data_type DUMMY"), ("data_type: IMAGE_RAW", "data_type IMAGE_RAW"), ("data_type: SLIDING_WINDOW", "data_type SLIDING_WINDOW"),
    ("data_type: TXT", "data_type TXT"), ("data_type: BOUNDING_BOX", "data_type BOUNDING_BOX"), ("data_type: CROPS", "data_type CROPS"),
    ("data_type: VIDEO_RAW", "data_type VIDEO_RAW"), ("is_sequence: true", "is_sequence"), ('noise_layer_name: "output"', "noise_layer_name"),
    ("gpu_id: 1", "gpu_id 1")])
def test_refused_streams_stop_with_their_own_message_naming_the_layer(rows_file, stream, message):
    path, _ = rows_file
    with pytest.raises(SystemExit) as e:
        DataHandler(_config(path, stream=stream))
    assert message in str(e.value) and "layer input" in str(e.value)
    messages = set()
    for s in ("data_type: DUMMY", "data_type: TXT", "is_sequence: true", 'noise_layer_name: "output"', "gpu_id: 1"):
        with pytest.raises(SystemExit) as e:
            DataHandler(_config(path, stream=s))
        messages.add(str(e.value))
    assert len(messages) == 5


def test_parallel_disk_access_is_accepted(rows_file):
    path, data = rows_file
    dh = DataHandler(_config(path, stream="parallel_disk_access: true"))
    assert _rows_of(dh.DiskAccess(), data) == list(range(ROWS))
    dh.close()
