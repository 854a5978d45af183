"""HDF5 checkpoint I/O with the reference's on-disk layout, over the HDF5 C library through ctypes
(h5py is not in the image; libhdf5 is — the same library the reference links, Makefile:75).

Mirrors src/util.cc:128-208: ``WriteHDF5CPU`` / ``ReadHDF5CPU`` / ``ReadHDF5Shape`` (2-D float32 datasets; a column-major
(rows, cols) matrix is stored as a row-major (cols, rows) dataset, matrix.cc:419-423) and ``WriteHDF5IntAttr`` /
``ReadHDF5IntAttr`` (scalar int attributes on the file root).  A file written here opens in the reference and vice
versa: names are ``<source>:<dest>:weight``, ``…:bias``, ``…:weight_gradient_history`` with attribute ``…:weight_step``
(edge_with_weight.cc:27-64, optimizer.cc:138-156) plus ``__current_iter__`` / ``__lr_reduce_counter__``
(convnet.cc:672-673,744-749)."""
import ctypes
import ctypes.util
import functools
import os
import threading

import numpy as np

_LIB = None
_T = {}


def _lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    cands = [os.environ.get("CONVNET_HDF5_LIB"), "/opt/conda/lib/libhdf5.so", ctypes.util.find_library("hdf5"), "libhdf5.so"]
    err = None
    for c in cands:
        if not c:
            continue
        try:
            _LIB = ctypes.CDLL(c)
            break
        except OSError as e:
            err = e
    if _LIB is None:
        raise ImportError(f"libhdf5 not found (set CONVNET_HDF5_LIB): {err}")
    L = _LIB
    hid, herr, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    hs = ctypes.POINTER(ctypes.c_uint64)

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype, f.argtypes = res, list(args)

    sig("H5open", herr)
    sig("H5Fcreate", hid, ctypes.c_char_p, ctypes.c_uint, hid, hid)
    sig("H5Fopen", hid, ctypes.c_char_p, ctypes.c_uint, hid)
    sig("H5Fclose", herr, hid)
    sig("H5Screate_simple", hid, ctypes.c_int, hs, hs)
    sig("H5Screate", hid, ctypes.c_int)
    sig("H5Sclose", herr, hid)
    sig("H5Sget_simple_extent_ndims", ctypes.c_int, hid)
    sig("H5Sget_simple_extent_dims", ctypes.c_int, hid, hs, hs)
    sig("H5Dcreate2", hid, hid, ctypes.c_char_p, hid, hid, hid, hid, hid)
    sig("H5Dopen2", hid, hid, ctypes.c_char_p, hid)
    sig("H5Dget_space", hid, hid)
    sig("H5Dwrite", herr, hid, hid, hid, hid, hid, ctypes.c_void_p)
    sig("H5Dread", herr, hid, hid, hid, hid, hid, ctypes.c_void_p)
    sig("H5Dclose", herr, hid)
    sig("H5Lexists", ctypes.c_int, hid, ctypes.c_char_p, hid)
    sig("H5Acreate2", hid, hid, ctypes.c_char_p, hid, hid, hid, hid)
    sig("H5Aopen", hid, hid, ctypes.c_char_p, hid)
    sig("H5Aexists", ctypes.c_int, hid, ctypes.c_char_p)
    sig("H5Awrite", herr, hid, hid, ctypes.c_void_p)
    sig("H5Aread", herr, hid, hid, ctypes.c_void_p)
    sig("H5Aclose", herr, hid)
    sig("H5Eset_auto2", herr, hid, ctypes.c_void_p, ctypes.c_void_p)
    sig("H5Dget_type", hid, hid)
    sig("H5Tget_size", sz, hid)
    sig("H5Tget_class", ctypes.c_int, hid)
    sig("H5Tget_sign", ctypes.c_int, hid)
    sig("H5Tclose", herr, hid)
    sig("H5Pcreate", hid, hid)
    sig("H5Pset_chunk_cache", herr, hid, sz, sz, ctypes.c_double)
    sig("H5Pclose", herr, hid)
    sig("H5Sselect_hyperslab", herr, hid, ctypes.c_int, hs, hs, hs, hs)
    assert L.H5open() >= 0
    L.H5Eset_auto2(0, None, None)      # errors are reported through return codes below, not the library's stderr stack
    _T["float"] = ctypes.c_int64.in_dll(L, "H5T_NATIVE_FLOAT_g").value
    _T["int"] = ctypes.c_int64.in_dll(L, "H5T_NATIVE_INT_g").value
    for dt, sym in _ROW_TYPES.items():
        _T[dt] = ctypes.c_int64.in_dll(L, f"H5T_NATIVE_{sym}_g").value
    _T["dapl"] = ctypes.c_int64.in_dll(L, "H5P_CLS_DATASET_ACCESS_ID_g").value
    return L


H5F_ACC_RDONLY, H5F_ACC_TRUNC, H5P_DEFAULT, H5S_ALL, H5S_SCALAR = 0, 2, 0, 0, 0
H5T_INTEGER, H5T_FLOAT, H5T_SGN_NONE, H5T_SGN_2, H5S_SELECT_SET = 0, 1, 0, 1, 0
# the eight element types of DataIterator::ChooseDataIterator (src/datahandler.cc:361-389): numpy dtype -> libhdf5's native type
_ROW_TYPES = {np.dtype(np.int8): "INT8", np.dtype(np.int32): "INT32", np.dtype(np.int64): "INT64", np.dtype(np.uint8): "UINT8",
              np.dtype(np.uint32): "UINT32", np.dtype(np.uint64): "UINT64", np.dtype(np.float32): "FLOAT", np.dtype(np.float64): "DOUBLE"}


# libhdf5 may be built without thread safety, so no two threads may be inside it at once.  Every method below that enters the library
# holds this one lock for its whole duration — the main thread (checkpoints, means), the data handler's preload thread (RowReader.Get)
# and the data writer's thread (RowWriter.WriteRows) all come through here.  Re-entrant: a method may call another.
LOCK = threading.RLock()


def _serialized(method):
    @functools.wraps(method)
    def locked(*args, **kw):
        with LOCK:
            return method(*args, **kw)
    return locked


class File:
    """``with File(path, "w") as f`` — H5Fcreate(H5F_ACC_TRUNC) / H5Fopen(H5F_ACC_RDONLY) (convnet.cc:668,741)."""

    @_serialized
    def __init__(self, path, mode="r"):
        L = _lib()
        self.path = path
        self.id = (L.H5Fcreate(path.encode(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT) if mode == "w"
                   else L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT))
        if self.id < 0:
            raise OSError(f"cannot {'create' if mode == 'w' else 'open'} HDF5 file {path}")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @_serialized
    def close(self):
        if self.id >= 0:
            _lib().H5Fclose(self.id)
            self.id = -1

    # ---- util.cc:128-138 ----
    @_serialized
    def WriteHDF5CPU(self, mat, rows, cols, name):
        """``mat``: the floats in memory order; stored as a (rows, cols) row-major dataset."""
        L = _lib()
        a = np.ascontiguousarray(mat, np.float32).reshape(-1)
        if a.size != rows * cols:
            raise ValueError("Size mismatch")
        dims = (ctypes.c_uint64 * 2)(rows, cols)
        space = L.H5Screate_simple(2, dims, None)
        ds = L.H5Dcreate2(self.id, name.encode(), _T["float"], space, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT)
        if ds < 0:
            L.H5Sclose(space)
            raise OSError(f"cannot create dataset {name} in {self.path}")
        rc = L.H5Dwrite(ds, _T["float"], H5S_ALL, H5S_ALL, H5P_DEFAULT, a.ctypes.data_as(ctypes.c_void_p))
        L.H5Sclose(space)
        L.H5Dclose(ds)
        if rc < 0:
            raise OSError(f"H5Dwrite failed for {name}")

    @_serialized
    def Has(self, name):
        return _lib().H5Lexists(self.id, name.encode(), H5P_DEFAULT) > 0

    # ---- util.cc:163-175: (rows, cols) of the column-major matrix = (dims[1] or 1, dims[0]) ----
    @_serialized
    def ReadHDF5Shape(self, name):
        L = _lib()
        ds = L.H5Dopen2(self.id, name.encode(), H5P_DEFAULT)
        if ds < 0:
            raise KeyError(f"no dataset {name} in {self.path}")
        space = L.H5Dget_space(ds)
        nd = L.H5Sget_simple_extent_ndims(space)
        dims = (ctypes.c_uint64 * 2)(1, 1)
        L.H5Sget_simple_extent_dims(space, dims, None)
        L.H5Sclose(space)
        L.H5Dclose(ds)
        cols = int(dims[0])
        rows = 1 if nd == 1 else int(dims[1])
        return rows, cols

    # ---- util.cc:188-206 ----
    @_serialized
    def ReadHDF5CPU(self, size, name):
        L = _lib()
        rows, cols = self.ReadHDF5Shape(name)
        if rows * cols != size:
            raise ValueError(f"Dimension mismatch: Expected {size} Got {rows}-{cols}")
        out = np.empty(size, np.float32)
        ds = L.H5Dopen2(self.id, name.encode(), H5P_DEFAULT)
        rc = L.H5Dread(ds, _T["float"], H5S_ALL, H5S_ALL, H5P_DEFAULT, out.ctypes.data_as(ctypes.c_void_p))
        L.H5Dclose(ds)
        if rc < 0:
            raise OSError(f"H5Dread failed for {name}")
        return out

    # ---- util.cc:177-186 / :188-196 ----
    @_serialized
    def WriteHDF5IntAttr(self, name, val):
        L = _lib()
        aid = L.H5Screate(H5S_SCALAR)
        attr = L.H5Acreate2(self.id, name.encode(), _T["int"], aid, H5P_DEFAULT, H5P_DEFAULT)
        v = ctypes.c_int(int(val))
        rc = L.H5Awrite(attr, _T["int"], ctypes.byref(v)) if attr >= 0 else -1
        L.H5Sclose(aid)
        if attr >= 0:
            L.H5Aclose(attr)
        if rc < 0:
            raise OSError(f"cannot write attribute {name}")

    @_serialized
    def ReadHDF5IntAttr(self, name, default):
        """Missing attribute: the reference prints a note and leaves the caller's value untouched."""
        L = _lib()
        if L.H5Aexists(self.id, name.encode()) <= 0:
            return default
        attr = L.H5Aopen(self.id, name.encode(), H5P_DEFAULT)
        v = ctypes.c_int(0)
        L.H5Aread(attr, _T["int"], ctypes.byref(v))
        L.H5Aclose(attr)
        return v.value

    # ---- datasets of rows: what a DataHandler stream reads (src/datahandler.cc:604-721) ----
    @_serialized
    def WriteDataset(self, name, array):
        """A 1-D or 2-D numpy array of one of the eight row types, stored in its own type."""
        L = _lib()
        a = np.ascontiguousarray(array)
        if a.dtype not in _ROW_TYPES or a.ndim not in (1, 2):
            raise ValueError(f"WriteDataset({name}): a 1-D or 2-D array of {sorted(str(d) for d in _ROW_TYPES)} is needed, not {a.dtype} {a.shape}")
        dims = (ctypes.c_uint64 * a.ndim)(*a.shape)
        space = L.H5Screate_simple(a.ndim, dims, None)
        ds = L.H5Dcreate2(self.id, name.encode(), _T[a.dtype], space, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT)
        rc = L.H5Dwrite(ds, _T[a.dtype], H5S_ALL, H5S_ALL, H5P_DEFAULT, a.ctypes.data_as(ctypes.c_void_p)) if ds >= 0 else -1
        L.H5Sclose(space)
        if ds >= 0:
            L.H5Dclose(ds)
        if rc < 0:
            raise OSError(f"cannot write dataset {name} to {self.path}")

    def RowReader(self, name):
        return RowReader(self, name)

    def CreateRows(self, name, num_rows, num_dims, dtype=np.float32):
        """A (num_rows, num_dims) float dataset created empty, to be filled by ``RowWriter.WriteRows`` (DataWriter::SetNumDims,
        src/datawriter.cc:29-45); ``dtype=np.uint8``: an unsigned 8-bit one (apps/image2hdf5.cc)."""
        return RowWriter(self, name, num_rows, num_dims, dtype)


class RowWriter:
    """The write side of a dataset of rows: DataWriter::SetNumDims creates it, DataWriter::WriteHDF5 (src/datawriter.cc:48-94) fills it
    by hyperslabs of consecutive rows."""

    @_serialized
    def __init__(self, file, name, num_rows, num_dims, dtype=np.float32):
        L = _lib()
        self.file_, self.name_, self.num_rows_, self.num_dims_ = file, name, int(num_rows), int(num_dims)
        self.dataset_ = -1
        self.dtype_ = np.dtype(dtype)              # the stored type: float32, or unsigned 8-bit for rows of bytes
        if self.dtype_ not in (np.float32, np.uint8):
            raise ValueError(f"dataset {name}: rows are written as float32 or uint8, not {self.dtype_}")
        dims = (ctypes.c_uint64 * 2)(self.num_rows_, self.num_dims_)
        space = L.H5Screate_simple(2, dims, None)
        self.dataset_ = L.H5Dcreate2(file.id, name.encode(), _T[self.dtype_], space, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT) if space >= 0 else -1
        if space >= 0:
            L.H5Sclose(space)
        if self.dataset_ < 0:
            raise OSError(f"Could not create dataset {name} of {num_rows} x {num_dims} in {file.path}")

    @_serialized
    def WriteRows(self, data, row_start):
        """``data``: a C-contiguous array of whole rows in the dataset's stored type (float32 unless it was created as uint8), written to
        rows ``row_start`` ... of the dataset."""
        L = _lib()
        if not isinstance(data, np.ndarray) or data.dtype != self.dtype_ or not data.flags.c_contiguous or data.size % self.num_dims_:
            raise ValueError(f"dataset {self.name_}: WriteRows needs a contiguous {self.dtype_} array of whole rows of {self.num_dims_}")
        num_rows = data.size // self.num_dims_
        if self.dataset_ < 0:
            raise OSError(f"dataset {self.name_} of {self.file_.path} is closed")
        if row_start < 0 or num_rows <= 0 or row_start + num_rows > self.num_rows_:
            raise IndexError(f"dataset {self.name_}: rows {row_start}:{row_start + num_rows} are not inside its {self.num_rows_} rows")
        start = (ctypes.c_uint64 * 2)(row_start, 0)
        count = (ctypes.c_uint64 * 2)(num_rows, self.num_dims_)
        fspace = L.H5Dget_space(self.dataset_)
        mspace = L.H5Screate_simple(2, count, None)
        rc = L.H5Sselect_hyperslab(fspace, H5S_SELECT_SET, start, None, count, None) if fspace >= 0 and mspace >= 0 else -1
        if rc >= 0:
            rc = L.H5Dwrite(self.dataset_, _T[self.dtype_], mspace, fspace, H5P_DEFAULT, data.ctypes.data_as(ctypes.c_void_p))
        if mspace >= 0:
            L.H5Sclose(mspace)
        if fspace >= 0:
            L.H5Sclose(fspace)
        if rc < 0:
            raise OSError(f"Could not write rows {row_start}:{row_start + num_rows} of {self.name_} to {self.file_.path}")

    @_serialized
    def close(self):
        if self.dataset_ >= 0:
            _lib().H5Dclose(self.dataset_)
            self.dataset_ = -1


class RowReader:
    """HDF5DataIterator<T> (src/datahandler.cc:604-721): the rows of one dataset, read as hyperslabs through a 1 GiB chunk cache.
    ``Get`` fills a caller-owned buffer: a float32 one takes the reference's ``static_cast<float>`` of every element, whatever the
    stored type; a uint8 one takes the bytes as they are and is accepted for an unsigned 8-bit dataset only."""

    @_serialized
    def __init__(self, file, name):
        L = _lib()
        self.file_, self.name_ = file, name
        self.dapl_ = L.H5Pcreate(_T["dapl"])
        L.H5Pset_chunk_cache(self.dapl_, ctypes.c_size_t(-1).value, 1024 * 1024 * 1024, -1.0)   # (:610-613; -1: the library's defaults)
        self.dataset_ = L.H5Dopen2(file.id, name.encode(), self.dapl_)
        if self.dataset_ < 0:
            L.H5Pclose(self.dapl_)
            raise KeyError(f"no dataset {name} in {file.path}")
        space = L.H5Dget_space(self.dataset_)
        self.ndims_ = L.H5Sget_simple_extent_ndims(space)
        dims = (ctypes.c_uint64 * max(self.ndims_, 2))()
        L.H5Sget_simple_extent_dims(space, dims, None)
        L.H5Sclose(space)
        self.dataset_size_ = int(dims[0])
        self.num_dims_ = 1 if self.ndims_ == 1 else int(dims[1])    # (:619)
        t = L.H5Dget_type(self.dataset_)
        cls, size, sign = L.H5Tget_class(t), L.H5Tget_size(t), L.H5Tget_sign(t)
        L.H5Tclose(t)
        kind = {H5T_FLOAT: "f"}.get(cls) or ({H5T_SGN_2: "i", H5T_SGN_NONE: "u"}.get(sign) if cls == H5T_INTEGER else None)
        self.dtype_ = np.dtype(f"{kind}{size}") if kind else None
        if self.ndims_ not in (1, 2) or self.dtype_ not in _ROW_TYPES:
            what = f"{'unsigned ' if kind == 'u' else ''}{ {'f': 'float', 'i': 'integer', 'u': 'integer'}.get(kind, 'class %d' % cls)} of {size} bytes"
            self.close()
            raise TypeError(f"dataset {name} in {file.path}: {self.ndims_}-D {what} is not a type a data stream can read "
                            "(signed or unsigned integers of 1, 4 or 8 bytes, float, double)")
        self.row_ = 0
        self.num_reads_ = 0     # H5Dread calls so far

    @_serialized
    def close(self):
        if self.dataset_ >= 0:
            _lib().H5Dclose(self.dataset_)
            _lib().H5Pclose(self.dapl_)
            self.dataset_ = -1

    def __del__(self):
        if getattr(self, "dataset_", -1) >= 0 and self.file_.id >= 0:
            self.close()

    def GetDataSetSize(self):
        return self.dataset_size_

    def SetMaxDataSetSize(self, max_dataset_size):
        if 0 < max_dataset_size < self.dataset_size_:
            self.dataset_size_ = max_dataset_size

    def GetDims(self):
        return self.num_dims_

    def GetStoredType(self):
        return self.dtype_

    def Seek(self, row):
        self.row_ = row

    def Tell(self):
        return self.row_

    @_serialized
    def Get(self, out, row_start, row_end):
        L = _lib()
        num_rows = row_end - row_start
        if row_start < 0 or row_end < 0 or num_rows <= 0 or row_end > self.dataset_size_:
            raise IndexError(f"Invalid start / end {row_start} {row_end}")
        n = num_rows * self.num_dims_
        if not isinstance(out, np.ndarray) or not out.flags.c_contiguous or out.size < n or out.dtype not in (np.float32, np.uint8):
            raise ValueError(f"dataset {self.name_}: Get needs a contiguous float32 or uint8 buffer of at least {n} elements")
        if out.dtype == np.uint8 and self.dtype_ != np.uint8:
            raise TypeError(f"dataset {self.name_} holds {self.dtype_}: only unsigned 8-bit rows can be read as stored")
        flat = out.reshape(-1)[:n]
        buf = flat if out.dtype == self.dtype_ else np.empty(n, self.dtype_)
        rank = self.ndims_
        start = (ctypes.c_uint64 * rank)(*[row_start, 0][:rank])
        count = (ctypes.c_uint64 * rank)(*[num_rows, self.num_dims_][:rank])
        fspace = L.H5Dget_space(self.dataset_)
        mspace = L.H5Screate_simple(rank, count, None)
        rc = L.H5Sselect_hyperslab(fspace, H5S_SELECT_SET, start, None, count, None)
        if rc >= 0:
            rc = L.H5Dread(self.dataset_, _T[self.dtype_], mspace, fspace, H5P_DEFAULT, buf.ctypes.data_as(ctypes.c_void_p))
        L.H5Sclose(mspace)
        L.H5Sclose(fspace)
        if rc < 0:
            raise OSError(f"Could not read from {row_start}:{row_end} of {self.name_}")
        self.num_reads_ += 1
        if buf is not flat:
            flat[:] = buf      # the reference's static_cast<float> of every element (:701-704)

    def GetNext(self, out):
        self.Get(out, self.row_, self.row_ + 1)
        self.row_ += 1
        if self.row_ == self.dataset_size_:     # (:717-721)
            self.row_ = 0
