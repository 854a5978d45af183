"""DataWriter (src/datawriter.{h,cc}): the feature file of ``ConvNet.ExtractFeatures(config)`` — one float dataset per feature stream,
named after its layer, ``dataset_size * multiplicity / (average_online * average_batches)`` rows of the layer's dims, created up front
and filled by hyperslab row writes.

Per stream the reference keeps a batch counter (``average_batches`` consecutive ``Write`` calls are summed and divided: the views of a
``multiplicity`` handler), a consumed count (``average_online`` consecutive cases are averaged into one row, across batches) and the
current row.  Here every ``Write`` is ONE ``feature_rows`` launch per stream (csrc/feature_rows.hip): it adds into the stream's sum, or —
on the last pass — leaves the batch's rows in file order, case per row, averaged, in a device buffer that goes to a pinned host buffer in
one contiguous asynchronous copy and from there to the file in one ``H5Dwrite``.

Threads.  Each stream owns two (device rows, pinned host) buffer pairs.  ``Write`` queues launch + copy + an event on the library's
stream; the PREVIOUS batch's events are waited for on the main thread only after the current batch's work has been queued, and its host
buffers then go to the writer thread, which calls libhdf5 (``hdf5io.RowWriter.WriteRows``, under ``hdf5io.LOCK``) and nothing else.  A
host buffer is reused only after the writer thread has released it.  An exception in the writer thread is kept and re-raised on the main
thread by the next ``Write`` or by ``close()``, after the thread has been joined.  ``pipelined=False``: the same launches, waited for and
written on the main thread at once."""
import queue
import threading
from typing import NamedTuple


class StreamPlan(NamedTuple):
    layer: str
    average_batches: int
    average_online: int
    num_dims: int
    num_rows: int


def plan_streams(features, dataset_size, multiplicity, batch_size, dims_of):
    """The streams of a FeatureExtractorConfig's ``feature`` list, checked: [StreamPlan].  ``dataset_size``: cases of the input;
    ``dims_of``: layer name -> dims of its state, or None for a layer the net does not have.  Supported: ``average_batches`` divides
    ``multiplicity`` (otherwise the reference averages different cases with each other) and ``dataset_size * multiplicity /
    average_batches`` is a multiple of ``average_online`` (otherwise the last group never completes).  One more refusal, where the
    reference's loop and the plain reading part ways (NOTES.md): ``average_online > 1`` with a partial last batch and more than one
    averaged batch per input batch (``multiplicity != average_batches``) — the loop walks the padding columns of the partial batch's
    first view into the file and never reaches its later views.  No GPU is needed."""
    features = list(features)
    if not features:
        raise SystemExit("Feature extraction: the config names no feature.")
    plans = []
    for f in features:
        name, P, G = f.layer, f.average_batches, f.average_online
        dims = dims_of(name)
        if dims is None:
            raise SystemExit(f"Feature {name}: the model has no layer of that name.")
        if P < 1 or G < 1:
            raise SystemExit(f"Feature {name}: average_batches {P} and average_online {G} must be at least 1.")
        if multiplicity % P:
            raise SystemExit(f"Feature {name}: average_batches {P} does not divide the input's multiplicity {multiplicity}: "
                             "the averages would mix different cases.")
        passes = dataset_size * multiplicity // P
        if passes % G:
            raise SystemExit(f"Feature {name}: {passes} rows (dataset_size {dataset_size} x multiplicity {multiplicity} / average_batches {P}) "
                             f"are not a multiple of average_online {G}.")
        if G > 1 and dataset_size % batch_size and multiplicity != P:
            raise SystemExit(f"Feature {name}: average_online {G} with a partial last batch ({dataset_size} cases in batches of {batch_size}) "
                             f"and {multiplicity // P} averaged batches per input batch is not supported: the reference's loop would write "
                             "the partial batch's padding columns; choose a batch_size that divides the dataset.")
        if any(p.layer == name for p in plans):
            raise SystemExit(f"Feature {name}: named twice; a file holds one dataset per layer.")
        plans.append(StreamPlan(name, P, G, int(dims), passes // G))
    return plans


class _WriterSide:
    """All the writer thread touches: a queue of (row writer, host rows, first row, release) and the first exception.  No way back to
    the DataWriter, so a writer that is dropped without ``close()`` is collected."""

    def __init__(self):
        self.jobs_ = queue.Queue()
        self.error_ = None

    def Run(self):
        while True:
            job = self.jobs_.get()
            if job is None:
                return
            dataset, rows, row_start, release = job
            try:
                if self.error_ is None:          # after a failure the remaining buffers are released unwritten
                    dataset.WriteRows(rows, row_start)
            except BaseException as e:           # handed to the main thread
                self.error_ = e
            finally:
                release.set()


class _Slot:
    """One of a stream's two buffer pairs."""

    def __init__(self, Matrix, torch, dims, max_rows):
        self.rows_ = Matrix()
        self.rows_.AllocateGPUMemory(dims, max_rows, "feature rows")
        self.host_tensor_ = torch.empty(max_rows * dims, dtype=torch.float32, pin_memory=True)
        self.host_ = self.host_tensor_.numpy()
        self.copied_ = torch.cuda.Event()
        self.free_ = threading.Event()           # set: the writer thread is not reading host_
        self.free_.set()


class _Stream:
    def __init__(self, plan, layer, dataset):
        self.plan_, self.layer_, self.dataset_ = plan, layer, dataset
        self.counter_ = self.consumed_ = self.current_row_ = 0        # the reference's per-stream state (src/datawriter.h)
        self.sum_ = self.carry_ = None
        self.slots_, self.turn_ = [], 0


class DataWriter:
    def __init__(self, config, layers, dataset_size, multiplicity, batch_size, pipelined=True):
        """``layers``: the nets' layers to look the features up in (allocated: their states give dims); ``dataset_size``: cases of the
        input.  Everything is checked before the file is created."""
        import torch
        from . import hdf5io
        from .matrix import Matrix
        by_name = {l.GetName(): l for l in layers}
        plans = plan_streams(config.feature, dataset_size, multiplicity, batch_size,
                             lambda name: by_name[name].GetState().GetCols() if name in by_name else None)
        self.batch_size_, self.pipelined_ = int(batch_size), bool(pipelined)
        self.file_ = hdf5io.File(config.output_file, "w")
        self.streams_ = {}
        self.pending_ = []                       # (stream, slot, first row, rows) of the last Write, not yet handed to the file
        self.side_, self.thread_ = _WriterSide(), None
        self.closed_ = False
        for plan in plans:
            s = self.streams_[plan.layer] = _Stream(plan, by_name[plan.layer], self.file_.CreateRows(plan.layer, plan.num_rows, plan.num_dims))
            N, D, G = self.batch_size_, plan.num_dims, plan.average_online
            if plan.average_batches > 1:
                s.sum_ = Matrix()
                s.sum_.AllocateGPUMemory(N, D, "feature sum")
            if G > 1:
                s.carry_ = Matrix()
                s.carry_.AllocateGPUMemory(D, 1, "feature carry")
                s.carry_.Set(0.0)
            max_rows = N if G == 1 else (G - 1 + N) // G
            s.slots_ = [_Slot(Matrix, torch, D, max(max_rows, 1)) for _ in range(2 if self.pipelined_ else 1)]
        self.Matrix_, self.torch_ = Matrix, torch
        if self.pipelined_:
            self.thread_ = threading.Thread(target=self.side_.Run, name="DataWriter", daemon=True)
            self.thread_.start()

    # ---- DataWriter::Write (src/datawriter.cc:130-152) + WriteHDF5SeqBuf (:96-128) ----
    def Write(self, layers, numcases):
        self._check_writer()
        queued = []
        for l in layers:
            s = self.streams_[l.GetName()]
            p, m = s.plan_, l.GetState()
            P, G = p.average_batches, p.average_online
            if s.counter_ < P - 1:               # buf.Add(m)
                self.Matrix_.FeatureRows(m, s.sum_, s.counter_, P, 0, None, 0, 1, s.slots_[0].rows_)
                s.counter_ += 1
                continue
            if G == 1:
                cases = rows = int(numcases)
                consumed_after = 0
            else:
                # The reference walks ALL columns of the batch here, whatever numcases says, and stops only when the dataset is full,
                # right behind the row that filled it (NOTES.md).
                room = p.num_rows - s.current_row_
                rows = min((s.consumed_ + m.GetRows()) // G, room)
                full = rows == room
                cases = rows * G - s.consumed_ if full else m.GetRows()
                consumed_after = 0 if full else (s.consumed_ + cases) % G
            if cases > 0:
                slot = s.slots_[s.turn_]
                s.turn_ = (s.turn_ + 1) % len(s.slots_)
                self._wait_free(slot)            # the writer thread has let go of this pair's host buffer
                self.Matrix_.FeatureRows(m, s.sum_, s.counter_, P, cases, s.carry_, s.consumed_, G, slot.rows_)
                if rows > 0:
                    n = rows * p.num_dims
                    slot.host_tensor_[:n].copy_(slot.rows_._t[:n], non_blocking=True)
                    slot.copied_.record(self.torch_.cuda.current_stream())
                    queued.append((s, slot, s.current_row_, rows))
                    s.current_row_ += rows
            s.counter_, s.consumed_ = 0, consumed_after
        if not self.pipelined_:
            self._retire(queued)
            return
        self._retire(self.pending_)              # the previous batch: its work has had this batch's launches to finish behind
        self.pending_ = queued

    def _retire(self, jobs):
        for s, slot, row_start, rows in jobs:
            slot.copied_.synchronize()
            data = slot.host_[:rows * s.plan_.num_dims].reshape(rows, s.plan_.num_dims)
            if self.pipelined_:
                slot.free_.clear()
                self.side_.jobs_.put((s.dataset_, data, row_start, slot.free_))
            else:
                s.dataset_.WriteRows(data, row_start)

    def _wait_free(self, slot):
        while not slot.free_.wait(0.05):
            if self.thread_ is None or not self.thread_.is_alive():
                raise RuntimeError("DataWriter: the writer thread is gone while it holds a buffer")
        self._check_writer()

    def _stop_thread(self):
        if self.thread_ is not None:
            self.side_.jobs_.put(None)
            self.thread_.join()
            self.thread_ = None

    def _check_writer(self):
        """Re-raise what the writer thread met, on this thread, with no thread left running and the file closed."""
        if self.closed_:
            raise RuntimeError("DataWriter: Write after close()")
        if self.side_.error_ is not None:
            err, self.side_.error_ = self.side_.error_, None
            self.pending_ = []
            self._shutdown()
            raise err

    def _shutdown(self):
        self._stop_thread()
        self.closed_ = True
        for s in self.streams_.values():
            s.dataset_.close()
        self.file_.close()

    def close(self):
        if self.closed_:
            return
        try:
            pending, self.pending_ = self.pending_, []
            self._retire(pending)
        finally:
            self._shutdown()
        if self.side_.error_ is not None:
            err, self.side_.error_ = self.side_.error_, None
            raise err

    def __del__(self):
        if not getattr(self, "closed_", True):
            try:
                self._shutdown()
            except Exception:
                pass

    def GetRows(self, name):
        """Rows of stream ``name`` handed to the file so far (queued ones included)."""
        return self.streams_[name].current_row_
