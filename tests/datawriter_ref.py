"""A float64 numpy restatement of the reference's DataWriter::Write / WriteHDF5SeqBuf / WriteHDF5 (src/datawriter.cc:48-152), line by
line, quirks included.  A layer state is an (N, D) array, one case per row (the reference's (N, D) column-major matrix read case by
case); the "file" of a stream is the list ``rows`` of D-vectors.

Quirks kept:
 * with average_online > 1 the loop walks ALL N columns of the batch (a local ``numcases = m_t.GetCols()`` shadows the argument) and
   stops only on ``current_row * average_online < dataset_size`` — dataset_size being cases x multiplicity, NOT divided by
   average_batches;
 * a row written past the end of the dataset (``dataset_size / (average_online * average_batches)`` rows) is the reference's failing
   hyperslab selection followed by exit(1): here ``IndexError``."""
import numpy as np


class Stream:
    def __init__(self, average_batches, average_online):
        self.average_batches, self.average_online = average_batches, average_online
        self.counter = self.consumed = 0
        self.buf = self.seq_buf = None
        self.rows = []

    current_row = property(lambda self: len(self.rows))


class DataWriterRef:
    def __init__(self, streams, dataset_size):
        """``streams``: {name: (average_batches, average_online)}; ``dataset_size``: what SetDataSetSize gets, cases x multiplicity."""
        self.dataset_size_ = dataset_size
        self.streams_ = {name: Stream(p, g) for name, (p, g) in streams.items()}

    def NumRows(self, name):
        s = self.streams_[name]
        return self.dataset_size_ // (s.average_online * s.average_batches)          # SetNumDims (:33)

    def WriteHDF5(self, rows, name):
        s = self.streams_[name]
        if s.current_row + len(rows) > self.NumRows(name):
            raise IndexError(f"{name}: rows {s.current_row}:{s.current_row + len(rows)} of a dataset of {self.NumRows(name)}")
        s.rows.extend(np.array(r, np.float64) for r in rows)

    def WriteHDF5SeqBuf(self, m, name, numcases):
        s = self.streams_[name]
        if s.average_online == 1:
            self.WriteHDF5(m[:numcases], name)
            return
        if s.seq_buf is None:
            s.seq_buf = np.zeros(m.shape[1])
        numcases = m.shape[0]                                                        # (:110) every column, whatever the caller said
        start = 0
        while start < numcases and s.current_row * s.average_online < self.dataset_size_:
            end = min(start + s.average_online - s.consumed, numcases)
            s.seq_buf = s.seq_buf + m[start:end].sum(axis=0) * (1.0 / s.average_online)   # SumCols(buf, 1, 1 / average_online)
            s.consumed += end - start
            if s.consumed == s.average_online:
                self.WriteHDF5([s.seq_buf], name)
                s.seq_buf = np.zeros(m.shape[1])
                s.consumed = 0
            start = end

    def Write(self, states, numcases):
        """``states``: {name: (N, D) array}."""
        for name, m in states.items():
            s, m = self.streams_[name], np.asarray(m, np.float64)
            if s.average_batches == 1:
                self.WriteHDF5SeqBuf(m, name, numcases)
            else:
                s.buf = (np.zeros_like(m) if s.buf is None else s.buf) + m
                s.counter += 1
                if s.counter == s.average_batches:
                    self.WriteHDF5SeqBuf(s.buf / s.average_batches, name, numcases)
                    s.buf, s.counter = None, 0

    def Rows(self, name):
        r = self.streams_[name].rows
        return np.array(r, np.float64).reshape(len(r), -1)


def run_extraction(dataset_size, batch_size, multiplicity, streams, state_of):
    """ConvNet::ExtractFeatures' loop (src/convnet.cc:606-657) over the restatement; ``state_of(name, batch, view)`` -> the (N, D) state
    the net holds for view ``view`` of batch number ``batch`` (which cases a partial last batch is padded with is the handler's business)."""
    w = DataWriterRef(streams, dataset_size * multiplicity)
    num_batches, left_overs = divmod(dataset_size, batch_size)
    if left_overs > 0:
        num_batches += 1
    for k in range(num_batches):
        numcases = left_overs if (left_overs > 0 and k == num_batches - 1) else batch_size
        for view in range(multiplicity):
            w.Write({name: state_of(name, k, view) for name in streams}, numcases)
    return w
