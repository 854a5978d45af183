"""Data handlers.  The contract is the reference's (src/datahandler.cc:145-198): ``GetBatch(data_layers)``
leaves a batch in every input layer's ``state_`` (N, X*Y*C CHWN) and every output layer's ``data_``.
``DataHandler`` (below) is the reference's own, for HDF5 streams: built from a DatasetConfig, it reads
chunks from disk and stages batches on the GPU — rows of a dataset, or clips of consecutive frames of one (``is_sequence``); JPEG / video /
text streams are refused.
``ChunkDataHandler`` stages from numpy arrays the caller holds; ``SyntheticDataHandler`` makes noise: inputs are N(0,1) (the real pipeline feeds mean/std-normalised
pixels, :496-507), labels uniform ints stored as float (N,1); ``num_batches`` distinct batches are
pre-generated on the device and cycled, so no host work sits inside a timed step."""
import numpy as np

from .matrix import Matrix


class SyntheticDataHandler:
    def __init__(self, net, batch_size, seed=0, num_batches=2, num_classes=None):
        self.batch_size_ = batch_size
        self.batches_ = []
        self.pos_ = 0
        rng = np.random.default_rng(seed)
        for _ in range(num_batches):
            b = {}
            for l in net.data_layers_:
                if l.IsInput():
                    dims = l.GetSizeY() * l.GetSizeX() * l.GetSizeT() * l.GetNumChannels()
                    m = Matrix()
                    m.AllocateGPUMemory(batch_size, dims)
                    m.FromNumpy(rng.standard_normal((dims, batch_size), dtype=np.float32))
                else:
                    k = num_classes or l.GetNumChannels()
                    m = Matrix()
                    m.AllocateGPUMemory(batch_size, 1)
                    m.FromNumpy(rng.integers(0, k, batch_size).astype(np.float32))
                b[l.GetName()] = m
            self.batches_.append(b)

    def GetBatchSize(self):
        return self.batch_size_

    def GetDataSetSize(self):
        return self.batch_size_ * len(self.batches_)

    def Seek(self, row):
        self.pos_ = row // self.batch_size_

    def Sync(self):
        pass

    def GetBatch(self, data_layers):
        b = self.batches_[self.pos_ % len(self.batches_)]
        self.pos_ += 1
        for l in data_layers:
            (l.GetState() if l.IsInput() else l.GetData()).Set(b[l.GetName()])


class ChunkDataHandler:
    """GPU-resident dataset chunk + per-batch staging on the GPU: DataHandler::GetBatch (src/datahandler.cc:146-198) and
    DataIterator::SampleNoise / AddNoise / Preprocess (:496-570) for one image stream and one label stream.

    The chunk sits on the GPU as a (dims, cases) matrix (one case per column, [colour][row][col] contiguous), exactly
    as the reference keeps it.  Every GetBatch: sample per-case crop offsets and flip bits on the device, then ONE
    ``extract_patches`` (crop + flip + transpose) writes the CHWN batch straight into the input layer's state — or
    ``copy_transpose`` when there is no jitter; when the chunk is exhausted the columns are shuffled in place by a fresh
    permutation (``ShuffleColumns``), images and labels alike.  Mean/std normalisation is applied once when the chunk is
    loaded, like ``DataIterator::Preprocess``.  Disk/HDF5/JPEG loading is not part of this row: ``images`` / ``labels``
    are numpy arrays."""

    def __init__(self, images, labels, batch_size, image_size, crop_size=None, colors=3, translate=True, flip=True, mean=None,
                 std=None, randomize=True, seed=0):
        images = np.ascontiguousarray(images, np.float32)
        self.chunk_size_, dims = images.shape
        assert dims == colors * image_size * image_size and labels.shape[0] == self.chunk_size_
        assert batch_size <= self.chunk_size_
        self.batch_size_ = batch_size
        self.image_size_, self.gpu_image_size_ = image_size, crop_size or image_size
        self.colors_, self.translate_, self.flip_, self.randomize_ = colors, translate, flip, randomize
        self.rng_ = np.random.default_rng(seed)
        # Sequential (non-shuffled) use — validation, feature extraction — reads the dataset round-robin, so the batch that
        # straddles the end continues with the first cases (the reference's chunk loader wraps the same way): keep a copy
        # of the first batch_size cases behind the last one so that window is one contiguous slice.
        pad = 0 if randomize else batch_size
        if pad:
            images = np.concatenate([images, images[:pad]], axis=0)
            labels = np.concatenate([np.asarray(labels).reshape(-1), np.asarray(labels).reshape(-1)[:pad]])
        self.data_ = Matrix()
        self.data_.AllocateGPUMemory(dims, self.chunk_size_ + pad)
        self.data_.FromNumpy(images)                       # numpy (cases, dims) = column-major (dims, cases)
        if mean is not None:                               # DataIterator::Preprocess: m.AddColVec(mean_, -1); m.DivideByColVec(std_)
            self.data_.AddColVec(self._colvec(mean, dims), -1)
            self.data_.DivideByColVec(self._colvec(std, dims))
        self.labels_ = Matrix()
        self.labels_.AllocateGPUMemory(1, self.chunk_size_ + pad)
        self.labels_.FromNumpy(np.asarray(labels, np.float32).reshape(-1))
        self.perm_ = Matrix()
        self.perm_.AllocateGPUMemory(1, self.chunk_size_)
        self.perm_host_ = np.arange(self.chunk_size_, dtype=np.float32)
        self.start_ = 0
        self.width_offset_, self.height_offset_, self.flip_bit_ = Matrix(), Matrix(), Matrix()
        for m in (self.width_offset_, self.height_offset_, self.flip_bit_):
            m.AllocateGPUMemory(1, batch_size)
        self.slice_, self.label_slice_ = Matrix(), Matrix()
        self.multiplicity_counter_ = 0

    @staticmethod
    def _colvec(v, dims):
        m = Matrix()
        m.AllocateGPUMemory(dims, 1)
        m.FromNumpy(np.broadcast_to(np.asarray(v, np.float32).reshape(-1), (dims,)) if np.size(v) != dims else np.asarray(v, np.float32))
        return m

    def GetBatchSize(self):
        return self.batch_size_

    def GetDataSetSize(self):
        return self.chunk_size_

    def Seek(self, row):
        self.start_ = row

    def Sync(self):
        pass

    def _jitter(self):
        return self.image_size_ != self.gpu_image_size_ or self.flip_

    def ShuffleIndices(self):
        # DataHandler::ShuffleIndices (:139-144): random_shuffle of the SAME index array every time, then to the device
        self.rng_.shuffle(self.perm_host_)
        self.perm_.FromNumpy(self.perm_host_)

    def SampleNoise(self):
        # DataIterator::SampleNoise (:533-570)
        if not self._jitter():
            return
        max_off = self.image_size_ - self.gpu_image_size_
        if self.translate_:
            self.height_offset_.FillWithRand()
            self.width_offset_.FillWithRand()
            self.height_offset_.Mult(max_off + 1)          # rounded down by the kernel's int()
            self.width_offset_.Mult(max_off + 1)
        else:                                              # centre / corner patches by multiplicity id
            mid = self.multiplicity_counter_ % 5
            w, h = [(max_off // 2, max_off // 2), (0, 0), (max_off, 0), (max_off, max_off), (0, max_off)][mid]
            self.height_offset_.Set(h)
            self.width_offset_.Set(w)
        if self.flip_:
            self.flip_bit_.FillWithRand()                  # flip if > 0.5
        else:
            self.flip_bit_.Set(self.multiplicity_counter_ // 5)

    def GetBatch(self, data_layers):
        end = self.start_ + self.batch_size_
        if end > self.chunk_size_ and self.randomize_:     # DataHandler::GetBatch :147-166: drop the tail, reshuffle, restart
            self.ShuffleIndices()
            self.data_.ShuffleColumns(self.perm_)
            self.labels_.ShuffleColumns(self.perm_)
            self.start_, end = 0, self.batch_size_
        self.SampleNoise()
        for l in data_layers:
            if l.IsInput():
                self.data_.GetSlice(self.slice_, self.start_, end)
                dest = l.GetState()
                if self._jitter():                         # DataIterator::AddNoise (:520-531)
                    Matrix.ExtractPatches(self.slice_, dest, self.width_offset_, self.height_offset_, self.flip_bit_, self.image_size_,
                                          self.image_size_, self.gpu_image_size_, self.gpu_image_size_)
                else:
                    self.slice_.CopyTranspose(dest)
            else:
                self.labels_.GetSlice(self.label_slice_, self.start_, end)
                self.label_slice_.CopyTranspose(l.GetData())
        self.start_ = end % self.chunk_size_ if not self.randomize_ else end


_REFUSED_TYPES = {
    "DUMMY": "random numbers in place of data", "IMAGE_RAW": "JPEG files decoded and resized on the host",
    "SLIDING_WINDOW": "sliding windows over raw images", "TXT": "text files of numbers", "BOUNDING_BOX": "bounding-box files",
    "CROPS": "crops of raw images", "VIDEO_RAW": "video files decoded on the host"}


class _SequenceReader:
    """SequenceDataIterator (src/datahandler.cc:1100-1200) over a row reader of frames: row ``i`` is the clip of ``seq_length`` frames that
    starts at frame ``row_mapping_[i]`` (its first frame alone with ``pick_first``).  The rest is the row reader's protocol."""

    def __init__(self, base, seq_length, boundary_file, pick_first, layer_name):
        import sys
        self.base_, self.seq_length_, self.pick_first_ = base, seq_length, pick_first
        self.frame_size_ = base.GetDims()
        self.num_dims_ = self.frame_size_ * (1 if pick_first else seq_length)
        frames = base.GetDataSetSize()
        if not boundary_file:
            print("No boundary file found. Assuming entire dataset is one sequence.", file=sys.stderr)
            num_frames = [frames]
        else:
            try:
                with open(boundary_file) as f:
                    num_frames = [int(w) for w in f.read().split()]
            except (OSError, ValueError) as e:
                raise SystemExit(f"Data stream for layer {layer_name}: Could not open boundary file : {boundary_file} ({e})")
            if sum(num_frames) != frames:
                raise SystemExit(f"Data stream for layer {layer_name}: Error: Dataset has {frames} frames but boundary_file adds up to "
                                 f"{sum(num_frames)}")
        self.row_mapping_ = self.SetupRowMapping(num_frames, seq_length)
        self.dataset_size_ = len(self.row_mapping_)
        if self.dataset_size_ == 0:
            raise SystemExit(f"Data stream for layer {layer_name}: no sequence holds seq_length {seq_length} frames.")
        self.row_ = 0

    @staticmethod
    def SetupRowMapping(num_frames, seq_length):
        """(:1158-1173): every frame a whole clip can start at, in dataset order."""
        mapping, start = [], 0
        for num_f in num_frames:
            num_valid_start_pos = num_f - seq_length + 1
            if num_valid_start_pos <= 0:
                print(f"Warning: Number of frames {num_f} is smaller than sequence length {seq_length} for sequence starting at {start}. "
                      "This sequence will be skipped.")
            mapping.extend(range(start, start + max(num_valid_start_pos, 0)))
            start += num_f
        return np.asarray(mapping, np.int64)

    def GetDataSetSize(self):
        return self.dataset_size_

    def SetMaxDataSetSize(self, max_dataset_size):
        self.base_.SetMaxDataSetSize(max_dataset_size)      # the base's alone: the clip count stays (:1198-1200; NOTES.md)

    def GetDims(self):
        return self.num_dims_

    def GetStoredType(self):
        return self.base_.GetStoredType()

    @property
    def num_reads_(self):
        return self.base_.num_reads_

    def Seek(self, row):
        self.row_ = row

    def Tell(self):
        return self.row_

    def Get(self, out, row_start, row_end):
        """Row by row, as DataIterator::Get(start, end) (:578-583): one read of the base per clip."""
        if row_start < 0 or row_end <= row_start or row_end > self.dataset_size_:
            raise IndexError(f"Asking for row {row_start} {row_end}")
        rows = out.reshape(-1)[:(row_end - row_start) * self.num_dims_].reshape(row_end - row_start, self.num_dims_)
        for i, row in enumerate(range(row_start, row_end)):
            mapped = int(self.row_mapping_[row])
            self.base_.Get(rows[i], mapped, mapped + (1 if self.pick_first_ else self.seq_length_))

    def close(self):
        self.base_.close()


def _run_frames(row_mapping, seq_length, length):
    """The most frames a run of ``length`` consecutive clip rows lays into a frame buffer, over every row it can start at.  A clip adds the
    frames its predecessor did not hold: min(seq_length, gap to it) — the mapping is increasing — and a whole clip behind the wrap to row
    0; prefix sums of that over the doubled list give every start's total."""
    gaps = np.append(np.minimum(np.diff(row_mapping), seq_length), seq_length)
    sums = np.concatenate([[0], np.cumsum(np.concatenate([gaps, gaps]))])
    starts = np.arange(len(row_mapping))
    return int(seq_length + (sums[starts + length - 1] - sums[starts]).max())


class _Stream:
    """DataIterator + HDF5DataIterator<T> for one ``data_config`` (src/datahandler.cc:415-570, 604-721)."""

    def __init__(self, dsc):
        from . import hdf5io
        name = dsc.layer_name
        if dsc.is_sequence and dsc.seq_length < 1:
            raise SystemExit(f"Data stream for layer {name}: is_sequence needs a seq_length of at least 1, not {dsc.seq_length}.")
        if dsc.is_sequence and dsc.pca_noise_stddev > 0:
            raise SystemExit(f"Data stream for layer {name}: pca_noise_stddev is not supported on a sequence stream: the colour noise "
                             "has 3 columns, a clip 3 x seq_length planes.")
        if dsc.data_type != "HDF5":
            what = _REFUSED_TYPES.get(dsc.data_type)
            if what is None:
                raise SystemExit(f"Data stream for layer {name}: Unknown data type {dsc.data_type}")
            raise SystemExit(f"Data stream for layer {name}: data_type {dsc.data_type} ({what}) is not supported; only HDF5 streams are.")
        if dsc.noise_layer_name:
            raise SystemExit(f"Data stream for layer {name}: noise_layer_name ({dsc.noise_layer_name}) is not supported: "
                             "no stream takes its jitter from another.")
        if dsc.gpu_id != 0:
            raise SystemExit(f"Data stream for layer {name}: gpu_id {dsc.gpu_id} is not supported: one process drives one GPU, gpu_id 0.")
        self.config_, self.layer_name_ = dsc, name
        self.file_ = hdf5io.File(dsc.file_pattern)
        self.reader_ = self.file_.RowReader(dsc.dataset_name)
        self.frame_size_, self.frames_ = self.reader_.GetDims(), 1      # a row is frames_ frames of frame_size_ values
        self.is_sequence_, self.frames_once_ = dsc.is_sequence, False
        if dsc.is_sequence:
            try:
                self.reader_ = _SequenceReader(self.reader_, dsc.seq_length, dsc.boundary_file, dsc.pick_first, name)
            except BaseException:
                self.close()
                raise
            self.frames_ = 1 if dsc.pick_first else dsc.seq_length
        self.image_size_y_ = dsc.image_size_y if dsc.has_image_size_y() else dsc.image_size
        self.image_size_x_ = dsc.image_size_x if dsc.has_image_size_x() else dsc.image_size
        self.gpu_image_size_y_ = dsc.gpu_image_size_y if dsc.has_gpu_image_size_y() else self.image_size_y_
        self.gpu_image_size_x_ = dsc.gpu_image_size_x if dsc.has_gpu_image_size_x() else self.image_size_x_
        self.num_colors_, self.translate_, self.flip_ = dsc.num_colors, dsc.can_translate, dsc.can_flip
        self.normalize_ = dsc.normalize or dsc.pixelwise_normalize
        self.pixelwise_normalize_, self.normalize_local_ = dsc.pixelwise_normalize, dsc.normalize_local
        self.pca_noise_stddev_ = dsc.pca_noise_stddev
        self.add_pca_noise_ = dsc.pca_noise_stddev > 0
        self.raw_ = False            # the chunk form: bytes (True) or float (DataHandler.SetInputLayers decides)
        self.mean_ = self.std_ = None
        self.width_offset_, self.height_offset_, self.flip_bit_ = Matrix(), Matrix(), Matrix()
        self.pca_noise1_, self.pca_noise2_ = Matrix(), Matrix()
        self.slice_, self.index_slice_ = Matrix(), Matrix()

    def GetDims(self):
        return self.reader_.GetDims()

    def Jitters(self):
        return self.image_size_y_ != self.gpu_image_size_y_ or self.image_size_x_ != self.gpu_image_size_x_ or self.flip_

    def StagedDims(self):
        """The width of the batch this stream leaves in its layer."""
        return self.frames_ * self.num_colors_ * self.gpu_image_size_y_ * self.gpu_image_size_x_ if self.Jitters() else self.GetDims()

    def CheckGeometry(self):
        if self.Jitters() and self.frame_size_ != self.num_colors_ * self.image_size_y_ * self.image_size_x_:
            what = "frames" if self.is_sequence_ else "rows"
            raise SystemExit(f"Data stream for layer {self.layer_name_}: {what} of {self.frame_size_} values are not {self.num_colors_} colours of "
                             f"{self.image_size_y_} x {self.image_size_x_} pixels.")
        if self.gpu_image_size_y_ > self.image_size_y_ or self.gpu_image_size_x_ > self.image_size_x_:
            raise SystemExit(f"Data stream for layer {self.layer_name_}: gpu_image_size exceeds image_size.")

    # ---- DataIterator::LoadMeans (:445-474) ----
    def LoadMeans(self):
        from . import hdf5io
        dims = self.frame_size_                # a sequence stream's mean / std are its base stream's: per FRAME pixel (:1152-1156)
        with hdf5io.File(self.config_.mean_file) as f:
            if self.pixelwise_normalize_:
                # mean_ = zeros(num_pixels, num_channels) + the row vector pixel_mean, reshaped to a column: every channel's value repeated
                # over its pixels (0 + x is exact, so the host does it)
                pm, ps = (f.ReadHDF5CPU(int(np.prod(f.ReadHDF5Shape(n))), n) for n in ("pixel_mean", "pixel_std"))
                if pm.size == 0 or dims % pm.size or ps.size != pm.size:
                    raise SystemExit(f"Data stream for layer {self.layer_name_}: pixel_mean of {pm.size} channels does not divide {dims} dims.")
                mean, std = np.repeat(pm, dims // pm.size), np.repeat(ps, dims // pm.size)
                if self.add_pca_noise_:
                    self.eig_values_, self.eig_vectors_ = Matrix(), Matrix()
                    self.eig_values_.AllocateAndReadHDF5(f, "S")
                    self.eig_vectors_.AllocateAndReadHDF5(f, "U")
            else:
                mean, std = f.ReadHDF5CPU(dims, "mean"), f.ReadHDF5CPU(dims, "std")
        self.mean_, self.std_ = Matrix(), Matrix()
        for m, v in ((self.mean_, mean), (self.std_, std)):
            m.AllocateGPUMemory(dims, 1, "normalizer")
            m.FromNumpy(v)

    # ---- DataIterator::Preprocess (:496-507): the float chunk, once per load ----
    def Preprocess(self, m):
        if self.frames_ > 1:                   # SequenceDataIterator::Preprocess (:1152-1156): the base stream's, frame by frame
            m.Reshape(self.frame_size_, -1)
            self._preprocess_frames(m)
            m.Reshape(self.frame_size_ * self.frames_, -1)
        else:
            self._preprocess_frames(m)

    def _preprocess_frames(self, m):
        if self.normalize_local_:
            dims = m.GetRows()
            m.Reshape(dims // self.num_colors_, -1)
            m.NormalizeColumnwise()
            m.Reshape(dims, -1)
        if self.normalize_:
            m.AddColVec(self.mean_, -1)
            m.DivideByColVec(self.std_)

    # ---- DataIterator::SampleNoise (:534-570) ----
    def SampleNoise(self, batch_size, multiplicity_id):
        if not self.Jitters():
            return
        max_offset_y = self.image_size_y_ - self.gpu_image_size_y_
        max_offset_x = self.image_size_x_ - self.gpu_image_size_x_
        if self.width_offset_.GetCols() != batch_size:
            for m in (self.width_offset_, self.height_offset_, self.flip_bit_):
                m.AllocateGPUMemory(1, batch_size)
        if self.translate_:
            self.height_offset_.FillWithRand()
            self.width_offset_.FillWithRand()
            self.height_offset_.Mult(max_offset_y + 1)
            self.width_offset_.Mult(max_offset_x + 1)
        else:
            w, h = [(max_offset_x // 2, max_offset_y // 2), (0, 0), (max_offset_x, 0), (max_offset_x, max_offset_y),
                    (0, max_offset_y)][multiplicity_id % 5]
            self.height_offset_.Set(h)
            self.width_offset_.Set(w)
        if self.flip_:
            self.flip_bit_.FillWithRand()
        else:
            self.flip_bit_.Set(multiplicity_id // 5)

    # ---- DataIterator::AddPCANoise (:509-518) ----
    def AddPCANoise(self, m):
        if self.pca_noise1_.GetRows() != m.GetRows():
            self.pca_noise1_.AllocateGPUMemory(m.GetRows(), self.eig_vectors_.GetRows())
            self.pca_noise2_.AllocateGPUMemory(m.GetRows(), self.eig_vectors_.GetCols())
        self.pca_noise1_.FillWithRandn()
        self.pca_noise1_.MultByRowVec(self.eig_values_)
        Matrix.Dot(self.pca_noise1_, self.eig_vectors_, self.pca_noise2_, 0, 1)
        m.AddToEachPixel(self.pca_noise2_, self.pca_noise_stddev_)

    # ---- DataIterator::AddNoise (:520-532), from either chunk form ----
    def AddNoise(self, handler, start, end, output):
        jit = self.Jitters()
        if self.frames_once_:
            name, fs = self.layer_name_, self.frame_size_
            handler.first_frame_dev_[name].GetSlice(self.index_slice_, start, end)
            used = handler.frames_used_[name]
            offs = (self.width_offset_, self.height_offset_, self.flip_bit_) if jit else (None, None, None)
            geom = ((self.image_size_y_, self.image_size_x_, self.gpu_image_size_y_, self.gpu_image_size_x_) if jit else (1, fs, 1, fs))
            Matrix.StageClipsU8(handler.raw_data_[name][:used * fs], fs, used, self.index_slice_, self.frames_,
                                self.mean_ if self.normalize_ else None, self.std_ if self.normalize_ else None, output, *offs, *geom)
        elif self.raw_:
            handler.col_index_dev_.GetSlice(self.index_slice_, start, end)
            dims = self.GetDims()
            offs = (self.width_offset_, self.height_offset_, self.flip_bit_) if jit else (None, None, None)
            # no jitter: a transpose of whole rows, whatever image_size says (the reference's CopyTranspose)
            geom = ((self.image_size_y_, self.image_size_x_, self.gpu_image_size_y_, self.gpu_image_size_x_) if jit else (1, dims, 1, dims))
            Matrix.StagePatchesU8(handler.raw_data_[self.layer_name_], dims, handler.chunk_size_, self.index_slice_,
                                  self.mean_ if self.normalize_ else None, self.std_ if self.normalize_ else None, output, *offs, *geom)
        else:
            handler.data_[self.layer_name_].GetSlice(self.slice_, start, end)
            if jit:
                Matrix.ExtractPatches(self.slice_, output, self.width_offset_, self.height_offset_, self.flip_bit_, self.image_size_y_,
                                      self.image_size_x_, self.gpu_image_size_y_, self.gpu_image_size_x_)
            else:
                self.slice_.CopyTranspose(output)
        if self.add_pca_noise_:
            self.AddPCANoise(output)

    def close(self):
        self.reader_.close()
        self.file_.close()


class _DiskSide:
    """DataHandler::DiskAccess / LoadChunk (src/datahandler.cc:239-314): everything the preload thread touches — the row readers, the
    host buffers and the random-row list.  libhdf5 and numpy only: no GPU call, no ``Matrix``, and no way back to the handler, so a
    handler that is dropped while a preload runs is collected (and joins the thread) at once."""

    def __init__(self, readers, chunk_size, dataset_size, randomize_cpu, random_access_chunk_size, rng):
        self.readers_ = readers              # layer name -> RowReader, in data_config order
        self.chunk_size_, self.dataset_size_ = chunk_size, dataset_size
        self.randomize_cpu_, self.random_access_chunk_size_ = randomize_cpu, random_access_chunk_size
        self.rng_ = rng
        self.random_indices_ind_ = 0
        if randomize_cpu:
            self.random_indices_ = rng.permutation(dataset_size)
        self.host_ = None                    # [buffer][layer name] -> (chunk_size, dims) array
        self.error_ = None
        # frames-once streams (sequence streams that keep their bytes): host_ holds (frames, frame_size) — every frame of a run once —
        self.frames_once_ = set()            # their layer names
        self.first_frame_ = None             # [buffer][layer name] -> (chunk_size,) float32: the buffer row of every clip's first frame
        self.frames_used_ = None             # [buffer][layer name] -> how many rows of host_ the chunk filled

    def Preload(self, buf):
        try:
            self.DiskAccess(buf)
        except BaseException as e:           # handed to the thread that joins
            self.error_ = e

    def DiskAccess(self, buf):
        random_rows = None
        if self.randomize_cpu_:
            num_rand = (self.chunk_size_ + self.random_access_chunk_size_ - 1) // self.random_access_chunk_size_
            if self.random_indices_ind_ + num_rand > self.dataset_size_:     # (:241-246)
                self.rng_.shuffle(self.random_indices_)
                self.random_indices_ind_ = 0
            random_rows = self.random_indices_[self.random_indices_ind_:self.random_indices_ind_ + num_rand].tolist()
            self.random_indices_ind_ += num_rand
        for name, reader in self.readers_.items():
            out = self.host_[buf][name]
            once = name in self.frames_once_
            load = self._lay_run if once else self._load_run
            if once:
                out = (out, self.first_frame_[buf][name], [0])
            if random_rows is None:
                load(reader, out, 0, reader.Tell(), self.chunk_size_, seek=True)
            else:
                for i, row in enumerate(random_rows):
                    at = i * self.random_access_chunk_size_
                    # (the last run stops at the end of the chunk: the reference reads a whole run there, past its buffer)
                    load(reader, out, at, row, min(self.random_access_chunk_size_, self.chunk_size_ - at))
            if once:
                self.frames_used_[buf][name] = out[2][0]
        return self.host_[buf]

    def _load_run(self, reader, out, at, row, count, seek=False):
        """``count`` consecutive rows from ``row``, wrapping at the end of the dataset (GetNext's wrap, :717-721; LoadChunk's, :305-311)."""
        size = self.dataset_size_
        while count > 0:
            n = min(count, size - row)
            reader.Get(out[at:at + n], row, row + n)
            at, count, row = at + n, count - n, (row + n) % size
        if seek:
            reader.Seek(row)

    def _lay_run(self, reader, out, at, row, count, seek=False):
        """The same run of clip rows for a frames-once stream: the union of the clips' frame ranges goes behind what the buffer holds,
        in dataset order and every frame once; clips ``at`` ... of the table get the buffer row of their first frame.  A piece — one
        hyperslab read — ends where the next clip does not start one frame on: at a sequence boundary, at a skipped sequence, at the wrap
        to row 0."""
        frames, table, filled = out
        mapping, T, size = reader.row_mapping_, reader.seq_length_, self.dataset_size_
        while count > 0:
            n = min(count, size - row)
            m = mapping[row:row + n]
            cuts = np.flatnonzero(np.diff(m) != 1) + 1
            for a, b in zip([0, *cuts.tolist()], [*cuts.tolist(), n]):
                lo, hi = int(m[a]), int(m[b - 1]) + T
                reader.base_.Get(frames[filled[0]:filled[0] + hi - lo], lo, hi)
                table[at + a:at + b] = filled[0] + (m[a:b] - lo)
                filled[0] += hi - lo
            at, count, row = at + n, count - n, (row + n) % size
        if seek:
            reader.Seek(row)


class DataHandler:
    """DataHandler for HDF5 streams, built from a ``pbtxt.DatasetConfig`` (src/datahandler.cc:8-336): chunks of the dataset are read
    from disk (sequentially, or ``randomize_cpu`` in runs of ``random_access_chunk_size`` rows), copied to the GPU, and every
    ``GetBatch`` stages one batch from the resident chunk into the data layers.

    Two chunk forms per stream.  **float** is the reference's: rows are cast to float on the host, the chunk is a (dims, cases)
    ``Matrix``, ``Preprocess`` normalises all of it at load, ``randomize_gpu`` swaps its columns, and a batch is ``ExtractPatches`` /
    ``CopyTranspose`` of a slice.  **bytes** — taken when the dataset is stored as unsigned 8-bit, its layer is an input layer and
    ``normalize_local`` is off — keeps the chunk on the GPU exactly as read (a ``torch.uint8`` tensor, a quarter of the transfer and of
    the memory); nothing touches it after the copy, ``randomize_gpu`` swaps entries of a column index instead, and a batch is ONE
    ``StagePatchesU8``: cast, mean / std, crop, flip and transpose together, bit for bit what the float form leaves.
    ``raw_chunks=False`` forces the float form everywhere.

    A sequence stream (``is_sequence``, ``seq_length`` T) reads clips: its float form is the reference's, one materialised clip of T frames
    per column.  Its bytes form (the same conditions, and not ``pick_first``) keeps every frame of a run of consecutive clip rows ONCE —
    the union of the clips' frame ranges, in dataset order — beside a table of the buffer column of every clip's first frame;
    ``randomize_gpu`` swaps entries of that table, and a batch is ONE ``StageClipsU8`` that gathers each clip's T consecutive columns.
    The buffers are sized once, to the exact worst case over run starts (``FrameBufferSize``); only the used prefix is uploaded.

    The two host RNGs (random rows, column permutation) are numpy generators seeded from ``seed``; the device RNG calls are the
    library's, in the reference's order.  ``pipeline_loads``: one preload thread reads the next chunk into the idle one of two pinned
    host buffers; it calls libhdf5 and nothing else."""

    def __init__(self, config, raw_chunks=True, seed=0):
        self.config_ = config
        self.raw_chunks_ = bool(raw_chunks)
        self.preload_thread_ = None
        self.batch_size_, self.chunk_size_ = config.batch_size, config.chunk_size
        self.max_reuse_count_, self.reuse_counter_ = config.max_reuse_count, 0
        self.random_access_chunk_size_ = max(config.random_access_chunk_size, 1)
        self.dataset_size_ = -1
        self.start_ = self.multiplicity_counter_ = 0
        self.restart_, self.nothing_on_gpu_, self.fits_on_gpu_ = True, True, False
        self.pipeline_loads_, self.randomize_cpu_, self.randomize_gpu_ = config.pipeline_loads, config.randomize_cpu, config.randomize_gpu
        self.multiplicity_ = config.multiplicity
        self.row_rng_, self.perm_rng_ = (np.random.default_rng(s) for s in np.random.SeedSequence(seed).spawn(2))
        self.layer_names_, self.streams_ = [], {}
        for dsc in config.data_config:
            st = _Stream(dsc)
            self.layer_names_.append(dsc.layer_name)
            self.streams_[dsc.layer_name] = st
            st.reader_.SetMaxDataSetSize(config.max_dataset_size)
            size = st.reader_.GetDataSetSize()
            if self.dataset_size_ == -1:
                self.dataset_size_ = size
            elif size != self.dataset_size_:
                raise SystemExit("All data streams must have the same size.")
            st.CheckGeometry()
        if not self.streams_:
            raise SystemExit("Error: the dataset has no data_config.")
        if self.chunk_size_ <= 0 or self.chunk_size_ > self.dataset_size_:
            self.chunk_size_, self.fits_on_gpu_ = self.dataset_size_, True
        if self.batch_size_ > self.chunk_size_:
            raise SystemExit(f"batch_size {self.batch_size_} exceeds the chunk of {self.chunk_size_} cases.")
        self.disk_ = _DiskSide({n: self.streams_[n].reader_ for n in self.layer_names_}, self.chunk_size_, self.dataset_size_,
                               self.randomize_cpu_, self.random_access_chunk_size_, self.row_rng_)
        self.perm_host_ = np.arange(self.chunk_size_, dtype=np.float32)     # SetupShuffler: shuffled in place, again and again
        self.col_index_ = np.arange(self.chunk_size_, dtype=np.float32)     # bytes form: where each column of the chunk sits now
        self.data_, self.raw_data_ = {}, {}  # layer name -> device chunk (Matrix (dims, chunk) / torch.uint8 tensor)
        # frames-once streams: where every clip's first frame sits in raw_data_ (host copy, device copy) and how many frames that holds
        self.first_frame_, self.first_frame_dev_, self.frames_used_ = {}, {}, {}
        self.input_layers_set_ = self.allocated_ = False
        self.copy_done_ = [None, None]       # per host buffer: the event behind the last copy that read it
        self.last_copied_, self.pending_ = -1, 0
        self.Seek(0)

    # ---- which streams keep their bytes ----
    def SetInputLayers(self, names):
        for name, st in self.streams_.items():
            st.raw_ = (self.raw_chunks_ and name in names and st.reader_.GetStoredType() == np.uint8 and not st.normalize_local_
                       and not (st.is_sequence_ and st.config_.pick_first))
            st.frames_once_ = st.raw_ and st.is_sequence_
            if st.frames_once_ and self.FrameBufferSize(name) > 1 << 24:
                raise SystemExit(f"Data stream for layer {name}: a byte chunk of more than 2^24 frames cannot be indexed; set chunk_size.")
            if st.raw_ and self.chunk_size_ > 1 << 24:
                raise SystemExit(f"Data stream for layer {name}: a byte chunk of more than 2^24 cases cannot be indexed; set chunk_size.")
        self.disk_.frames_once_ = {name for name, st in self.streams_.items() if st.frames_once_}
        self.input_layers_set_ = True

    def FrameBufferSize(self, name):
        """The frames a chunk of a frames-once stream can need at the most: the exact worst case over the rows its runs can start at —
        one run of the whole chunk read sequentially, ``random_access_chunk_size`` rows each (the last one cut at the chunk's end) under
        ``randomize_cpu``.  Runs follow each other in the buffer, so their worst cases add up."""
        r = self.streams_[name].reader_
        if not self.randomize_cpu_:
            return _run_frames(r.row_mapping_, r.seq_length_, self.chunk_size_)
        whole, last = divmod(self.chunk_size_, self.random_access_chunk_size_)
        return (whole * _run_frames(r.row_mapping_, r.seq_length_, min(self.random_access_chunk_size_, self.chunk_size_)) if whole else 0) + \
            (_run_frames(r.row_mapping_, r.seq_length_, last) if last else 0)

    def AllocateHostMemory(self, pinned=True):
        """One host buffer per stream, two with ``pipeline_loads``; ``pinned=False`` gives plain numpy arrays (no GPU needed)."""
        if not self.input_layers_set_:
            self.SetInputLayers(())
        host, self.host_tensors_ = [], []
        sizes = {name: self.FrameBufferSize(name) for name, st in self.streams_.items() if st.frames_once_}    # once: here
        self.disk_.first_frame_, self.disk_.frames_used_ = [], []
        for _ in range(2 if self.pipeline_loads_ else 1):
            arrays, tensors = {}, {}
            self.disk_.first_frame_.append({name: np.zeros(self.chunk_size_, np.float32) for name in sizes})
            self.disk_.frames_used_.append({name: 0 for name in sizes})
            for name, st in self.streams_.items():
                shape, dtype = (self.chunk_size_, st.GetDims()), (np.uint8 if st.raw_ else np.float32)
                if st.frames_once_:
                    shape = (sizes[name], st.frame_size_)
                if pinned:
                    import torch
                    tensors[name] = torch.empty(shape, dtype=torch.uint8 if st.raw_ else torch.float32, pin_memory=True)
                    arrays[name] = tensors[name].numpy()
                else:
                    arrays[name] = np.zeros(shape, dtype)
            host.append(arrays)
            self.host_tensors_.append(tensors)
        self.disk_.host_ = host

    def AllocateMemory(self):
        import torch
        self.AllocateHostMemory(pinned=True)
        for name, st in self.streams_.items():
            if st.frames_once_:              # (the host buffer's size: the worst case, allocated once)
                self.raw_data_[name] = torch.empty(self.host_[0][name].size, dtype=torch.uint8, device=Matrix()._dev())
                self.first_frame_[name] = np.zeros(self.chunk_size_, np.float32)
                self.first_frame_dev_[name] = Matrix()
                self.first_frame_dev_[name].AllocateGPUMemory(1, self.chunk_size_)
                self.frames_used_[name] = 0
            elif st.raw_:
                self.raw_data_[name] = torch.empty(self.chunk_size_ * st.GetDims(), dtype=torch.uint8, device=Matrix()._dev())
            else:
                self.data_[name] = Matrix()
                self.data_[name].AllocateGPUMemory(st.GetDims(), self.chunk_size_, "databuffer")
            if st.normalize_:
                st.LoadMeans()
            elif st.add_pca_noise_:
                raise SystemExit(f"Data stream for layer {name}: pca_noise_stddev needs pixelwise_normalize (S and U come from mean_file).")
        if self.randomize_gpu_:
            self.rand_perm_indices_ = Matrix()
            self.rand_perm_indices_.AllocateGPUMemory(1, self.chunk_size_)
        if any(st.raw_ and not st.frames_once_ for st in self.streams_.values()):
            self.col_index_dev_ = Matrix()
            self.col_index_dev_.AllocateGPUMemory(1, self.chunk_size_)
            self.col_index_dev_.FromNumpy(self.col_index_)
        self.copy_done_ = [torch.cuda.Event() for _ in self.host_]
        self.allocated_ = True

    # ---- the trainer's protocol ----
    def GetBatchSize(self):
        return self.batch_size_

    def GetDataSetSize(self):
        return self.dataset_size_

    def GetDims(self, layer_name):
        if layer_name not in self.streams_:
            raise SystemExit(f"Layer name {layer_name} not found.")
        return self.streams_[layer_name].GetDims()

    def Seek(self, row):
        self.Sync()
        self.start_ = row
        self.reuse_counter_ = self.multiplicity_counter_ = 0
        self.restart_ = True
        for st in self.streams_.values():
            st.reader_.Seek(row)

    def Sync(self):
        if self.pipeline_loads_:
            self.WaitForPreload()

    def close(self):
        self.WaitForPreload()
        for st in self.streams_.values():
            st.close()

    def __del__(self):
        t = getattr(self, "preload_thread_", None)
        if t is not None:
            t.join()

    # ---- DataHandler::ShuffleIndices + the column shuffle (:139-144, 158-165) ----
    def ShuffleIndices(self):
        self.perm_rng_.shuffle(self.perm_host_)
        self.rand_perm_indices_.FromNumpy(self.perm_host_)

    def _shuffle_columns(self, data_layers):
        self.ShuffleIndices()
        for l in data_layers:
            if l.GetName() in self.data_:
                self.data_[l.GetName()].ShuffleColumns(self.rand_perm_indices_)
        if self.raw_data_:
            # shuffleColumns swaps columns idx[2j] and idx[2j+1] for every pair; a permutation's pairs are disjoint.  The byte chunk
            # stays where it is: the same swaps go to the index of where each column sits
            pairs = self.perm_host_[:2 * (self.chunk_size_ // 2)].astype(np.int64)
            a, b = pairs[0::2], pairs[1::2]
            if len(self.raw_data_) > len(self.first_frame_):
                self.col_index_[a], self.col_index_[b] = self.col_index_[b].copy(), self.col_index_[a].copy()
                self.col_index_dev_.FromNumpy(self.col_index_)
            for name, table in self.first_frame_.items():        # a frames-once stream: the same swaps on its first-frame table
                table[a], table[b] = table[b].copy(), table[a].copy()
                self.first_frame_dev_[name].FromNumpy(table)

    # ---- DataHandler::GetBatch (:146-200) ----
    def GetBatch(self, data_layers):
        if not self.allocated_:
            if not self.input_layers_set_:
                self.SetInputLayers([l.GetName() for l in data_layers if l.IsInput()])
            self.AllocateMemory()
        end = self.start_ + self.batch_size_
        if end > self.chunk_size_ or self.restart_:
            if self.reuse_counter_ < self.max_reuse_count_ and not self.restart_:
                self.reuse_counter_ += 1
            elif self.nothing_on_gpu_ or not self.fits_on_gpu_:
                if self.restart_ and self.pipeline_loads_:
                    self.StartPreload()
                self.nothing_on_gpu_ = False
                self.reuse_counter_ = 0
                self.PipelinedDiskAccess()
            self.restart_ = False
            if self.randomize_gpu_:
                self._shuffle_columns(data_layers)
            self.start_, end = 0, self.batch_size_
        streams = [(l, self.streams_[l.GetName()]) for l in data_layers if l.GetName() in self.streams_]
        for l, st in streams:            # all the noise first: a layer may need another's (:170-181)
            st.SampleNoise(self.batch_size_, self.multiplicity_counter_)
        for l, st in streams:
            st.AddNoise(self, self.start_, end, l.GetState() if l.IsInput() else l.GetData())
        self.multiplicity_counter_ += 1
        if self.multiplicity_counter_ == self.multiplicity_:
            self.multiplicity_counter_ = 0
            self.start_ = end

    # ---- DataHandler::PipelinedDiskAccess / StartPreload / WaitForPreload (:202-237) ----
    def PipelinedDiskAccess(self):
        import torch
        if self.pipeline_loads_:
            self.WaitForPreload()
            buf = self.pending_
        else:
            buf = 0
            self.copy_done_[0].synchronize()     # the last copy out of this buffer
            self.DiskAccess(0)
        for name, st in self.streams_.items():   # on the stream the step runs on
            src = self.host_tensors_[buf][name].view(-1)
            if st.frames_once_:                  # the used prefix alone, and the table that goes with it
                used = self.frames_used_[name] = self.disk_.frames_used_[buf][name]
                self.raw_data_[name][:used * st.frame_size_].copy_(src[:used * st.frame_size_], non_blocking=True)
                self.first_frame_[name][:] = self.disk_.first_frame_[buf][name]
                self.first_frame_dev_[name].FromNumpy(self.first_frame_[name])
            elif st.raw_:
                self.raw_data_[name].copy_(src, non_blocking=True)
            else:
                self.data_[name]._t[:src.numel()].copy_(src, non_blocking=True)
                st.Preprocess(self.data_[name])
        self.copy_done_[buf].record(torch.cuda.current_stream())
        self.last_copied_ = buf
        if len(self.raw_data_) > len(self.first_frame_):
            self.col_index_[:] = np.arange(self.chunk_size_, dtype=np.float32)
            self.col_index_dev_.FromNumpy(self.col_index_)
        if self.pipeline_loads_:
            self.StartPreload()

    def StartPreload(self):
        import threading
        if self.preload_thread_ is not None:
            raise SystemExit("Trying to create new thread when previous one is still running.")
        buf = (self.last_copied_ + 1) % 2        # the buffer no copy is reading — once its own last copy is over
        if self.allocated_:
            self.copy_done_[buf].synchronize()
        self.pending_ = buf
        if self.disk_.host_ is None:
            self.AllocateHostMemory(pinned=False)
        self.preload_thread_ = threading.Thread(target=self.disk_.Preload, args=(buf,), name="DataHandler preload", daemon=True)
        self.preload_thread_.start()

    def WaitForPreload(self):
        if self.preload_thread_ is not None:
            self.preload_thread_.join()
            self.preload_thread_ = None
            err, self.disk_.error_ = self.disk_.error_, None
            if err is not None:
                raise err

    # ---- DataHandler::DiskAccess (:239-276): the host side, on this thread ----
    def DiskAccess(self, buf=0):
        if self.disk_.host_ is None:
            self.AllocateHostMemory(pinned=False)
        return self.disk_.DiskAccess(buf)

    @property
    def host_(self):
        return self.disk_.host_
