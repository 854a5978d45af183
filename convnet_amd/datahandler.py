"""Data handlers.  The contract is the reference's (src/datahandler.cc:145-198): ``GetBatch(data_layers)``
leaves a batch in every input layer's ``state_`` (N, X*Y*C CHWN) and every output layer's ``data_``.
``DataHandler`` (below) is the reference's own, for HDF5 streams and lists of image files: built from a DatasetConfig, it reads
chunks from disk and stages batches on the GPU — rows of a dataset, clips of consecutive frames of one (``is_sequence``), or crops of
image files resized — and with ``jitter_raw_image`` randomly cropped, zoomed and rotated — on the way (``data_type: IMAGE_RAW``,
image_iterators.py); video / text / sliding-window streams are refused.
``ChunkDataHandler`` stages from numpy arrays the caller holds; ``SyntheticDataHandler`` makes noise: inputs are N(0,1) (the real pipeline feeds mean/std-normalised
pixels, :496-507), labels uniform ints stored as float (N,1); ``num_batches`` distinct batches are
pre-generated on the device and cycled, so no host work sits inside a timed step."""
import numpy as np
import torch

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


class _Jitter:
    """The crop / flip of one stream: its geometry and the per-case offsets and flip bits on the device — DataIterator::SampleNoise
    (src/datahandler.cc:534-570) and what every staging call takes of it."""

    def __init__(self, image_size_y, image_size_x, gpu_image_size_y, gpu_image_size_x, translate, flip):
        self.image_size_y_, self.image_size_x_ = image_size_y, image_size_x
        self.gpu_image_size_y_, self.gpu_image_size_x_ = gpu_image_size_y, gpu_image_size_x
        self.translate_, self.flip_ = translate, flip
        self.width_offset_, self.height_offset_, self.flip_bit_ = Matrix(), Matrix(), Matrix()

    def Jitters(self):
        return self.image_size_y_ != self.gpu_image_size_y_ or self.image_size_x_ != self.gpu_image_size_x_ or self.flip_

    def Sample(self, batch_size, multiplicity_id):
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
            self.height_offset_.Mult(max_offset_y + 1)         # rounded down by the kernel's int()
            self.width_offset_.Mult(max_offset_x + 1)
        else:                                                  # centre / corner patches by multiplicity id
            w, h = [(max_offset_x // 2, max_offset_y // 2), (0, 0), (max_offset_x, 0), (max_offset_x, max_offset_y),
                    (0, max_offset_y)][multiplicity_id % 5]
            self.height_offset_.Set(h)
            self.width_offset_.Set(w)
        if self.flip_:
            self.flip_bit_.FillWithRand()                      # flip if > 0.5
        else:
            self.flip_bit_.Set(multiplicity_id // 5)

    def StagingArgs(self, dims):
        """The (offsets, flip bits, geometry) arguments of ExtractPatches / StagePatchesU8 / StageClipsU8 for rows (frames) of ``dims``
        values.  No jitter: a transpose of whole rows, whatever image_size says (the reference's CopyTranspose)."""
        if self.Jitters():
            return (self.width_offset_, self.height_offset_, self.flip_bit_, self.image_size_y_, self.image_size_x_, self.gpu_image_size_y_,
                    self.gpu_image_size_x_)
        return (None, None, None, 1, dims, 1, dims)

    def StageColumns(self, chunk, slice_, start, end, output):
        """DataIterator::AddNoise (:520-531) from a float chunk: columns ``start:end`` of ``chunk``, through the view ``slice_``."""
        chunk.GetSlice(slice_, start, end)
        if self.Jitters():
            Matrix.ExtractPatches(slice_, output, *self.StagingArgs(chunk.GetRows()))
        else:
            slice_.CopyTranspose(output)


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
        self.jitter_ = _Jitter(image_size, image_size, crop_size or image_size, crop_size or image_size, translate, flip)
        self.colors_, self.randomize_ = colors, randomize
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
        self.width_offset_, self.height_offset_, self.flip_bit_ = self.jitter_.width_offset_, self.jitter_.height_offset_, self.jitter_.flip_bit_
        for m in (self.width_offset_, self.height_offset_, self.flip_bit_):     # (here, jitter or not)
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

    def ShuffleIndices(self):
        # DataHandler::ShuffleIndices (:139-144): random_shuffle of the SAME index array every time, then to the device
        self.rng_.shuffle(self.perm_host_)
        self.perm_.FromNumpy(self.perm_host_)

    def GetBatch(self, data_layers):
        end = self.start_ + self.batch_size_
        if end > self.chunk_size_ and self.randomize_:     # DataHandler::GetBatch :147-166: drop the tail, reshuffle, restart
            self.ShuffleIndices()
            self.data_.ShuffleColumns(self.perm_)
            self.labels_.ShuffleColumns(self.perm_)
            self.start_, end = 0, self.batch_size_
        self.jitter_.Sample(self.batch_size_, self.multiplicity_counter_)
        for l in data_layers:
            if l.IsInput():
                self.jitter_.StageColumns(self.data_, self.slice_, self.start_, end, l.GetState())
            else:
                self.labels_.GetSlice(self.label_slice_, self.start_, end)
                self.label_slice_.CopyTranspose(l.GetData())
        self.start_ = end % self.chunk_size_ if not self.randomize_ else end


_REFUSED_TYPES = {
    "DUMMY": "random numbers in place of data",
    "SLIDING_WINDOW": "sliding windows over raw images", "TXT": "text files of numbers", "BOUNDING_BOX": "bounding-box files",
    "CROPS": "crops of raw images", "VIDEO_RAW": "video files decoded on the host"}


def size_yx(dsc, field, default=None):
    """(y, x) of a stream's ``field`` (image_size; raw_image_size, the size every image of an IMAGE_RAW stream is resized to cover,
    src/datahandler.cc:725-726; gpu_image_size): ``field_y`` / ``field_x`` where the config sets them, else ``field`` for both — or
    ``default`` = (y, x), for the size that has no field of its own (gpu_image_size: the image size)."""
    y, x = default if default is not None else (getattr(dsc, field),) * 2
    return (getattr(dsc, field + "_y") if getattr(dsc, f"has_{field}_y")() else y,
            getattr(dsc, field + "_x") if getattr(dsc, f"has_{field}_x")() else x)


def _check_image_stream(dsc):
    """What an IMAGE_RAW stream cannot be here, each with a message of its own naming the layer and the field."""
    head = f"Data stream for layer {dsc.layer_name}: "
    raw_y, raw_x = size_yx(dsc, "raw_image_size")
    if raw_y <= 0 or raw_x <= 0:
        raise SystemExit(head + "data_type IMAGE_RAW without a raw_image_size (the size every image is resized to cover) is not supported; "
                         "set raw_image_size, or raw_image_size_y and raw_image_size_x.")
    if dsc.is_sequence:
        raise SystemExit(head + "is_sequence is not supported on an IMAGE_RAW stream: clips are read from HDF5 frame datasets.")
    # jitter_raw_image (image_iterators.Transform): refused where the reference would silently do nothing, or could not run
    if not dsc.jitter_raw_image and dsc.random_rotate_max_angle != 0:
        raise SystemExit(head + f"random_rotate_max_angle {dsc.random_rotate_max_angle:g} without jitter_raw_image is not supported: the "
                         "reference ignores the angle there; set jitter_raw_image: true (and min_scale: 1 or more).")
    if not dsc.jitter_raw_image and dsc.min_scale != 0:
        raise SystemExit(head + f"min_scale {dsc.min_scale:g} without jitter_raw_image is not supported: the reference ignores the scale "
                         "there; set jitter_raw_image: true.")
    if dsc.jitter_raw_image and dsc.min_scale < 1:
        raise SystemExit(head + f"jitter_raw_image with min_scale {dsc.min_scale:g} (the default is 0) is not supported: every drawn scale "
                         "would be ignored, because the reference zooms only by scales above 1; min_scale: 1 gives translation and rotation "
                         "alone, a larger one zooms in by up to that factor.")
    if dsc.jitter_raw_image and abs(int(dsc.random_rotate_max_angle)) > 90:
        raise SystemExit(head + f"jitter_raw_image with random_rotate_max_angle {dsc.random_rotate_max_angle:g} is not supported: beyond 90 "
                         "degrees the rotated image is smaller than raw_image_size and the reference cannot crop it.")
    if dsc.bbox_file:
        raise SystemExit(head + f"bbox_file ({dsc.bbox_file}) is not supported: crops around bounding boxes are not built.")
    if dsc.num_colors != 3:
        raise SystemExit(head + f"num_colors {dsc.num_colors} is not supported on an IMAGE_RAW stream: a decoded image has 3 colour planes "
                         "(the reference writes three into a buffer of num_colors).")
    size_y, size_x = size_yx(dsc, "image_size")
    if size_y <= 0 or size_x <= 0:
        raise SystemExit(head + "an IMAGE_RAW stream needs an image_size (the crop taken from every resized image).")
    if size_y > raw_y or size_x > raw_x:
        raise SystemExit(head + f"image_size {size_y} x {size_x} exceeds raw_image_size {raw_y} x {raw_x}: the crop must fit the resized image.")
    if dsc.avg10_full_image and dsc.parallel_disk_access:
        raise SystemExit(head + "avg10_full_image together with parallel_disk_access is not supported: the reference indexes its file list "
                         "with a row of the ten times larger dataset there.")


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
        self.is_images_ = dsc.data_type == "IMAGE_RAW"
        if self.is_images_:
            _check_image_stream(dsc)
        if dsc.is_sequence and dsc.seq_length < 1:
            raise SystemExit(f"Data stream for layer {name}: is_sequence needs a seq_length of at least 1, not {dsc.seq_length}.")
        if dsc.is_sequence and dsc.pca_noise_stddev > 0:
            raise SystemExit(f"Data stream for layer {name}: pca_noise_stddev is not supported on a sequence stream: the colour noise "
                             "has 3 columns, a clip 3 x seq_length planes.")
        if not self.is_images_ and dsc.data_type != "HDF5":
            what = _REFUSED_TYPES.get(dsc.data_type)
            if what is None:
                raise SystemExit(f"Data stream for layer {name}: Unknown data type {dsc.data_type}")
            raise SystemExit(f"Data stream for layer {name}: data_type {dsc.data_type} ({what}) is not supported; only HDF5 and IMAGE_RAW streams are.")
        if dsc.noise_layer_name:
            raise SystemExit(f"Data stream for layer {name}: noise_layer_name ({dsc.noise_layer_name}) is not supported: "
                             "no stream takes its jitter from another.")
        if dsc.gpu_id != 0:
            raise SystemExit(f"Data stream for layer {name}: gpu_id {dsc.gpu_id} is not supported: one process drives one GPU, gpu_id 0.")
        self.config_, self.layer_name_ = dsc, name
        size_y, size_x = size_yx(dsc, "image_size")
        if self.is_images_:          # ImageDataIterator (:723-754): a list of image files, resized to cover the raw size and cropped
            from . import image_iterators
            self.file_ = None
            self.raw_size_y_, self.raw_size_x_ = size_yx(dsc, "raw_image_size")
            self.reader_ = image_iterators.ImageReader(image_iterators.ReadFileList(dsc.file_pattern), size_y, size_x, self.raw_size_y_,
                                                       self.raw_size_x_, dsc.avg10_full_image, dsc.parallel_disk_access, name,
                                                       dsc.jitter_raw_image, dsc.random_rotate_max_angle, dsc.min_scale)
        else:
            self.file_ = hdf5io.File(dsc.file_pattern)
            self.reader_ = self.file_.RowReader(dsc.dataset_name)
        self.frame_size_, self.frames_ = self.reader_.GetDims(), 1      # a row is frames_ frames of frame_size_ values
        self.is_sequence_ = dsc.is_sequence
        self.form_ = None            # how the chunk is kept: DataHandler.SetInputLayers decides
        if dsc.is_sequence:
            try:
                self.reader_ = _SequenceReader(self.reader_, dsc.seq_length, dsc.boundary_file, dsc.pick_first, name)
            except BaseException:
                self.close()
                raise
            self.frames_ = 1 if dsc.pick_first else dsc.seq_length
        self.jitter_ = j = _Jitter(size_y, size_x, *size_yx(dsc, "gpu_image_size", (size_y, size_x)), dsc.can_translate, dsc.can_flip)
        self.width_offset_, self.height_offset_, self.flip_bit_ = j.width_offset_, j.height_offset_, j.flip_bit_
        self.num_colors_ = dsc.num_colors
        self.normalize_ = dsc.normalize or dsc.pixelwise_normalize
        self.pixelwise_normalize_, self.normalize_local_ = dsc.pixelwise_normalize, dsc.normalize_local
        self.pca_noise_stddev_ = dsc.pca_noise_stddev
        self.add_pca_noise_ = dsc.pca_noise_stddev > 0
        self.mean_ = self.std_ = None
        self.pca_noise1_, self.pca_noise2_ = Matrix(), Matrix()

    raw_ = property(lambda self: self.form_ is not None and self.form_.raw_)
    frames_once_ = property(lambda self: self.form_ is not None and self.form_.frames_once_)

    def GetDims(self):
        return self.reader_.GetDims()

    def StagedDims(self):
        """The width of the batch this stream leaves in its layer."""
        j = self.jitter_
        return self.frames_ * self.num_colors_ * j.gpu_image_size_y_ * j.gpu_image_size_x_ if j.Jitters() else self.GetDims()

    def CheckGeometry(self):
        j = self.jitter_
        if j.Jitters() and self.frame_size_ != self.num_colors_ * j.image_size_y_ * j.image_size_x_:
            what = "frames" if self.is_sequence_ else "rows"
            raise SystemExit(f"Data stream for layer {self.layer_name_}: {what} of {self.frame_size_} values are not {self.num_colors_} colours of "
                             f"{j.image_size_y_} x {j.image_size_x_} pixels.")
        if j.gpu_image_size_y_ > j.image_size_y_ or j.gpu_image_size_x_ > j.image_size_x_:
            raise SystemExit(f"Data stream for layer {self.layer_name_}: gpu_image_size exceeds image_size.")

    def Normalizers(self):
        """(mean, std) for a staging call that normalises on the way, or no pair."""
        return (self.mean_, self.std_) if self.normalize_ else (None, None)

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

    # ---- DataIterator::AddPCANoise (:509-518) ----
    def AddPCANoise(self, m):
        if self.pca_noise1_.GetRows() != m.GetRows():
            self.pca_noise1_.AllocateGPUMemory(m.GetRows(), self.eig_vectors_.GetRows())
            self.pca_noise2_.AllocateGPUMemory(m.GetRows(), self.eig_vectors_.GetCols())
        self.pca_noise1_.FillWithRandn()
        self.pca_noise1_.MultByRowVec(self.eig_values_)
        Matrix.Dot(self.pca_noise1_, self.eig_vectors_, self.pca_noise2_, 0, 1)
        m.AddToEachPixel(self.pca_noise2_, self.pca_noise_stddev_)

    # ---- DataIterator::AddNoise (:520-532) ----
    def AddNoise(self, start, end, output):
        self.form_.Stage(self, start, end, output)
        if self.add_pca_noise_:
            self.AddPCANoise(output)

    def close(self):
        self.reader_.close()
        if self.file_ is not None:
            self.file_.close()


# ---- the chunk forms ----------------------------------------------------------------------------------------------------------------------
# A form has two halves.  The DISK half (_RowsDisk / _FramesDisk / _ImagesDisk) is all the preload thread sees of it: the row reader, the
# shape of a host buffer and how a run of rows gets into one — libhdf5, the image decoders and numpy only.  The DEVICE half (_FloatForm /
# _BytesForm / _FramesOnceForm / _ImagesOnceForm, which
# holds its disk half as ``disk_``) owns the chunk on the GPU: storage, upload, what randomize_gpu does to it, staging a batch.

class _RowsDisk:
    """Rows as they are in the dataset, one per buffer row: cast to float by the reader (float form) or kept as bytes (bytes form)."""

    def __init__(self, reader, chunk_size, dataset_size, dtype):
        self.reader_, self.chunk_size_, self.dataset_size_, self.dtype_ = reader, chunk_size, dataset_size, dtype

    def HostBuffers(self, count):
        """(shape, dtype) of a host buffer of this stream; ``count`` of them are about to be made."""
        return (self.chunk_size_, self.reader_.GetDims()), self.dtype_

    def Prep(self):
        """DataIterator::Prep: once per DiskAccess, before any run is loaded — not once per LoadRun piece."""
        prep = getattr(self.reader_, "Prep", None)
        if prep is not None:
            prep(self.chunk_size_)

    def LoadRun(self, out, buf, at, row, count, seek=False):
        """``count`` consecutive rows from ``row`` into host buffer ``out`` (number ``buf``) from chunk position ``at`` on, wrapping at the
        end of the dataset (GetNext's wrap, :717-721; LoadChunk's, :305-311)."""
        size = self.dataset_size_
        while count > 0:
            n = min(count, size - row)
            self.LoadPiece(out, buf, at, row, n)
            at, count, row = at + n, count - n, (row + n) % size
        if seek:
            self.reader_.Seek(row)

    def LoadPiece(self, out, buf, at, row, n):
        self.reader_.Get(out[at:at + n], row, row + n)


class _FramesDisk(_RowsDisk):
    """Clip rows of a sequence stream with every frame held once: a buffer is (frames, frame_size); beside each there is the table of the
    buffer row of every clip's first frame (float32, as it goes to the device) and the number of buffer rows the chunk filled."""

    def __init__(self, reader, chunk_size, dataset_size, buffer_frames):
        super().__init__(reader, chunk_size, dataset_size, np.uint8)
        self.buffer_frames_ = buffer_frames  # DataHandler.FrameBufferSize: the worst case, sized once
        self.first_frame_ = self.frames_used_ = None         # [buffer]

    def HostBuffers(self, count):
        self.first_frame_ = [np.zeros(self.chunk_size_, np.float32) for _ in range(count)]
        self.frames_used_ = [0] * count
        return (self.buffer_frames_, self.reader_.frame_size_), self.dtype_

    def LoadPiece(self, frames, buf, at, row, n):
        """The union of the clips' frame ranges goes behind what the buffer holds (a run at chunk position 0 begins it), in dataset order
        and every frame once; clips ``at`` ... of the table get the buffer row of their first frame.  One hyperslab read ends where the
        next clip does not start one frame on: at a sequence boundary, at a skipped sequence, at the wrap to row 0."""
        table, filled = self.first_frame_[buf], self.frames_used_[buf] if at else 0
        m, T = self.reader_.row_mapping_[row:row + n], self.reader_.seq_length_
        cuts = np.flatnonzero(np.diff(m) != 1) + 1
        for a, b in zip([0, *cuts.tolist()], [*cuts.tolist(), n]):
            lo, hi = int(m[a]), int(m[b - 1]) + T
            self.reader_.base_.Get(frames[filled:filled + hi - lo], lo, hi)
            table[at + a:at + b] = filled + (m[a:b] - lo)
            filled += hi - lo
        self.frames_used_[buf] = filled


class _ImagesDisk(_RowsDisk):
    """Rows of an IMAGE_RAW stream with every file of the chunk decoded ONCE: a buffer is plain bytes — the images at their original
    sizes as interleaved R, G, B rows, back to back.  Beside each buffer (numpy, [buffer]): ``image_table_`` {byte offset, w, h, new_w,
    new_h, first tap} per image, ``taps_`` {source index, coefficient 0, coefficient 1} per column and row of every resized image, built
    here in the preload thread, ``case_table_`` {image, left, top, mirrored} per case, and how much of each the chunk filled.  The ten
    positions of a file share its pixels and its taps.  A ``jitter_raw_image`` stream has the 11-column image table and the rotation rows
    of ``stage_images_jitter_u8`` instead (``_jittered``), drawn anew for every chunk by the reader's ``Prep``.  Buffers start at chunk_size * raw_y * raw_x * 3 * 2 bytes (twice a chunk of images
    that are exactly the raw size); a chunk that needs more gets new ones of twice its need, through ``grow_`` (the handler's, which
    knows whether host buffers are pinned)."""

    def __init__(self, reader, chunk_size, dataset_size):
        super().__init__(reader, chunk_size, dataset_size, np.uint8)
        self.start_bytes_ = chunk_size * reader.raw_y_ * reader.raw_x_ * 3 * 2
        self.image_table_ = self.taps_ = self.case_table_ = self.bytes_used_ = self.images_used_ = self.taps_used_ = None
        self.image_of_file_ = None           # [buffer]: file -> image number, of the chunk in the buffer
        self.bytes_ = None                   # [buffer]: the host array as it is now (DataHandler.AllocateHostMemory)
        self.grow_ = None                    # (buffer number, bytes) -> the new host array, in place of the old one everywhere

    def HostBuffers(self, count):
        r = self.reader_
        self.image_table_ = [np.zeros((self.chunk_size_, 11 if r.jitter_ else 6), np.int64) for _ in range(count)]
        self.taps_ = [np.zeros((self.chunk_size_ * (r.raw_y_ + r.raw_x_) * 2, 3), np.int32) for _ in range(count)]
        self.case_table_ = [np.zeros((self.chunk_size_, 4), np.int32) for _ in range(count)]
        self.bytes_used_, self.images_used_, self.taps_used_ = [0] * count, [0] * count, [0] * count
        self.image_of_file_ = [{} for _ in range(count)]
        return (self.start_bytes_,), self.dtype_

    def Used(self, buf):
        """What the chunk in host buffer ``buf`` filled: the bytes, the image table, the taps and the case table (views)."""
        return (self.bytes_[buf][:self.bytes_used_[buf]], self.image_table_[buf][:self.images_used_[buf]],
                self.taps_[buf][:self.taps_used_[buf]], self.case_table_[buf])

    def LoadPiece(self, out, buf, at, row, n):
        """The files of rows ``row:row + n`` that the buffer does not hold yet go behind what it holds (a run at chunk position 0 begins
        it); cases ``at`` ... of the case table get their image and the crop of their position in the RESIZED image."""
        from . import image_iterators as ii
        r = self.reader_
        if at == 0:
            self.bytes_used_[buf] = self.images_used_[buf] = self.taps_used_[buf] = 0
            self.image_of_file_[buf] = {}
        known = self.image_of_file_[buf]
        files = [f for f in r.FilesOf(row, row + n) if f not in known]
        images = r.Decode(files)
        if r.jitter_:                        # (left, top, crop w, crop h, angle, new_w, new_h) per file, and the tap rows it takes
            sizes = [r.JitterGeometry(f, im.shape[1], im.shape[0]) for f, im in zip(files, images)]
            tap_rows = [new_w + new_h + ((r.raw_x_ + r.raw_y_) if angle != 0 else 0) for *_, angle, new_w, new_h in sizes]
        else:
            sizes = [(im.shape[1], im.shape[0], *ii.ResizedSize(im.shape[1], im.shape[0], r.raw_y_, r.raw_x_)) for im in images]
            tap_rows = [new_w + new_h for _, _, new_w, new_h in sizes]
        used, taps_used = self.bytes_used_[buf], self.taps_used_[buf]
        need = used + sum(im.size for im in images)
        out = self.bytes_[buf]               # (not the caller's: an earlier piece of this chunk may have replaced it)
        if need > out.size:
            grown = self.grow_(buf, 2 * need)
            grown[:used] = out[:used]
            out = grown
        taps_need = taps_used + sum(tap_rows)
        if taps_need > len(self.taps_[buf]):
            grown = np.zeros((2 * taps_need, 3), np.int32)
            grown[:taps_used] = self.taps_[buf][:taps_used]
            self.taps_[buf] = grown
        for f, im, size, count in zip(files, images, sizes, tap_rows):
            k = known[f] = self.images_used_[buf]
            out[used:used + im.size] = im.reshape(-1)
            t = self.taps_[buf][taps_used:taps_used + count]
            if r.jitter_:
                self.image_table_[buf][k] = self._jittered(t, im.shape[1], used, taps_used, *size)
            else:
                w, h, new_w, new_h = size
                t[:new_w], t[new_w:] = ii.ImageTaps(w, h, new_w, new_h)
                self.image_table_[buf][k] = (used, w, h, new_w, new_h, taps_used)
            used, taps_used, self.images_used_[buf] = used + im.size, taps_used + count, k + 1
        self.bytes_used_[buf], self.taps_used_[buf] = used, taps_used
        for i in range(n):
            f, position = r.FileAndPosition(row + i)
            new_w, new_h = (r.raw_x_, r.raw_y_) if r.jitter_ else self.image_table_[buf][known[f]][3:5]
            left, top, mirrored = ii.Coordinates(int(new_w), int(new_h), position, r.size_y_, r.size_x_)
            self.case_table_[buf][at + i] = (known[f], left, top, mirrored)

    def _jittered(self, t, width, at, first_tap, left, top, sx, sy, angle, new_w, new_h):
        """The image-table row of a jittered file (include/convnet_hip.h: stage_images_jitter_u8) whose pixels start at byte ``at``, and
        its tap rows into ``t``: the view of the crop inside the file, the taps crop -> new_w x new_h, and behind them, when the crop is
        rotated, the rotation rows of the columns and of the rows that the raw-size window covers."""
        from . import image_iterators as ii
        raw_x, raw_y = self.reader_.raw_x_, self.reader_.raw_y_
        t[:new_w], t[new_w:new_w + new_h] = ii.ImageTaps(sx, sy, new_w, new_h)
        if angle != 0:
            adelta, bdelta, X0, Y0 = ii.RotationTables(new_w, new_h, angle)
            ox, oy = new_w // 2 - raw_x // 2, new_h // 2 - raw_y // 2
            rot = t[new_w + new_h:]
            rot[:raw_x, 0], rot[:raw_x, 1] = adelta[ox:ox + raw_x], bdelta[ox:ox + raw_x]
            rot[raw_x:, 0], rot[raw_x:, 1] = X0[oy:oy + raw_y], Y0[oy:oy + raw_y]
            rot[:, 2] = 0
        return (at + (top * width + left) * 3, sx, sy, new_w, new_h, first_tap, width * 3, int(angle != 0), first_tap + new_w + new_h,
                raw_x, raw_y)


class _Index:
    """``chunk_size`` column numbers beside a byte chunk, as floats, on the host and on the device: a batch gathers the columns that
    entries ``start:end`` name.  The chunk stays where the copy left it; randomize_gpu swaps entries here."""

    def __init__(self, chunk_size):
        self.host_ = np.arange(chunk_size, dtype=np.float32)
        self.dev_ = Matrix()

    def Allocate(self):
        self.dev_.AllocateGPUMemory(1, len(self.host_))

    def Set(self, values):
        self.host_[:] = values
        self.dev_.FromNumpy(self.host_)

    def Reset(self):
        self.Set(np.arange(len(self.host_), dtype=np.float32))

    def Swap(self, a, b):
        self.host_[a], self.host_[b] = self.host_[b].copy(), self.host_[a].copy()
        self.dev_.FromNumpy(self.host_)


class _Form:
    """What randomize_gpu does to a chunk, given the shuffled permutation: shuffleColumns swaps columns idx[2j] and idx[2j + 1] for every
    pair (``a[j]``, ``b[j]`` on the host; a permutation's pairs are disjoint).  A float chunk has its columns swapped on the device; a
    byte chunk stays where it is, and the same swaps go to the index of where each column sits."""

    def ShuffleColumns(self, rand_perm_indices):
        pass

    def SwapEntries(self, a, b):
        pass


class _FloatForm(_Form):
    """The reference's form: rows are cast to float on the host, the chunk is a (dims, cases) ``Matrix``, ``Preprocess`` normalises all of
    it at load, randomize_gpu swaps its columns, and a batch is ``ExtractPatches`` / ``CopyTranspose`` of a slice."""
    raw_ = frames_once_ = False

    def __init__(self, st, chunk_size, dataset_size):
        self.chunk_size_ = chunk_size
        self.disk_ = _RowsDisk(st.reader_, chunk_size, dataset_size, np.float32)
        self.data_, self.slice_ = Matrix(), Matrix()

    def AllocateMemory(self, st):
        self.data_.AllocateGPUMemory(st.GetDims(), self.chunk_size_, "databuffer")

    def Upload(self, st, src, buf):
        self.data_._t[:src.numel()].copy_(src, non_blocking=True)
        st.Preprocess(self.data_)

    def ShuffleColumns(self, rand_perm_indices):
        self.data_.ShuffleColumns(rand_perm_indices)

    def Stage(self, st, start, end, output):
        st.jitter_.StageColumns(self.data_, self.slice_, start, end, output)


class _BytesForm(_Form):
    """The chunk stays on the GPU exactly as read — a ``torch.uint8`` tensor, a quarter of the transfer and of the memory — and nothing
    touches it after the copy.  Which column a case sits in is the handler's one column index, shared by all its streams of this form (the
    handler resets and swaps it); a batch is ONE ``StagePatchesU8``: cast, mean / std, crop, flip and transpose together."""
    raw_, frames_once_ = True, False

    def __init__(self, st, chunk_size, dataset_size, col_index):
        self.chunk_size_, self.col_index_ = chunk_size, col_index
        self.disk_ = _RowsDisk(st.reader_, chunk_size, dataset_size, np.uint8)
        self.data_, self.index_slice_ = None, Matrix()

    def AllocateMemory(self, st):
        self.data_ = torch.empty(self.chunk_size_ * st.GetDims(), dtype=torch.uint8, device=Matrix()._dev())

    def Upload(self, st, src, buf):
        self.data_.copy_(src, non_blocking=True)

    def Stage(self, st, start, end, output):
        self.col_index_.dev_.GetSlice(self.index_slice_, start, end)
        dims = st.GetDims()
        Matrix.StagePatchesU8(self.data_, dims, self.chunk_size_, self.index_slice_, *st.Normalizers(), output, *st.jitter_.StagingArgs(dims))


class _FramesOnceForm(_Form):
    """A sequence stream's byte form: every frame of a run of consecutive clip rows is held ONCE — the union of the clips' frame ranges, in
    dataset order — beside this stream's own table of the buffer column of every clip's first frame.  Only the used prefix of a host buffer
    is uploaded; randomize_gpu swaps entries of the table; a batch is ONE ``StageClipsU8`` that gathers each clip's consecutive columns."""
    raw_ = frames_once_ = True

    def __init__(self, st, chunk_size, dataset_size, buffer_frames):
        self.disk_ = _FramesDisk(st.reader_, chunk_size, dataset_size, buffer_frames)
        self.data_, self.frames_used_ = None, 0
        self.first_frame_, self.index_slice_ = _Index(chunk_size), Matrix()

    def AllocateMemory(self, st):            # (the host buffer's size: the worst case, allocated once)
        self.data_ = torch.empty(self.disk_.buffer_frames_ * st.frame_size_, dtype=torch.uint8, device=Matrix()._dev())
        self.first_frame_.Allocate()

    def Upload(self, st, src, buf):          # the used prefix alone, and the table that goes with it
        used = self.frames_used_ = self.disk_.frames_used_[buf]
        self.data_[:used * st.frame_size_].copy_(src[:used * st.frame_size_], non_blocking=True)
        self.first_frame_.Set(self.disk_.first_frame_[buf])

    def SwapEntries(self, a, b):
        self.first_frame_.Swap(a, b)

    def Stage(self, st, start, end, output):
        self.first_frame_.dev_.GetSlice(self.index_slice_, start, end)
        fs, used = st.frame_size_, self.frames_used_
        Matrix.StageClipsU8(self.data_[:used * fs], fs, used, self.index_slice_, st.frames_, *st.Normalizers(), output,
                            *st.jitter_.StagingArgs(fs))


class _ImagesOnceForm(_Form):
    """An IMAGE_RAW stream's byte form: the decoded files of a chunk at their original sizes, each once, and the three tables of
    ``_ImagesDisk`` beside them on the device.  Only the used prefixes are uploaded; the device buffer starts at the host buffer's size and
    is reallocated at twice the need when a chunk needs more; randomize_gpu swaps rows of the case table; a batch is ONE ``StageImagesU8``
    that resamples, crops, mirrors, normalises and transposes the pixels of the patch — the resized image is never made.  A
    ``jitter_raw_image`` stream takes ``StageImagesJitterU8``, which also crops, zooms and rotates on the way."""
    raw_, frames_once_ = True, False

    def __init__(self, st, chunk_size, dataset_size):
        self.disk_ = _ImagesDisk(st.reader_, chunk_size, dataset_size)
        self.data_ = self.image_table_ = self.taps_ = self.case_table_ = self.case_host_ = None
        self.bytes_used_, self.rotated_ = 0, False

    def AllocateMemory(self, st):
        self.data_ = torch.empty(self.disk_.start_bytes_, dtype=torch.uint8, device=Matrix()._dev())

    def Upload(self, st, src, buf):
        d, dev = self.disk_, self.data_.device
        used = self.bytes_used_ = d.bytes_used_[buf]
        if used > self.data_.numel():
            self.data_ = torch.empty(2 * used, dtype=torch.uint8, device=dev)
        self.data_[:used].copy_(src[:used], non_blocking=True)
        _, image_table, taps, case_table = d.Used(buf)
        self.image_table_, self.taps_ = torch.from_numpy(image_table).to(dev), torch.from_numpy(taps).to(dev)
        self.rotated_ = bool(image_table.shape[1] > 7 and image_table[:, 7].any())      # no rotated image: the arm without the blend
        self.case_host_ = case_table.copy()
        self.case_table_ = torch.from_numpy(self.case_host_).to(dev)

    def SwapEntries(self, a, b):
        self.case_host_[a], self.case_host_[b] = self.case_host_[b].copy(), self.case_host_[a].copy()
        self.case_table_ = torch.from_numpy(self.case_host_).to(self.data_.device)

    def Cases(self, start, end):
        """The chunk on the device as the image entries take it: the bytes, the image table, the taps and cases ``start:end``."""
        return self.data_[:self.bytes_used_], self.image_table_, self.taps_, self.case_table_[start:end]

    def Stage(self, st, start, end, output):
        j = st.jitter_
        offsets = (j.width_offset_, j.height_offset_, j.flip_bit_) if j.Jitters() else (None, None, None)
        sizes = (j.image_size_y_, j.image_size_x_, j.gpu_image_size_y_, j.gpu_image_size_x_)
        if st.reader_.jitter_:               # jitter_raw_image: the crop view, the zoom and the rotation live in the image table
            Matrix.StageImagesJitterU8(*self.Cases(start, end), self.rotated_, *st.Normalizers(), output, *offsets, *sizes)
        else:
            Matrix.StageImagesU8(*self.Cases(start, end), *st.Normalizers(), output, *offsets, *sizes)


class _DiskSide:
    """DataHandler::DiskAccess / LoadChunk (src/datahandler.cc:239-314): everything the preload thread touches — the disk halves of the
    streams' forms (their row readers), the host buffers and the random-row list.  libhdf5 and numpy only: no GPU call, no ``Matrix``, and
    no way back to the handler, so a handler that is dropped while a preload runs is collected (and joins the thread) at once."""

    def __init__(self, chunk_size, dataset_size, randomize_cpu, random_access_chunk_size, rng):
        self.halves_ = None                  # layer name -> disk half of the stream's form, in data_config order (SetInputLayers)
        self.chunk_size_, self.dataset_size_ = chunk_size, dataset_size
        self.randomize_cpu_, self.random_access_chunk_size_ = randomize_cpu, random_access_chunk_size
        self.rng_ = rng
        self.random_indices_ind_ = 0
        if randomize_cpu:
            self.random_indices_ = rng.permutation(dataset_size)
        self.host_ = None                    # [buffer][layer name] -> array, shaped as the disk half says
        self.error_ = None

    def _beside(self, what):
        return [{name: getattr(half, what)[buf] for name, half in self.halves_.items() if getattr(half, what, None) is not None}
                for buf in range(len(self.host_ or ()))]

    # [buffer][layer name] -> what a disk half keeps beside that host buffer (read-only views, as ``DataHandler.host_`` is)
    first_frame_ = property(lambda self: self._beside("first_frame_"))
    frames_used_ = property(lambda self: self._beside("frames_used_"))

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
        for half in self.halves_.values():       # every stream first (:253-257): an image stream draws its jitter_raw_image entries anew
            half.Prep()
        for name, half in self.halves_.items():
            out = self.host_[buf][name]
            if random_rows is None:
                half.LoadRun(out, buf, 0, half.reader_.Tell(), self.chunk_size_, seek=True)
            else:
                for i, row in enumerate(random_rows):
                    at = i * self.random_access_chunk_size_
                    # (the last run stops at the end of the chunk: the reference reads a whole run there, past its buffer)
                    half.LoadRun(out, buf, at, row, min(self.random_access_chunk_size_, self.chunk_size_ - at))
        return self.host_[buf]


def _grower(host, tensors, half, name, pinned):
    """What replaces a host buffer of an images-once stream by a larger one (``_ImagesDisk.grow_``): in the handler's lists and in the
    disk half's.  It holds no handler.  With pinned buffers this is the one GPU runtime call the preload thread can make."""
    def grow(buf, size):
        if pinned:
            tensors[buf][name] = torch.empty((size,), dtype=torch.uint8, pin_memory=True)
            host[buf][name] = tensors[buf][name].numpy()
        else:
            host[buf][name] = np.zeros((size,), np.uint8)
        half.bytes_[buf] = host[buf][name]
        return host[buf][name]
    return grow


class DataHandler:
    """DataHandler for HDF5 streams, built from a ``pbtxt.DatasetConfig`` (src/datahandler.cc:8-336): chunks of the dataset are read
    from disk (sequentially, or ``randomize_cpu`` in runs of ``random_access_chunk_size`` rows), copied to the GPU, and every
    ``GetBatch`` stages one batch from the resident chunk into the data layers.

    Every stream keeps its chunk in one of three forms, a class each (above); ``SetInputLayers`` picks.  **float** (``_FloatForm``) is the
    reference's.  **bytes** (``_BytesForm``) is taken when the dataset is stored as unsigned 8-bit, its layer is an input layer and
    ``normalize_local`` is off; a batch out of it is bit for bit what the float form leaves.  **frames-once** (``_FramesOnceForm``) is the
    bytes form of a sequence stream (``is_sequence``, not ``pick_first``), whose float form is one materialised clip of ``seq_length``
    frames per column; its buffers are sized once, to the exact worst case over run starts (``FrameBufferSize``).  **images-once**
    (``_ImagesOnceForm``) is the bytes form of an IMAGE_RAW stream, whose float form is resized and cropped on the host: the decoded files
    of a chunk at their original sizes, each once, and tables; its buffers grow when a chunk needs more.  ``raw_chunks=False``
    forces the float form everywhere.

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
        self.streams_ = {}                   # layer name -> stream, in data_config order
        for dsc in config.data_config:
            st = self.streams_[dsc.layer_name] = _Stream(dsc)
            if st.is_images_ and dsc.avg10_full_image and config.randomize_cpu:
                raise SystemExit(f"Data stream for layer {dsc.layer_name}: avg10_full_image together with randomize_cpu is not supported: "
                                 "the reference indexes its file list with a row of the ten times larger dataset there.")
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
        self.disk_ = _DiskSide(self.chunk_size_, self.dataset_size_, self.randomize_cpu_, self.random_access_chunk_size_, self.row_rng_)
        self.perm_host_ = np.arange(self.chunk_size_, dtype=np.float32)     # SetupShuffler: shuffled in place, again and again
        self.col_index_ = None               # where each column of a byte chunk sits now: ONE index for all the plain byte streams
        self.input_layers_set_ = self.allocated_ = False
        self.copy_done_ = [None, None]       # per host buffer: the event behind the last copy that read it
        self.last_copied_, self.pending_ = -1, 0
        self.Seek(0)

    # ---- which form every stream keeps its chunk in: the one place that decides ----
    def SetInputLayers(self, names):
        self.col_index_ = None
        for name, st in self.streams_.items():
            raw = (self.raw_chunks_ and name in names and st.reader_.GetStoredType() == np.uint8 and not st.normalize_local_
                   and not (st.is_sequence_ and st.config_.pick_first))
            frames = self.FrameBufferSize(name) if raw and st.is_sequence_ else 0
            if frames > 1 << 24:
                raise SystemExit(f"Data stream for layer {name}: a byte chunk of more than 2^24 frames cannot be indexed; set chunk_size.")
            if raw and self.chunk_size_ > 1 << 24:
                raise SystemExit(f"Data stream for layer {name}: a byte chunk of more than 2^24 cases cannot be indexed; set chunk_size.")
            if frames:
                st.form_ = _FramesOnceForm(st, self.chunk_size_, self.dataset_size_, frames)
            elif raw and st.is_images_:
                st.form_ = _ImagesOnceForm(st, self.chunk_size_, self.dataset_size_)
            elif raw:
                self.col_index_ = self.col_index_ or _Index(self.chunk_size_)
                st.form_ = _BytesForm(st, self.chunk_size_, self.dataset_size_, self.col_index_)
            else:
                st.form_ = _FloatForm(st, self.chunk_size_, self.dataset_size_)
        self.disk_.halves_ = {name: st.form_.disk_ for name, st in self.streams_.items()}
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
        count = 2 if self.pipeline_loads_ else 1
        buffers = {name: half.HostBuffers(count) for name, half in self.disk_.halves_.items()}
        host, self.host_tensors_ = [], []
        for _ in range(count):
            arrays, tensors = {}, {}
            for name, (shape, dtype) in buffers.items():
                if pinned:
                    tensors[name] = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), pin_memory=True)
                    arrays[name] = tensors[name].numpy()
                else:
                    arrays[name] = np.zeros(shape, dtype)
            host.append(arrays)
            self.host_tensors_.append(tensors)
        self.disk_.host_ = host
        for name, half in self.disk_.halves_.items():
            if isinstance(half, _ImagesDisk):
                half.bytes_ = [arrays[name] for arrays in host]
                half.grow_ = _grower(host, self.host_tensors_, half, name, pinned)

    def AllocateMemory(self):
        self.AllocateHostMemory(pinned=True)
        for name, st in self.streams_.items():
            st.form_.AllocateMemory(st)
            if st.normalize_:
                st.LoadMeans()
            elif st.add_pca_noise_:
                raise SystemExit(f"Data stream for layer {name}: pca_noise_stddev needs pixelwise_normalize (S and U come from mean_file).")
        if self.randomize_gpu_:
            self.rand_perm_indices_ = Matrix()
            self.rand_perm_indices_.AllocateGPUMemory(1, self.chunk_size_)
        if self.col_index_ is not None:
            self.col_index_.Allocate()
            self.col_index_.Reset()
        self.copy_done_ = [torch.cuda.Event() for _ in self.host_]
        self.allocated_ = True

    # ---- the trainer's protocol ----
    def GetBatchSize(self):
        return self.batch_size_

    def GetDataSetSize(self):
        return self.dataset_size_

    def GetMultiplicity(self):
        return self.multiplicity_

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
            if l.GetName() in self.streams_:
                self.streams_[l.GetName()].form_.ShuffleColumns(self.rand_perm_indices_)
        pairs = self.perm_host_[:2 * (self.chunk_size_ // 2)].astype(np.int64)     # the pairs shuffleColumns swaps (_Form)
        a, b = pairs[0::2], pairs[1::2]
        if self.col_index_ is not None:
            self.col_index_.Swap(a, b)
        for st in self.streams_.values():
            st.form_.SwapEntries(a, b)

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
            st.jitter_.Sample(self.batch_size_, self.multiplicity_counter_)
        for l, st in streams:
            st.AddNoise(self.start_, end, l.GetState() if l.IsInput() else l.GetData())
        self.multiplicity_counter_ += 1
        if self.multiplicity_counter_ == self.multiplicity_:
            self.multiplicity_counter_ = 0
            self.start_ = end

    # ---- DataHandler::PipelinedDiskAccess / StartPreload / WaitForPreload (:202-237) ----
    def PipelinedDiskAccess(self, preload_next=True):
        """``preload_next=False``: the chunk that is uploaded now is the last one a single pass needs (ChunkPass)."""
        if self.pipeline_loads_:
            self.WaitForPreload()
            buf = self.pending_
        else:
            buf = 0
            self.copy_done_[0].synchronize()     # the last copy out of this buffer
            self.DiskAccess(0)
        for name, st in self.streams_.items():   # on the stream the step runs on
            st.form_.Upload(st, self.host_tensors_[buf][name].view(-1), buf)
        self.copy_done_[buf].record(torch.cuda.current_stream())
        self.last_copied_ = buf
        if self.col_index_ is not None:          # the byte chunks are as read again
            self.col_index_.Reset()
        if self.pipeline_loads_ and preload_next:
            self.StartPreload()

    def ChunkPass(self):
        """ONE pass over the dataset, chunk by chunk (compute_mean, image2hdf5): starts the preload; per chunk waits for it, uploads the
        chunk and preloads the next one unless this is the last, then yields the chunk's number and how many of its cases count (a last
        chunk wraps to the first rows behind its valid part).  ``pass_wait_seconds_``: the time the pass spent waiting and uploading."""
        import time
        num_chunks = -(-self.dataset_size_ // self.chunk_size_)
        self.pass_wait_seconds_ = 0.0
        self.StartPreload()
        for k in range(num_chunks):
            t0 = time.perf_counter()
            self.PipelinedDiskAccess(preload_next=k + 1 < num_chunks)
            self.pass_wait_seconds_ += time.perf_counter() - t0
            yield k, min(self.chunk_size_, self.dataset_size_ - k * self.chunk_size_)

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

    @property
    def raw_data_(self):
        """layer name -> the chunk on the device, of the streams whose chunk stays a byte tensor (a read-only view)."""
        return {name: st.form_.data_ for name, st in self.streams_.items() if isinstance(st.form_.data_, torch.Tensor)}
