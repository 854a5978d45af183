"""Image files as a data stream: ``data_type: IMAGE_RAW`` — ImageDataIterator over RawImageFileIterator<unsigned char>
(src/datahandler.cc:723-796, src/image_iterators.cc:89-334).  A text file lists the images; every image is decoded, resized so that it
covers ``raw_image_size`` (``Resize``, :173-187), and a row of the stream is the ``image_size`` crop at one of the positions of
``GetCoordinates`` (:143-171), mirrored or not, as planar R, G, B bytes (``getData``, :60-87).

The resize is the reference's ``resizeOCV``: two 8-bit bilinear resizes, first the width at the old height, then the height.  What this
module (and ``stage_images_u8``, which resamples the crop's pixels on the GPU from the same taps) computes is the DEFINITION written down
in include/convnet_hip.h — OpenCV's 8-bit INTER_LINEAR as its generic C path computes it — and the tests pin that definition, not an
OpenCV build: none was at hand to compare with (NOTES.md).

numpy only; PIL is imported when a file is neither a binary PPM nor a binary PGM.  Nothing here touches the GPU."""
import numpy as np

NUM_COLORS = 3
MAX_DECODE_THREADS = 8     # parallel_disk_access: a chunk's files on a pool of at most this many threads, whatever the machine has


def ReadFileList(path):
    """readFileList (src/util.cc:13-27): the whitespace-separated words of a text file.  (The reference drops a last word that no
    whitespace follows; here it counts — NOTES.md.)"""
    try:
        with open(path) as f:
            return f.read().split()
    except (OSError, UnicodeDecodeError):
        raise SystemExit(f"Could not open data file : {path}")


# ---- decoding -----------------------------------------------------------------------------------------------------------------------------
def _pnm_header(data):
    """(magic, width, height, maxval, offset of the raster) of a binary PPM / PGM, comments allowed; None for anything else."""
    if data[:2] not in (b"P5", b"P6"):
        return None
    pos, values = 2, []
    while len(values) < 3:
        while pos < len(data) and data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            while pos < len(data) and data[pos:pos + 1] not in (b"\n", b"\r"):
                pos += 1
            continue
        end = pos
        while end < len(data) and data[end:end + 1].isdigit():
            end += 1
        if end == pos:
            return None
        values.append(int(data[pos:end]))
        pos = end
    if not data[pos:pos + 1].isspace():
        return None
    return data[:2], values[0], values[1], values[2], pos + 1


def DecodePNM(data):
    """A binary PPM (P6) or PGM (P5) of maxval 255 as (h, w, 3) bytes, grey repeated three times; None when ``data`` is neither."""
    header = _pnm_header(data)
    if header is None:
        return None
    magic, w, h, maxval, at = header
    channels = 3 if magic == b"P6" else 1
    if maxval != 255 or w < 1 or h < 1 or len(data) - at < w * h * channels:
        return None
    pixels = np.frombuffer(data, np.uint8, w * h * channels, at).reshape(h, w, channels)
    return np.ascontiguousarray(np.broadcast_to(pixels, (h, w, 3)))


def ReadImage(path):
    """LoadImageFile (:288-294): the file as (h, w, 3) R, G, B bytes.  Grey images become three equal planes, alpha is dropped, a palette
    is resolved, no EXIF rotation is applied."""
    try:
        with open(path, "rb") as f:
            data = f.read()
        image = DecodePNM(data)
        if image is None:
            import io
            from PIL import Image
            with Image.open(io.BytesIO(data)) as im:
                image = np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))
        if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(image.shape)
        return image
    except Exception:
        raise SystemExit(f"Error reading file {path}")


def ReadImages(paths, parallel=False):
    """The decoded images of ``paths``, in order; ``parallel``: on a thread pool (the decoders release the interpreter lock)."""
    if not parallel or len(paths) < 2:
        return [ReadImage(p) for p in paths]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(MAX_DECODE_THREADS, len(paths))) as pool:
        return list(pool.map(ReadImage, paths))


# ---- the resize -----------------------------------------------------------------------------------------------------------------------------
def Taps(ssize, dsize):
    """The taps of one bilinear pass from ``ssize`` to ``dsize`` samples as an int32 (dsize, 3) array of {source index, coefficient 0,
    coefficient 1}: the float sequence of include/convnet_hip.h, step by step in the types it names."""
    scale = 1.0 / (dsize / float(ssize))                                       # double
    fx = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(fx).astype(np.int64)
    fx = fx - s.astype(np.float32)                                             # float
    low, high = s < 0, s >= ssize - 1
    s[low], fx[low] = 0, 0
    s[high], fx[high] = ssize - 1, 0
    taps = np.empty((dsize, 3), np.int32)
    taps[:, 0] = s
    taps[:, 1] = np.rint((np.float32(1) - fx) * np.float32(2048))              # round half even, in float
    taps[:, 2] = np.rint(fx * np.float32(2048))
    return taps


def Bilinear(image, col_taps, row_taps):
    """One 8-bit bilinear resize of (h, w, 3) bytes by the taps of its columns and rows: integers only."""
    h, w = image.shape[:2]
    p = image.astype(np.int32)
    sx, sy = col_taps[:, 0], row_taps[:, 0]
    a0, a1 = col_taps[:, 1][None, :, None], col_taps[:, 2][None, :, None]
    rows = (p[:, sx] * a0 + p[:, np.minimum(sx + 1, w - 1)] * a1) >> 4         # (h, new_w, 3)
    b0, b1 = row_taps[:, 1][:, None, None], row_taps[:, 2][:, None, None]
    out = (((b0 * rows[sy]) >> 16) + ((b1 * rows[np.minimum(sy + 1, h - 1)]) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def ResizedSize(w, h, raw_y, raw_x):
    """(new_w, new_h) of Resize (:173-187): the image covers raw_y x raw_x, one side exactly; integer division."""
    if raw_x * h < raw_y * w:
        return (w * raw_y) // h, raw_y
    return raw_x, (h * raw_x) // w


def ImageTaps(w, h, new_w, new_h):
    """The taps stage_images_u8 takes for one image: (column taps, row taps) of resizeOCV's two passes seen from the destination — the
    width pass's columns and the height pass's rows; the other direction of either pass keeps its size and is the identity."""
    return Taps(w, new_w), Taps(h, new_h)


def Resize(image, raw_y, raw_x):
    """Resize + resizeOCV (:22-30): no resample when both sizes match, else first the width at the old height, then the height, each a
    full 8-bit bilinear resize of its own."""
    h, w = image.shape[:2]
    new_w, new_h = ResizedSize(w, h, raw_y, raw_x)
    if new_w == w and new_h == h:
        return image
    if new_w < 1 or new_h < 1:
        raise SystemExit(f"An image of {w} x {h} pixels resizes to {new_w} x {new_h}: nothing is left of it.")
    wide = Bilinear(image, Taps(w, new_w), Taps(h, h))
    return Bilinear(wide, Taps(new_w, new_w), Taps(h, new_h))


def ResizeTo(image, new_h, new_w):
    """resizeOCV applied unconditionally, as RawVideoFileIterator::GetNext does (src/video_iterators.cc:160): the image stretched to
    new_h x new_w, no aspect ratio kept, nothing cropped — first the width at the old height, rounded to a byte, then the height
    (include/convnet_hip.h: h(y), then result).  The same size gives the same bytes: both passes are then the identity."""
    h, w = image.shape[:2]
    if new_w < 1 or new_h < 1:
        raise SystemExit(f"{new_w} x {new_h} is not an image size.")
    wide = Bilinear(image, Taps(w, new_w), Taps(h, h))
    return Bilinear(wide, Taps(new_w, new_w), Taps(h, new_h))


# ---- positions and crops ----------------------------------------------------------------------------------------------------------------------
def Coordinates(width, height, position, size_y, size_x):
    """GetCoordinates (:143-171): (left, top, mirrored) of ``position``: centre, top-left, top-right, bottom-right, bottom-left, then the
    same five mirrored."""
    x_slack, y_slack = width - size_x, height - size_y
    left, top = [(x_slack // 2, y_slack // 2), (0, 0), (x_slack, 0), (x_slack, y_slack), (0, y_slack)][position % 5]
    return left, top, position >= 5


def PlanarCrop(image, left, top, size_y, size_x, mirrored):
    """ExtractRGB + getData (:60-87, 322-334): the crop, mirrored or not, as 3 * size_y * size_x bytes, planar R, G, B."""
    crop = image[top:top + size_y, left:left + size_x]
    if mirrored:
        crop = crop[:, ::-1]
    return np.ascontiguousarray(crop.transpose(2, 0, 1)).reshape(-1)


class ImageReader:
    """RawImageFileIterator<unsigned char> behind the row reader's protocol (hdf5io.RowReader's): row ``r`` of the stream is position
    ``r % positions`` of file ``r // positions``; ``positions`` is 10 with ``avg10_full_image`` and 1 without, where position 0 is also
    what the reference's random-access Get gives.  ``Seek`` / ``Tell`` count rows of the stream."""

    def __init__(self, files, size_y, size_x, raw_y, raw_x, avg10, parallel, layer_name):
        self.files_, self.layer_name_ = list(files), layer_name
        self.size_y_, self.size_x_, self.raw_y_, self.raw_x_ = size_y, size_x, raw_y, raw_x
        self.positions_ = 10 if avg10 else 1
        self.parallel_ = bool(parallel)
        self.num_files_ = len(self.files_)
        self.row_ = 0
        self.num_reads_ = 0      # files decoded so far
        self.last_ = (-1, None)  # the file resized last: consecutive positions share it (image_id_ / image_, :308-320)

    def GetDataSetSize(self):
        return self.positions_ * self.num_files_

    def SetMaxDataSetSize(self, max_dataset_size):          # caps the FILES (:124-129)
        if 0 < max_dataset_size < self.num_files_:
            self.num_files_ = max_dataset_size

    def GetDims(self):
        return NUM_COLORS * self.size_y_ * self.size_x_

    def GetStoredType(self):
        return np.dtype(np.uint8)

    def Seek(self, row):
        self.row_ = row

    def Tell(self):
        return self.row_

    def FileAndPosition(self, row):
        return divmod(row, self.positions_)

    def FilesOf(self, row_start, row_end):
        """The files rows ``row_start:row_end`` come from, each once, in order."""
        return list(range(row_start // self.positions_, (row_end - 1) // self.positions_ + 1))

    def Decode(self, files):
        """The decoded images of the files numbered ``files``, checked against what a crop needs."""
        images = ReadImages([self.files_[i] for i in files], self.parallel_)
        self.num_reads_ += len(files)
        for i, image in zip(files, images):
            h, w = image.shape[:2]
            new_w, new_h = ResizedSize(w, h, self.raw_y_, self.raw_x_)
            if new_w < self.size_x_ or new_h < self.size_y_:
                raise SystemExit(f"Data stream for layer {self.layer_name_}: {self.files_[i]} ({w} x {h}) resizes to {new_w} x {new_h}, "
                                 f"smaller than the image_size crop of {self.size_x_} x {self.size_y_}.")
        return images

    def Get(self, out, row_start, row_end):
        """Rows ``row_start:row_end`` into ``out`` (float32 or uint8), resized and cropped on the host: the float form's path."""
        if row_start < 0 or row_end <= row_start or row_end > self.GetDataSetSize():
            raise IndexError(f"Invalid start / end {row_start} {row_end}")
        dims = self.GetDims()
        rows = out.reshape(-1)[:(row_end - row_start) * dims].reshape(row_end - row_start, dims)
        files = [f for f in self.FilesOf(row_start, row_end) if f != self.last_[0]]
        resized = {f: Resize(image, self.raw_y_, self.raw_x_) for f, image in zip(files, self.Decode(files))}
        resized[self.last_[0]] = self.last_[1]
        for i, row in enumerate(range(row_start, row_end)):
            f, position = self.FileAndPosition(row)
            image = resized[f]
            left, top, mirrored = Coordinates(image.shape[1], image.shape[0], position, self.size_y_, self.size_x_)
            rows[i] = PlanarCrop(image, left, top, self.size_y_, self.size_x_, mirrored)
        self.last_ = (f, resized[f])

    def GetNext(self, out):
        self.Get(out, self.row_, self.row_ + 1)
        self.row_ = (self.row_ + 1) % self.GetDataSetSize()

    def close(self):
        self.last_ = (-1, None)
