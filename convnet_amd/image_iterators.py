"""Image files as a data stream: ``data_type: IMAGE_RAW`` — ImageDataIterator over RawImageFileIterator<unsigned char>
(src/datahandler.cc:723-796, src/image_iterators.cc:89-334).  A text file lists the images; every image is decoded, resized so that it
covers ``raw_image_size`` (``Resize``, :173-187), and a row of the stream is the ``image_size`` crop at one of the positions of
``GetCoordinates`` (:143-171), mirrored or not, as planar R, G, B bytes (``getData``, :60-87).

The resize is the reference's ``resizeOCV``: two 8-bit bilinear resizes, first the width at the old height, then the height.  What this
module (and ``stage_images_u8``, which resamples the crop's pixels on the GPU from the same taps) computes is the DEFINITION written down
in include/convnet_hip.h — OpenCV's 8-bit INTER_LINEAR as its generic C path computes it — and the tests pin that definition, not an
OpenCV build: none was at hand to compare with (NOTES.md).

``jitter_raw_image`` (:189-202, 231-285) puts a random translated crop, a zoom and a rotation of the decoded image in front of the
resize, drawn anew for every chunk: ``JitterStream`` is the engine's float stream, ``Transform`` the arithmetic, and the rotation is
again a written definition (include/convnet_hip.h: stage_images_jitter_u8, which does the same on the GPU from host-built tables).

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


# ---- jitter_raw_image: the random crop, zoom and rotation of the decoded image ------------------------------------------------------------------
REF_PI = 3.14159265        # the reference's own PI (src/image_iterators.cc:10), used for the rotated size alone


class JitterStream:
    """The float stream of RawImageFileIterator's ``std::default_random_engine`` (libstdc++: minstd_rand0) seeded with 0 (:108, state 1)
    behind a ``uniform_real_distribution<float>(0, 1)``: x = 16807 x mod (2^31 - 1), u = float(x - 1) / float(2^31 - 2), and the float
    below 1 where that rounds to 1."""
    MODULUS, MULTIPLIER = 2147483647, 16807

    def __init__(self):
        self.x_ = 1

    def Draws(self, count):
        """The next ``count`` values of the distribution, as float32."""
        x, m, a = self.x_, self.MODULUS, self.MULTIPLIER
        states = np.empty(count, np.int64)
        for i in range(count):
            x = a * x % m
            states[i] = x
        self.x_ = x
        u = (states - 1).astype(np.float32) / np.float32(m - 1)
        u[u >= np.float32(1)] = np.nextafter(np.float32(1), np.float32(0))
        return u

    def Sample(self, chunk_size, max_angle, min_scale):
        """SampleNoiseDistributions (:189-202): (angle, trans_x, trans_y, scale) of entries 0 ... chunk_size - 1 as float32 arrays, drawn
        entry by entry in that order.  ``max_angle_`` is a const int there, so the config's float is truncated; the angle goes through
        double, the scale stays in float."""
        u = self.Draws(4 * chunk_size).reshape(chunk_size, 4)
        angle = ((2 * int(max_angle)) * (u[:, 0].astype(np.float64) - 0.5)).astype(np.float32)
        low = np.float32(min_scale)
        scale = low + (np.float32(1) - low) * u[:, 3]
        return angle, u[:, 1].copy(), u[:, 2].copy(), scale.astype(np.float32)


def CropRect(w, h, tx, ty, scale, size_x, size_y):
    """(left, top, width, height) of the region Transform (:243-266) crops from a w x h image: the maximal region of the aspect
    size_x : size_y, both sides divided by ``scale`` only where it exceeds 1 (int / float in float, truncated), placed by the two
    translations (int * float in float, truncated)."""
    if size_x * h < size_y * w:
        sx, sy = (size_x * h) // size_y, h
    else:
        sx, sy = w, (size_y * w) // size_x
    scale = np.float32(scale)
    if scale > np.float32(1):
        sx, sy = int(np.float32(sx) / scale), int(np.float32(sy) / scale)
    return int(np.float32(w - sx) * np.float32(tx)), int(np.float32(h - sy) * np.float32(ty)), sx, sy


def RotSize(angle, size_x, size_y):
    """(RX, RY) (:272-274): the size the crop is resized to before it is rotated, so that the central size_x x size_y window of a
    square has no border: the sum of sine and cosine in double with the reference's PI, as a float, times the size in float."""
    t = float(abs(np.float32(angle))) * REF_PI / 180
    rot_scale = np.float32(np.sin(t) + np.cos(t))
    return int(np.float32(size_x) * rot_scale), int(np.float32(size_y) * rot_scale)


def RotationTables(RX, RY, angle):
    """The integer tables of the rotation by ``angle`` degrees about (RX // 2, RY // 2) as include/convnet_hip.h writes them down
    (stage_images_jitter_u8): int64 arrays (adelta[RX], bdelta[RX], X0[RY], Y0[RY]) in 1/1024 of a source pixel.  Doubles; rint rounds
    half to even."""
    t = float(np.float32(angle)) * (np.pi / 180)
    a, b = float(np.cos(t)), float(np.sin(t))
    cx, cy = RX // 2, RY // 2
    M = [a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy]
    D = 1 / (M[0] * M[4] - M[1] * M[3])
    i0, i4, i1, i3 = M[4] * D, M[0] * D, -M[1] * D, -M[3] * D
    i2, i5 = -i0 * M[2] - i1 * M[5], -i3 * M[2] - i4 * M[5]
    x, y = np.arange(RX, dtype=np.float64), np.arange(RY, dtype=np.float64)
    return (np.rint(i0 * x * 1024).astype(np.int64), np.rint(i3 * x * 1024).astype(np.int64),
            np.rint((i1 * y + i2) * 1024).astype(np.int64) + 16, np.rint((i4 * y + i5) * 1024).astype(np.int64) + 16)


def RotationSource(tables):
    """(sy, sx, fy, fx) of every destination pixel of the rotation with ``tables``: the source pixel and the 1/32 fractions."""
    adelta, bdelta, X0, Y0 = tables
    X, Y = (X0[:, None] + adelta[None, :]) >> 5, (Y0[:, None] + bdelta[None, :]) >> 5
    return Y >> 5, X >> 5, Y & 31, X & 31


def Rotate(image, angle):
    """(RY, RX, 3) bytes rotated by ``angle`` degrees about (RX // 2, RY // 2) into an image of the same size: the fixed-point bilinear
    warp of include/convnet_hip.h, border 0.  Integers only behind the tables."""
    RY, RX = image.shape[:2]
    sy, sx, fy, fx = RotationSource(RotationTables(RX, RY, angle))
    padded = np.zeros((RY + 2, RX + 2, image.shape[2]), np.int64)            # R(., .) with its border of zeros
    padded[1:-1, 1:-1] = image
    y0, x0 = np.clip(sy, -1, RY) + 1, np.clip(sx, -1, RX) + 1
    y1, x1 = np.clip(sy + 1, -1, RY) + 1, np.clip(sx + 1, -1, RX) + 1
    fy, fx = fy[:, :, None], fx[:, :, None]
    out = ((32 - fx) * (32 - fy) * padded[y0, x0] + fx * (32 - fy) * padded[y0, x1] + (32 - fx) * fy * padded[y1, x0]
           + fx * fy * padded[y1, x1] + 512) >> 10
    return out.astype(np.uint8)


def TransformCrop(crop, angle, size_x, size_y, rot_size=None):
    """What Transform (:268-284) makes of the region it has cropped: angle 0, the two-pass resize to size_y x size_x; else the resize to
    RotSize, the rotation, and the central size_y x size_x window.  ``rot_size``: (RX, RY) in place of RotSize's."""
    if np.float32(angle) == 0:
        return ResizeTo(crop, size_y, size_x)
    RX, RY = rot_size or RotSize(angle, size_x, size_y)
    if RX < size_x or RY < size_y:
        raise SystemExit(f"A rotation by {float(angle):g} degrees resizes to {RX} x {RY}, smaller than the {size_x} x {size_y} window.")
    left, top = RX // 2 - size_x // 2, RY // 2 - size_y // 2
    return Rotate(ResizeTo(crop, RY, RX), angle)[top:top + size_y, left:left + size_x]


def Transform(image, angle, tx, ty, scale, size_x, size_y):
    """RawImageFileIterator::Transform (:243-285): the random translated crop, zoom and rotation of a decoded image, to size_y x size_x."""
    h, w = image.shape[:2]
    left, top, sx, sy = CropRect(w, h, tx, ty, scale, size_x, size_y)
    if sx < 1 or sy < 1:
        raise SystemExit(f"An image of {w} x {h} pixels leaves a crop of {sx} x {sy}: nothing is left of it.")
    return TransformCrop(image[top:top + sy, left:left + sx], angle, size_x, size_y)


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

    def __init__(self, files, size_y, size_x, raw_y, raw_x, avg10, parallel, layer_name, jitter=False, max_angle=0, min_scale=0):
        self.files_, self.layer_name_ = list(files), layer_name
        self.jitter_, self.max_angle_, self.min_scale_ = bool(jitter), int(max_angle), float(min_scale)     # (a const int there, :94)
        self.stream_ = JitterStream() if jitter else None
        self.noise_ = None       # (angle, trans_x, trans_y, scale) of entries 0 ... chunk_size - 1, drawn by Prep
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

    def Prep(self, chunk_size):
        """ImageDataIterator::Prep (src/datahandler.cc:774-776): once per DiskAccess, before any row is loaded, the jitter of entries
        0 ... chunk_size - 1 is drawn anew.  (The image kept from the last row goes with the jitter it was made with — NOTES.md.)"""
        if self.jitter_:
            self.noise_ = self.stream_.Sample(chunk_size, self.max_angle_, self.min_scale_)
            self.last_ = (-1, None)

    def JitterOf(self, f):
        """(angle, trans_x, trans_y, scale) of file ``f``: entry f % chunk_size (AddRandomJitter, :231-240) — the file's row in the list,
        not its place in the chunk."""
        if self.noise_ is None:
            raise SystemExit(f"Data stream for layer {self.layer_name_}: jitter_raw_image needs Prep before a row is read.")
        k = f % len(self.noise_[0])
        return tuple(v[k] for v in self.noise_)

    def JitterGeometry(self, f, w, h):
        """What the jitter of file ``f`` makes of its w x h image: (left, top, crop width, crop height, angle, RX, RY), RX x RY being the
        size the crop is resized to — the raw size without a rotation."""
        angle, tx, ty, scale = self.JitterOf(f)
        left, top, sx, sy = CropRect(w, h, tx, ty, scale, self.raw_x_, self.raw_y_)
        if sx < 1 or sy < 1:
            raise SystemExit(f"Data stream for layer {self.layer_name_}: {self.files_[f]} ({w} x {h}) leaves a jitter_raw_image crop of "
                             f"{sx} x {sy}: nothing is left of it.")
        RX, RY = RotSize(angle, self.raw_x_, self.raw_y_) if angle != 0 else (self.raw_x_, self.raw_y_)
        return left, top, sx, sy, angle, RX, RY

    def Jittered(self, f, image):
        """AddRandomJitter (:231-240) of file ``f``'s decoded image: raw_y x raw_x pixels, which Resize then leaves alone."""
        left, top, sx, sy, angle, RX, RY = self.JitterGeometry(f, image.shape[1], image.shape[0])
        return TransformCrop(image[top:top + sy, left:left + sx], angle, self.raw_x_, self.raw_y_, (RX, RY))

    def Decode(self, files):
        """The decoded images of the files numbered ``files``, checked against what a crop needs."""
        images = ReadImages([self.files_[i] for i in files], self.parallel_)
        self.num_reads_ += len(files)
        if self.jitter_:         # (every jittered image has the raw size, which holds the crop)
            return images
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
        resized = {f: Resize(self.Jittered(f, image) if self.jitter_ else image, self.raw_y_, self.raw_x_)
                   for f, image in zip(files, self.Decode(files))}
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
