"""Videos as frames: RawVideoFileIterator (src/video_iterators.cc:76-170) on what can be decoded here.  A text file lists the videos;
the reference opens each with OpenCV's VideoCapture, counts its frames in a first pass (:97-117), and GetNext (:150-165) hands out one
frame after the other, resized to a fixed size (resizeOCV, unconditionally) and mirrored.  This package has no video decoder, so a VIDEO
is one of
  * a directory: its regular files are the frames, in natural name order (f_2.ppm before f_10.ppm; dot files and sub-directories are
    skipped), each decoded by ``image_iterators.ReadImage``;
  * a file PIL opens: its ``n_frames`` frames in order (GIF, APNG, multi-page TIFF, animated WebP, ...), each through
    ``convert("RGB")`` as ``ReadImage`` does; a binary PPM / PGM is taken by ``DecodePNM`` first; a single-frame file is a video of one
    frame.
Compressed video (mp4, avi, ...) is refused by name.  What this module hands out are the DECODED frames at their original sizes: the
resize (``image_iterators.ResizeTo``, or resize_frames_u8 on the GPU) and the mirror belong to the caller, convnet_amd/video2hdf5.py.

numpy and PIL only; nothing here touches the GPU."""
import os
import re

import numpy as np

from . import image_iterators
from .image_iterators import ReadFileList as ReadVideoList  # noqa: F401  (each word is one video)

_RUNS = re.compile(rb"(\d+)")


def NaturalKey(name):
    """The sort key of a frame's file name: the name split into runs of digits and of anything else; digit runs compare as integers,
    the rest bytewise, and ties (f_02 and f_2) go by the whole name bytewise."""
    raw = os.fsencode(name)
    return [(0, int(run), b"") if run[:1].isdigit() else (1, 0, run) for run in _RUNS.split(raw) if run], raw


def FrameFiles(directory):
    """The frame files of a directory video, in natural order: its regular files but for dot files."""
    try:
        names = [n for n in os.listdir(directory) if not n.startswith(".") and os.path.isfile(os.path.join(directory, n))]
    except OSError as e:
        raise SystemExit(f"Could not list video directory : {directory} ({e})")
    if not names:
        raise SystemExit(f"Video directory {directory} holds no frame file.")
    return [os.path.join(directory, n) for n in sorted(names, key=NaturalKey)]


def _open_frames(path):
    """The PIL image of a multi-frame file, or the SystemExit that names what is missing."""
    from PIL import Image
    try:
        return Image.open(path)
    except Exception:
        raise SystemExit(f"{path} is neither a directory of frames nor an image file that can be opened: compressed video needs a "
                         "decoder this package does not have; extract the frames into a directory and list the directory.")


def _is_pnm(path):
    with open(path, "rb") as f:
        return image_iterators._pnm_header(f.read(512)) is not None


def CountFrames(videos):
    """The first pass (:97-117): the number of frames of every video, without decoding a pixel — a directory listing, or ``n_frames``."""
    counts = []
    for path in videos:
        if os.path.isdir(path):
            counts.append(len(FrameFiles(path)))
        elif not os.path.exists(path):
            raise SystemExit(f"Video {path} does not exist.")
        elif _is_pnm(path):
            counts.append(1)
        else:
            with _open_frames(path) as im:
                counts.append(int(getattr(im, "n_frames", 1)))
    return counts


def _checked(image, path, frame):
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise SystemExit(f"Error reading file {path} (frame {frame})")
    return image


def _read_frame_file(job):
    path, frame = job
    try:
        return image_iterators.ReadImage(path)
    except SystemExit:
        raise SystemExit(f"Error reading file {path} (frame {frame})")


def ReadFrames(path, first, last):
    """Frames ``first:last`` of one video, decoded at their original size as (h, w, 3) R, G, B bytes.  A frame that fails to decode
    stops the run (the reference goes on with the previous frame — NOTES.md)."""
    if os.path.isdir(path):
        jobs = [(name, first + i) for i, name in enumerate(FrameFiles(path)[first:last])]
        if len(jobs) < last - first:
            raise SystemExit(f"Error reading file {path} (frame {first + len(jobs)})")
        if len(jobs) < 2:
            return [_read_frame_file(j) for j in jobs]
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(image_iterators.MAX_DECODE_THREADS, len(jobs))) as pool:
            return list(pool.map(_read_frame_file, jobs))
    if not os.path.exists(path):
        raise SystemExit(f"Video {path} does not exist.")
    if _is_pnm(path):
        return [_read_frame_file((path, 0))][first:last]
    frames = []
    with _open_frames(path) as im:
        for i in range(first, last):            # (forward seeks: the frames of a span are decoded one after the other)
            try:
                im.seek(i)
                frames.append(_checked(np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8)), path, i))
            except SystemExit:
                raise
            except Exception:
                raise SystemExit(f"Error reading file {path} (frame {i})")
    return frames


class VideoReader:
    """RawVideoFileIterator by its method names, over decoded frames at their original sizes.  Frame ``f`` of the stream is frame
    ``f - start`` of the video whose frames start at ``start``: every frame of every video, in list order and frame order."""

    def __init__(self, videos):
        self.videos_ = list(videos)
        self.counts_ = CountFrames(self.videos_)
        self.starts_ = np.concatenate([[0], np.cumsum(self.counts_)]).astype(np.int64)
        self.dataset_size_ = int(self.starts_[-1])
        self.frame_ = 0

    def GetDataSetSize(self):
        return self.dataset_size_

    def SetMaxDataSetSize(self, max_dataset_size):          # caps the FRAMES
        if 0 < max_dataset_size < self.dataset_size_:
            self.dataset_size_ = int(max_dataset_size)

    def Seek(self, frame):
        self.frame_ = frame

    def Tell(self):
        return self.frame_

    def Get(self, first, last):
        """The decoded frames ``first:last`` of the stream; a span may cross videos."""
        if first < 0 or last <= first or last > self.dataset_size_:
            raise IndexError(f"Invalid start / end {first} {last}")
        frames = []
        v = int(np.searchsorted(self.starts_, first, side="right")) - 1
        while first < last:
            start, count = int(self.starts_[v]), self.counts_[v]
            if first < start + count:
                end = min(last, start + count)
                frames += ReadFrames(self.videos_[v], first - start, end - start)
                first = end
            v += 1
        return frames

    def GetNext(self):
        """The next frame of the stream; after the last one it starts over."""
        frame = self.Get(self.frame_, self.frame_ + 1)[0]
        self.frame_ = (self.frame_ + 1) % self.dataset_size_
        return frame
