"""What tests/test_video2hdf5_cpu.py and tests/test_video2hdf5_gpu.py share: three videos of random bytes written from a seed — a directory
of binary PPM frames named f_1 ... f_12 (so natural order differs from bytewise order), a 5-frame APNG of another size and a 3-page grey
TIFF — their list, a labels file, and the frames as arrays.  A plain module (tests/ is on the path), no fixture of its own."""
import os

import numpy as np

import image_ref

SIZES = [(11, 9), (8, 6), (7, 10)]         # (w, h) of the three videos' frames
COUNTS = [12, 5, 3]
LABELS = [3, 1, 2]


def write(directory):
    from PIL import Image
    rng = np.random.default_rng(2110)
    d = str(directory)
    frames = []
    clip = os.path.join(d, "clip")
    os.mkdir(clip)
    os.mkdir(os.path.join(clip, "sub"))                      # skipped
    with open(os.path.join(clip, ".hidden"), "w") as f:      # skipped
        f.write("not a frame")
    w, h = SIZES[0]
    for i in range(COUNTS[0]):
        frames.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        image_ref.write_ppm(os.path.join(clip, f"f_{i + 1}.ppm"), frames[-1])
    w, h = SIZES[1]
    apng = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(COUNTS[1])]
    pages = [Image.fromarray(a, "RGB") for a in apng]
    pages[0].save(os.path.join(d, "moving.png"), save_all=True, append_images=pages[1:])
    frames += apng
    w, h = SIZES[2]
    grey = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(COUNTS[2])]
    pages = [Image.fromarray(a, "L") for a in grey]
    pages[0].save(os.path.join(d, "pages.tiff"), save_all=True, append_images=pages[1:])
    frames += [np.ascontiguousarray(np.broadcast_to(a[:, :, None], a.shape + (3,))) for a in grey]
    f = dict(dir=d, videos=[clip, os.path.join(d, "moving.png"), os.path.join(d, "pages.tiff")], frames=frames,
             list=os.path.join(d, "videos.txt"), labels=os.path.join(d, "labels.txt"))
    with open(f["list"], "w") as h:
        h.write("\n".join(f["videos"]) + "\n")
    with open(f["labels"], "w") as h:
        h.write(" ".join(map(str, LABELS)) + "\n")
    return f


def read(path, names=("data", "labels")):
    """The named datasets of an HDF5 file as arrays (None where the file has none)."""
    from convnet_amd import hdf5io
    out = []
    with hdf5io.File(path) as h:
        for name in names:
            if not h.Has(name):
                out.append(None)
                continue
            r = h.RowReader(name)
            a = np.empty((r.GetDataSetSize(), r.GetDims()), np.uint8 if r.GetStoredType() == np.uint8 else np.float32)
            r.Get(a, 0, len(a))
            r.close()
            out.append(a)
    return out
