"""The IMAGE_RAW stream's arithmetic once more, in scalar loops and sharing no code with the package: the taps of a bilinear pass, the
8-bit pass itself, Resize (two passes, first the width), GetCoordinates and the planar crop (reference src/image_iterators.cc:22-30,
60-87, 143-187).  This restates the DEFINITION of include/convnet_hip.h (stage_images_u8) — OpenCV's 8-bit INTER_LINEAR as its generic C
path computes it; it is not a recording of an OpenCV build.  Plain Python integers; float32 steps go through numpy scalars."""
import numpy as np

F = np.float32


def taps(ssize, dsize):
    """[(source index, coefficient 0, coefficient 1)] of a pass from ssize to dsize samples."""
    scale = 1.0 / (dsize / float(ssize))
    out = []
    for d in range(dsize):
        fx = F((d + 0.5) * scale - 0.5)
        s = int(np.floor(fx))
        fx = F(fx - F(s))
        if s < 0:
            s, fx = 0, F(0)
        if s >= ssize - 1:
            s, fx = ssize - 1, F(0)
        out.append((s, int(np.rint(F(F(1) - fx) * F(2048))), int(np.rint(fx * F(2048)))))
    return out


def resize_row(row, dsize):
    """One row of bytes through a width pass: the first pass, rounded to a byte."""
    w = len(row)
    out = []
    for s, a0, a1 in taps(w, dsize):
        x = int(row[s]) * a0 + int(row[min(s + 1, w - 1)]) * a1
        out.append((((2048 * (x >> 4)) >> 16) + 2) >> 2)
    return out


def width_pass(image, new_w):
    h, w, c = image.shape
    out = np.zeros((h, new_w, c), np.uint8)
    for y in range(h):
        for k in range(c):
            out[y, :, k] = resize_row(image[y, :, k], new_w)
    return out


def height_pass(image, new_h):
    h, w, c = image.shape
    out = np.zeros((new_h, w, c), np.uint8)
    for r, (s, b0, b1) in enumerate(taps(h, new_h)):
        for x in range(w):
            for k in range(c):
                p0, p1 = int(image[s, x, k]), int(image[min(s + 1, h - 1), x, k])
                out[r, x, k] = (((b0 * ((2048 * p0) >> 4)) >> 16) + ((b1 * ((2048 * p1) >> 4)) >> 16) + 2) >> 2
    return out


def resized_size(w, h, raw_y, raw_x):
    if raw_x * h < raw_y * w:
        return (w * raw_y) // h, raw_y
    return raw_x, (h * raw_x) // w


def resize(image, raw_y, raw_x):
    """(h, w, 3) bytes resized to cover raw_y x raw_x; untouched when it already has the size."""
    h, w = image.shape[:2]
    new_w, new_h = resized_size(w, h, raw_y, raw_x)
    if (new_w, new_h) == (w, h):
        return image
    return height_pass(width_pass(image, new_w), new_h)


def coordinates(width, height, position, size_y, size_x):
    """(left, top, mirrored) of a position 0 ... 9 in a resized image of width x height."""
    x_slack, y_slack = width - size_x, height - size_y
    p = position % 5
    if p == 0:
        left, top = x_slack // 2, y_slack // 2
    elif p == 1:
        left, top = 0, 0
    elif p == 2:
        left, top = x_slack, 0
    elif p == 3:
        left, top = x_slack, y_slack
    else:
        left, top = 0, y_slack
    return left, top, position >= 5


def planar_crop(image, left, top, size_y, size_x, mirrored):
    """The crop as a flat array: all of R, then G, then B, rows top to bottom; mirrored: columns right to left."""
    out = np.zeros(3 * size_y * size_x, np.uint8)
    for k in range(3):
        for r in range(size_y):
            for c in range(size_x):
                out[(k * size_y + r) * size_x + c] = image[top + r, left + (size_x - 1 - c if mirrored else c), k]
    return out


def row(image, raw_y, raw_x, size_y, size_x, position):
    """A row of the stream: the file's decoded image -> resized -> crop at position -> planar bytes."""
    big = resize(image, raw_y, raw_x)
    left, top, mirrored = coordinates(big.shape[1], big.shape[0], position, size_y, size_x)
    return planar_crop(big, left, top, size_y, size_x, mirrored)


def write_ppm(path, image):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (image.shape[1], image.shape[0]))
        f.write(np.ascontiguousarray(image, np.uint8).tobytes())


def write_pgm(path, grey):
    with open(path, "wb") as f:
        f.write(b"P5\n# a comment\n%d %d\n255\n" % (grey.shape[1], grey.shape[0]))
        f.write(np.ascontiguousarray(grey, np.uint8).tobytes())
