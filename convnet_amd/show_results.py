"""``python -m convnet_amd.show_results FILE.h5 [--dataset output] [--class-names FILE] [--top 10]`` — apps/show_results.py: the top
classes of every row of a feature file's dataset (the ``output`` layer's, as ``extract_representation`` writes it), with the reference's
lines of output: the split file name, then per row a rule and ``--top`` lines of class name and probability, best first.  A ``.txt`` file
is read as a text matrix.  The class names are the lines of ``--class-names`` (the reference's fixed ``class_names_CLS.txt``); without the
file a class is shown as its number."""
import argparse
import os
import sys

import numpy as np

from . import hdf5io


def ReadPredictions(path, dataset="output"):
    """(rows, classes) float array."""
    if os.path.splitext(path)[1] == ".txt":
        return np.atleast_2d(np.loadtxt(path))
    with hdf5io.File(path) as f:
        if not f.Has(dataset):
            raise SystemExit(f"{path} has no dataset {dataset}.")
        dims, rows = f.ReadHDF5Shape(dataset)            # a (rows, dims) dataset reads as a (dims, rows) column-major matrix
        return f.ReadHDF5CPU(dims * rows, dataset).reshape(rows, dims)


def TopClasses(predictions, top=10):
    """Per row the ``top`` class numbers, best first, as the reference sorts them: (-p).argsort()."""
    return [(-p).argsort()[:top].tolist() for p in predictions]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m convnet_amd.show_results", description=__doc__.split("\n\n")[0])
    ap.add_argument("file", help="feature file (.h5) or text matrix (.txt)")
    ap.add_argument("--dataset", default="output", help="dataset of the feature file")
    ap.add_argument("--class-names", default="class_names_CLS.txt", help="text file, one class name per line")
    ap.add_argument("--top", type=int, default=10, help="classes shown per row")
    args = ap.parse_args(argv)
    print(os.path.splitext(args.file))
    predictions = ReadPredictions(args.file, args.dataset)
    names = None
    if os.path.exists(args.class_names):
        with open(args.class_names) as f:
            names = [line.strip() for line in f]
    elif args.class_names != ap.get_default("class_names"):
        raise SystemExit(f"Could not open class names file : {args.class_names}")
    if names is not None and len(names) < predictions.shape[1]:
        raise SystemExit(f"{args.class_names} names {len(names)} classes, {args.file} has {predictions.shape[1]}.")
    for p, labels in zip(predictions, TopClasses(predictions, args.top)):
        print("----------------")
        for label in labels:
            print(names[label] if names is not None else label, p[label])
    return 0


if __name__ == "__main__":
    sys.exit(main())
