"""``python -m convnet_amd.train_convnet --board B --model M --train T [--val V]`` — apps/train_convnet.cc: set up the board, build the
net from the model pbtxt, attach the datasets named by the two DatasetConfig pbtxt files, allocate and train.  One board only: the
reference's several-boards form is model parallelism (MultiGPUConvNet), which is not built here."""
import argparse
import sys

from .convnet import ConvNet
from .matrix import Matrix


def ParseBoardIds(board):
    """ParseBoardIds (src/util.cc): one digit per board, "0" or "012"."""
    if not board.isdigit():
        raise SystemExit(f"--board takes board digits such as 0 or 012, not {board!r}")
    return [int(c) for c in board]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m convnet_amd.train_convnet", description=__doc__.split("\n\n")[0])
    ap.add_argument("--board", "-b", default="", help="GPU board: 0, 1, ...")
    ap.add_argument("--model", "-m", default="", help="Model pbtxt file")
    ap.add_argument("--train", "-t", default="", help="Training data pbtxt file")
    ap.add_argument("--val", "-v", default="", help="Validation data pbtxt file")
    ap.add_argument("--unfused", action="store_true", help="run the reference's unfused Matrix-call sequence instead of the fused entries")
    args = ap.parse_args(argv)
    if not args.board or not args.model:
        ap.print_help()
        return 1
    boards = ParseBoardIds(args.board)
    if len(boards) > 1:
        raise SystemExit(f"--board {args.board}: {len(boards)} boards ask for a model-parallel net, which is not built; name one board.")
    Matrix.SetupCUDADevice(boards[0])
    print(f"Using board {boards[0]}")
    net = ConvNet(args.model, fused=not args.unfused, verbose=True)
    net.SetupDataset(args.train, args.val)
    net.AllocateMemory(False)
    net.Train()
    net.train_dataset_.close()
    if getattr(net, "val_dataset_", None) is not None:
        net.val_dataset_.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
