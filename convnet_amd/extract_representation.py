"""``python -m convnet_amd.extract_representation --board B --model M --feature-config F`` — apps/extract_representation.cc: set up the
board, build the net from the model pbtxt and run ``ExtractFeatures`` on the FeatureExtractorConfig pbtxt.  A model that carries a
``timestamp`` (the stamped pbtxt a training run writes beside its checkpoints) gets that run's checkpoint loaded once the net is allocated
(src/convnet.cc:300-307); otherwise the weights are what the edges' ``initialization`` says (PRETRAINED loads them).  One board only: the
reference's several-boards form is model parallelism (MultiGPUConvNet), which is not built here."""
import argparse
import sys

from .convnet import ConvNet
from .matrix import Matrix
from .train_convnet import ParseBoardIds


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m convnet_amd.extract_representation", description=__doc__.split("\n\n")[0])
    ap.add_argument("--board", "-b", default="", help="GPU board: 0, 1, ...")
    ap.add_argument("--model", "-m", default="", help="Model pbtxt file")
    ap.add_argument("--feature-config", "-f", default="", help="Feature extraction pbtxt file")
    ap.add_argument("--unfused", action="store_true", help="run the reference's unfused Matrix-call sequence instead of the fused entries")
    args = ap.parse_args(argv)
    if not args.board or not args.model or not args.feature_config:
        ap.print_help()
        return 1
    boards = ParseBoardIds(args.board)
    if len(boards) > 1:
        raise SystemExit(f"--board {args.board}: {len(boards)} boards ask for a model-parallel net, which is not built; name one board.")
    Matrix.SetupCUDADevice(boards[0])
    print(f"Using board {boards[0]}")
    net = ConvNet(args.model, fused=not args.unfused, verbose=True)
    rows = net.ExtractFeatures(args.feature_config, on_allocated=net.Load if net.model_.timestamp else None)
    for name, n in rows.items():
        print(f"Wrote {n} rows of {name}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
