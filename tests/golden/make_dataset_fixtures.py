"""Generates the fixtures of tests/test_datahandler_cpu.py that come from the reference tree:

    ref_dataset_schema.json     every field (type, label, declared default) of DataStreamConfig / DatasetConfig, from
                                proto/convnet_config.proto parsed by oracle/seam/gen_config_pb.py
    dataset_pbtxt/*.pbtxt       examples/mnist-conv/train_data.pbtxt and val_data.pbtxt, copied as they are (settings only)

Run where the reference tree is available:

    python tests/golden/make_dataset_fixtures.py <reference tree>
"""
import importlib.util
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MESSAGES = ("DataStreamConfig", "DatasetConfig")


def main(ref):
    spec = importlib.util.spec_from_file_location("gen_config_pb", os.path.join(ROOT, "oracle", "seam", "gen_config_pb.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ref, "proto", "convnet_config.proto")) as f:
        msgs = {m.name: m for m in gen.flatten(gen.parse(f.read()))}
    schema = {"messages": {name: msgs[name].fields for name in MESSAGES},
              "enums": {e: [v for v, _ in vals] for name in MESSAGES for e, vals in msgs[name].enums}}
    with open(os.path.join(HERE, "ref_dataset_schema.json"), "w") as f:
        json.dump(schema, f, indent=1, sort_keys=True)
        f.write("\n")
    os.makedirs(os.path.join(HERE, "dataset_pbtxt"), exist_ok=True)
    for name in ("train_data.pbtxt", "val_data.pbtxt"):
        shutil.copyfile(os.path.join(ref, "examples", "mnist-conv", name), os.path.join(HERE, "dataset_pbtxt", name))
    print("wrote the schema of", ", ".join(MESSAGES), "and the two mnist-conv dataset files")


if __name__ == "__main__":
    main(sys.argv[1])
