"""Generates the fixtures that let tests/test_host_cpu.py check the python host against the reference's own model files and
config schema without the reference tree:

    ref_model_signatures.json   model_signature() of the reference's example nets (examples/imagenet/CLS_net_*.pbtxt,
                                examples/mnist-conv/net.pbtxt) as read by convnet_amd/pbtxt.py
    ref_config_schema.json      every field (type, label, declared default) of the messages pbtxt.py restates and every enum's
                                value names, from proto/convnet_config.proto parsed by oracle/seam/gen_config_pb.py
    pixel_mean.h5               examples/imagenet/pixel_mean.h5 (a data file the reference writes through HDF5), copied as is

Run where the reference tree is available:

    python tests/golden/make_reference_fixtures.py <reference tree>
"""
import importlib.util
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from convnet_amd import pbtxt  # noqa: E402
from test_host_cpu import REF_MODELS, SCHEMA_MESSAGES, model_signature  # noqa: E402


def main(ref):
    sigs = {path: model_signature(pbtxt.read(os.path.join(ref, "examples", path))) for path in REF_MODELS}
    with open(os.path.join(HERE, "ref_model_signatures.json"), "w") as f:
        json.dump(sigs, f, indent=0)
        f.write("\n")
    spec = importlib.util.spec_from_file_location("gen_config_pb", os.path.join(ROOT, "oracle", "seam", "gen_config_pb.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ref, "proto", "convnet_config.proto")) as f:
        msgs = {m.name: m for m in gen.flatten(gen.parse(f.read()))}
    schema = {"messages": {name: msgs[name].fields for name in SCHEMA_MESSAGES},
              "enums": {e: [v for v, _ in vals] for m in msgs.values() for e, vals in m.enums}}
    with open(os.path.join(HERE, "ref_config_schema.json"), "w") as f:
        json.dump(schema, f, indent=1, sort_keys=True)
        f.write("\n")
    shutil.copyfile(os.path.join(ref, "examples", "imagenet", "pixel_mean.h5"), os.path.join(HERE, "pixel_mean.h5"))
    print("wrote", ", ".join(sorted(sigs)), "signatures, the schema of", ", ".join(SCHEMA_MESSAGES), "and pixel_mean.h5")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
