"""The four byte-staging entries of convnet_amd/csrc/input_staging.hip executed FUNCTIONALLY on the CPU through the C ABI — the real
kernel source compiled as host C++ against tests/emu/hip/hip_runtime.h (tests/emu/input_staging_emu_main.cc) — each against a direct
scalar evaluation of its definition, exact to the bit.  crop_images_u8: six crop sizes at four output alignments inside a guarded
buffer, then tables of random numbers, which may give any pixels but must stay inside the buffers.  stage_images_u8: the same tables
and crops through the float cast, mean / std and a jittered patch, 3 and 65 cases, and the random tables.  stage_patches_u8 and
stage_clips_u8 (both grid modes): 3 x 5 x 70 into patches of 4 x 66 for 1, 5, 37, 64 and 68 cases.  All four (norm, jitter) builds of
the three staging kernels, and the entries' error codes in their precedence.  No GPU; not a product path."""
import os

import emu_build


def test_input_staging_kernels_run_correctly_in_emulation(tmp_path):
    exe = emu_build.build(tmp_path, ["input_staging.hip"], "input_staging_emu_main.cc", "the kernels use clang's vector extensions",
                          extras={"input_staging.hip": ["-include", os.path.join(emu_build.EMU, "input_staging_emu_prelude.h")]})
    lines = emu_build.run(exe, timeout=600)
    assert sum(l.startswith("PASS W=") for l in lines) == 24                  # crop_images_u8: 6 crops x 4 alignments
    assert sum(l.startswith("PASS patches N=") for l in lines) == 20          # 5 batch sizes x 4 builds
    assert sum(l.startswith("PASS clips T=3 grid=1") for l in lines) == 20 and sum(l.startswith("PASS clips T=3 grid=2") for l in lines) == 20
    assert sum(l.startswith("PASS images W=") for l in lines) == 16           # 2 crops x 2 batch sizes x 4 builds
    assert sum(l == "PASS errors" for l in lines) == 1
