"""resize_frames_u8 of convnet_amd/csrc/input_staging.hip executed FUNCTIONALLY on the CPU through the C ABI — the real kernel source
compiled as host C++ against tests/emu/hip/hip_runtime.h (tests/emu/resize_frames_emu_main.cc) — against a direct scalar evaluation of
the definition in 64-bit integers, compared with memcmp.  The geometries of tests/test_resize_frames_gpu.py and one whose width shrinks
past what a tile stages (the scalar arm), mirrored and not, at four source and output alignments inside guarded buffers; tap tables with
random source indices, which must give the definition's bytes under the entry's clamps; the error codes in their precedence.  No GPU;
not a product path."""
import os

import emu_build


def test_resize_frames_u8_runs_correctly_in_emulation(tmp_path):
    exe = emu_build.build(tmp_path, ["input_staging.hip"], "resize_frames_emu_main.cc", "the kernels use clang's vector extensions",
                          extras={"input_staging.hip": ["-include", os.path.join(emu_build.EMU, "input_staging_emu_prelude.h")]})
    lines = emu_build.run(exe, timeout=600)
    assert sum(l.startswith("PASS frames ") for l in lines) == 18             # 9 geometries x 2 mirror values
    assert sum(l.startswith("PASS wild ") for l in lines) == 10               # 5 geometries x 2 mirror values
    assert sum(l == "PASS errors" for l in lines) == 1
    assert lines[-1] == "ALL PASSED"
