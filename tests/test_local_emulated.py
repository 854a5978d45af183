"""The locally connected layer kernels (convnet_amd/csrc/local_conv.hip) executed FUNCTIONALLY on the CPU through the C ABI — the real
kernel source compiled as host C++ against tests/emu/hip/hip_runtime.h (tests/emu/local_emu_main.cc) — on three small ragged
geometries (N % 4 != 0, C = 3, F % 4 != 0, rectangular kernels and strides, stride > kernel), both matrix paths, scaleTargets 0 / 1,
scaleOutput != 1, and a guard region after the bank gradient.  No GPU; not a product path."""
import emu_build


def test_local_kernels_run_correctly_in_emulation(tmp_path):
    exe = emu_build.build(tmp_path, ["local_conv.hip"], "local_emu_main.cc", "the kernels use clang's vector extensions and __bf16")
    lines = emu_build.run(exe, timeout=600)
    assert sum(l.startswith("PASS local path=0") for l in lines) == 3 and sum(l.startswith("PASS local path=1") for l in lines) == 3
