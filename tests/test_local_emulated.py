"""The locally connected layer kernels (convnet_amd/csrc/local_conv.hip) executed FUNCTIONALLY on the CPU through the C ABI — the real
kernel source compiled as host C++ against tests/emu/hip/hip_runtime.h (tests/emu/local_emu_main.cc) — on three small ragged
geometries (N % 4 != 0, C = 3, F % 4 != 0, rectangular kernels and strides, stride > kernel), both matrix paths, scaleTargets 0 / 1,
scaleOutput != 1, and a guard region after the bank gradient.  No GPU; not a product path."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _clang():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


def test_local_kernels_run_correctly_in_emulation(tmp_path):
    cc = _clang()
    if not cc:
        pytest.skip("no clang++ (the kernels use clang's vector extensions and __bf16)")
    flags = ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(HERE, "emu"), "-I", os.path.join(ROOT, "convnet_amd", "csrc"), "-Wno-everything"]
    jobs = [(os.path.join(ROOT, "convnet_amd", "csrc", "local_conv.hip"), str(tmp_path / "local_conv.o")),
            (os.path.join(HERE, "emu", "local_emu_main.cc"), str(tmp_path / "local_emu_main.o"))]
    for src, obj in jobs:
        r = subprocess.run([cc, *flags, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, src + "\n" + r.stdout + r.stderr
    exe = str(tmp_path / "local_emu")
    subprocess.run([cc, *[o for _, o in jobs], "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert r.returncode == 0 and lines and lines[-1] == "ALL PASSED", r.stdout + r.stderr
    assert sum(l.startswith("PASS local path=0") for l in lines) == 3 and sum(l.startswith("PASS local path=1") for l in lines) == 3
