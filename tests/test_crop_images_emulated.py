"""crop_images_u8 (convnet_amd/csrc/input_staging.hip) executed FUNCTIONALLY on the CPU through the C ABI — the real kernel source
compiled as host C++ against tests/emu/hip/hip_runtime.h (tests/emu/crop_images_emu_main.cc) — against a direct evaluation of the
definition: six crop sizes at four output alignments inside a guarded buffer, then tables of random numbers, which may give any pixels
but must stay inside the buffers, and the error codes.  No GPU; not a product path."""
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


def test_crop_images_kernel_runs_correctly_in_emulation(tmp_path):
    cc = _clang()
    if not cc:
        pytest.skip("no clang++ (the kernels use clang's vector extensions)")
    flags = ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(HERE, "emu"), "-I", os.path.join(ROOT, "convnet_amd", "csrc"), "-Wno-everything"]
    jobs = [(os.path.join(ROOT, "convnet_amd", "csrc", "input_staging.hip"), str(tmp_path / "input_staging.o"),
             ["-include", os.path.join(HERE, "emu", "crop_images_emu_prelude.h")]),
            (os.path.join(HERE, "emu", "crop_images_emu_main.cc"), str(tmp_path / "crop_images_emu_main.o"), [])]
    for src, obj, extra in jobs:
        r = subprocess.run([cc, *flags, *extra, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, src + "\n" + r.stdout + r.stderr
    exe = str(tmp_path / "crop_images_emu")
    subprocess.run([cc, *[o for _, o, _ in jobs], "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert r.returncode == 0 and lines and lines[-1] == "ALL PASSED", r.stdout + r.stderr
    assert sum(l.startswith("PASS W=") for l in lines) == 24
