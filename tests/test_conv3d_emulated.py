"""What convnet_amd/csrc/conv3d.hip adds, executed FUNCTIONALLY on the CPU through the C ABI — the real source compiled as host C++
against tests/emu/hip/hip_runtime.h (tests/emu/conv3d_emu_main.cc): the frame slicing of the 3-D entries, the time gather of
convDown3DGemm (class banks of conv3d_dgrad_bank_kernel, uncovered frames) at C % 16 == 0 and its accumulating loop at other C, the frame accumulation of convOutp3DGemm, the fused
variants, the response-norm frame walk and pool3d_fwd_kernel / pool3d_undo_kernel, against a direct float64 evaluation of the
definitions.  Integer-valued operands make every sum exact: convolution (all directions) and max pooling compare exactly, average
pooling to fp32 rounding.  Guard regions before and after every output; the caller's cudamat structs byte-compared.  The 2-D convolution
kernels the 3-D entries launch per frame are replaced by plain loops there (response norm and pooling run pool_norm.hip itself) — the GPU suite runs the real ones.  No GPU; not a product path."""
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


def test_conv3d_kernels_run_correctly_in_emulation(tmp_path):
    cc = _clang()
    if not cc:
        pytest.skip("no clang++ (the kernels use clang's vector extensions)")
    flags = ["-std=c++17", "-O1", "-x", "c++", "-I", os.path.join(HERE, "emu"), "-I", os.path.join(ROOT, "convnet_amd", "csrc"), "-Wno-everything"]
    jobs = [(os.path.join(ROOT, "convnet_amd", "csrc", "conv3d.hip"), str(tmp_path / "conv3d.o")),
            (os.path.join(ROOT, "convnet_amd", "csrc", "pool_norm.hip"), str(tmp_path / "pool_norm.o")),   # pooling over time, response norm
            (os.path.join(HERE, "emu", "conv3d_emu_main.cc"), str(tmp_path / "conv3d_emu_main.o"))]
    for src, obj in jobs:
        r = subprocess.run([cc, *flags, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, src + "\n" + r.stdout + r.stderr
    exe = str(tmp_path / "conv3d_emu")
    subprocess.run([cc, *[o for _, o in jobs], "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert r.returncode == 0 and lines and lines[-1] == "ALL PASSED", r.stdout + r.stderr
    assert sum(l.startswith("PASS conv3d plain") for l in lines) == 7 and sum(l.startswith("PASS conv3d fused") for l in lines) == 7
    assert sum(l.startswith("PASS pool3d") for l in lines) == 9 and sum(l.startswith("PASS rnorm3d") for l in lines) == 1
