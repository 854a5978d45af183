"""What convnet_amd/csrc/conv3d.hip adds, executed FUNCTIONALLY on the CPU through the C ABI — the real source compiled as host C++
against tests/emu/hip/hip_runtime.h (tests/emu/conv3d_emu_main.cc): the frame slicing of the 3-D entries, the time gather of
convDown3DGemm (class banks of conv3d_dgrad_bank_kernel, uncovered frames) at C % 16 == 0 and its accumulating loop at other C, the frame accumulation of convOutp3DGemm, the fused
variants, the response-norm frame walk and pool3d_fwd_kernel / pool3d_undo_kernel, against a direct float64 evaluation of the
definitions.  Integer-valued operands make every sum exact: convolution (all directions) and max pooling compare exactly, average
pooling to fp32 rounding.  Guard regions before and after every output; the caller's cudamat structs byte-compared.  The 2-D convolution
kernels the 3-D entries launch per frame are replaced by plain loops there (response norm and pooling run pool_norm.hip itself) — the GPU suite runs the real ones.  No GPU; not a product path."""
import emu_build


def test_conv3d_kernels_run_correctly_in_emulation(tmp_path):
    # (pool_norm.hip: pooling over time, response norm)
    exe = emu_build.build(tmp_path, ["conv3d.hip", "pool_norm.hip"], "conv3d_emu_main.cc", "the kernels use clang's vector extensions")
    lines = emu_build.run(exe, timeout=600)
    assert sum(l.startswith("PASS conv3d plain") for l in lines) == 7 and sum(l.startswith("PASS conv3d fused") for l in lines) == 7
    assert sum(l.startswith("PASS pool3d") for l in lines) == 9 and sum(l.startswith("PASS rnorm3d") for l in lines) == 1
