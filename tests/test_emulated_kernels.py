"""The library's GEMM-shaped kernels executed FUNCTIONALLY on the CPU: the real kernel sources (convnet_amd/csrc/gather_gemm.hip,
patch_gemm.hip, wgrad_wide.hip) compiled as host C++ against tests/emu/hip/hip_runtime.h (every thread of a block a fiber; wave
collectives, the MFMAs in the register layouts the kernels assume, LDS-DMA as an immediate copy) and run on small problems against a
double-precision reference (tests/emu/emu_main.cc).
* The default kernels, through the C ABI (convUp / convDown / convOutpBias / dot: ggp_kernel incl. its generic-k mode and the
  stride-class table, gg_kernel, wg_kernel in both tile sizes with the bias row, the slab reduces).  They are green on hardware: here
  they are the calibration of the harness, and a functional check of the product kernels that needs no GPU.
* gpw_kernel and wgw_kernel (and their variants) — written after the last hardware run of their round — through their own launchers.
* The HBM-bound kernels of the path through the C ABI against the CPU oracle (oracle/liboracle.so): max pooling and its undo (both
  undo kernels), cross-map response normalisation and its undo, the fused SGD step.
No GPU; not a product path.  What this cannot see: timing, late-landing loads (tests/test_patch_wide_cpu.py / test_wgrad_wide_cpu.py model
those), the M0 range above 84 KB, instruction hazards.  CONVNET_EMU_ALL=1 runs every case (~5 minutes) instead of a subset (~1.5)."""
import os

import pytest

import emu_build


SOURCES = ["gather_gemm.hip", "patch_gemm.hip", "wgrad_wide.hip", "fewc_conv.hip", "pool_norm.hip", "elementwise.hip"]


@pytest.fixture(scope="module")
def emu_binary(tmp_path_factory):
    oracle_dir = os.path.join(emu_build.ROOT, "oracle")
    if not os.path.exists(os.path.join(oracle_dir, "liboracle.so")):
        pytest.skip("oracle/liboracle.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    return emu_build.build(tmp_path_factory.mktemp("emu"), SOURCES, "emu_main.cc", "the kernels use clang's vector extensions and __bf16",
                           link_args=["-L", oracle_dir, "-loracle", "-Wl,-rpath," + oracle_dir])


def test_wide_kernels_run_correctly_in_emulation(emu_binary):
    which = "all" if os.environ.get("CONVNET_EMU_ALL") else "quick"
    lines = emu_build.run(emu_binary, which, timeout=1200)
    # the calibration cases and both new kernels really ran
    assert any(l.startswith("PASS abi convUp") for l in lines) and any(l.startswith("PASS abi convOutpBias") for l in lines)
    assert any(l.startswith("PASS gpp(raw)") for l in lines) and any(l.startswith("PASS gpw fprop") for l in lines)
    assert any(l.startswith("PASS gpw dgrad") for l in lines) and any(l.startswith("PASS wgw wgrad") for l in lines)
    # gpv_kernel: conv2's forward form and its four stride classes (the latter through convDown)
    assert any(l.startswith("PASS gpv fprop") for l in lines) and any(l.startswith("PASS abi convDown") and "k5 s2" in l and "gpw_kernel(dgrad)" in l for l in lines)
    # the library's own state.hip is what runs: a parked convUp absorbed the two element-wise calls behind it, same bits as eager
    assert any(l.startswith("PASS abi deferred convUp") and "2 deferred; 0 of" in l for l in lines)


def test_wide_wgrad_kernel_single_block_epilogue_in_emulation(emu_binary):
    """one block per tile (forced: the launch policy splits the reduction at emulation sizes): scaleTargets, scaleOutput and the bias
    row in the kernel's own epilogue, through the 16-byte write-out and through the direct one (F % 4 != 0)"""
    lines = emu_build.run(emu_binary, "wgwfin", timeout=1200)
    assert sum("splits=1 " in l and l.startswith("PASS wgw") for l in lines) == 2, lines


def test_wide_patch_kernel_tail_split_in_emulation(emu_binary):
    """11 tiles on an 8-slot "chip": the last round's three tiles are cut into three K-ranges (the kernel's tail-split branch, its raw
    partial tiles, gpw_tail_fix_kernel) — forced by the harness, the cost model never picks it at emulation sizes"""
    lines = emu_build.run(emu_binary, "gpwtail", timeout=1200)
    assert "tail_splits=3" in lines[0], lines


def test_group_patch_kernel_tail_split_in_emulation(emu_binary):
    """gpv_kernel (5 x 5 stride 2: superchunks of three and two chunks): 13 tiles on an 8-slot "chip", the last round's five tiles cut
    into three K-ranges whose borders fall inside a tap row's groups"""
    lines = emu_build.run(emu_binary, "gpvtail", timeout=1200)
    assert "tail_splits=3" in lines[0], lines


def test_split_builds_error_against_double_in_emulation(emu_binary):
    """The precision half of parity, before any GPU run: every split build emulation runs (gfc_kernel, generic-k and tap-major
    ggp_kernel, gg_kernel rc and kc, gpw_kernel, gpv_kernel's stride classes, wg_kernel 2,2,2,2 and x16 with the bias row, the FC NT /
    NN / TN products) on N(0,1) data and on data whose terms cancel in pairs along the axis each product reduces over, against double:
    max |out - exact| / sum|ab| within tests/emu/prec.h's bounds.  The 1e-4 parity cases above cannot tell a dropped cross term from
    rounding; these can (the bounds' calibration against the m*m-dropped and zero-l-plane mutants is in tests/emu/prec.h)."""
    lines = emu_build.run(emu_binary, "prec", timeout=1200)
    assert sum(l.startswith("PASS prec") for l in lines) == 32, lines
