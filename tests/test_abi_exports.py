"""CPU: libconvnet_hip.so loads and exports every symbol include/convnet_hip.h declares, and the
ctypes struct mirrors have the reference's layout.  No compute calls (no GPU here)."""
import ctypes

import pytest

from convnet_amd import _lib


def test_every_declared_symbol_is_exported():
    names = _lib.declared_symbols()
    assert len(names) >= 75, names
    missing = [n for n in names if not hasattr(_lib.lib, n)]
    assert not missing, missing


def test_struct_layouts_match_reference_abi():
    # struct cudamat: 2 pointers + 6 ints + 64-bit slot = 48 bytes (cudamat/cudamat.cuh:28-37)
    assert ctypes.sizeof(_lib.cudamat) == 48
    assert _lib.cudamat.size.offset == 24 and _lib.cudamat.is_trans.offset == 32 and _lib.cudamat.tex_obj.offset == 40
    assert ctypes.sizeof(_lib.ConvDesc) == 64 and ctypes.sizeof(_lib.Shape4D) == 16
    assert _lib.ConvDesc.padding_y.offset == 32 and _lib.ConvDesc.num_groups.offset == 60


def test_version_and_error_strings():
    assert b"gfx950" in _lib.lib.convnet_hip_version()
    assert "dimensions" in _lib.GetStringError(-1)


def test_host_only_view_ops():
    # reshape / get_slice are pure host bookkeeping (cudamat.cu:587-626): callable without a GPU
    m = _lib.cudamat()
    m.size[0], m.size[1], m.on_device, m.data_device = 6, 4, 1, 4096
    assert _lib.lib.reshape(ctypes.byref(m), -1, 8) == 0 and (m.size[0], m.size[1]) == (3, 8)
    assert _lib.lib.reshape(ctypes.byref(m), 5, -1) == -1
    s = _lib.cudamat()
    assert _lib.lib.get_slice(ctypes.byref(m), ctypes.byref(s), 2, 5) == 0
    assert (s.size[0], s.size[1], s.owns_data) == (3, 3, 0) and s.data_device == 4096 + 2 * 3 * 4
    assert _lib.lib.get_slice(ctypes.byref(m), ctypes.byref(s), 5, 9) == -1


def test_library_default_matrix_path_is_ieee_fp32():
    """The C ABI's default is path 0 (v_mfma_f32_32x32x2_f32: exact fp32 products, inf / NaN as cublasSgemm gives them) — the
    bf16-split products are something a host selects (convnet_hip_set_matrix_path(1) or CONVNET_GG_SPLIT=1), as Matrix.SetupCUDADevice
    does for the Python trainer, the tests and bench.py.  No device call is made here."""
    import os
    import subprocess
    import sys
    code = "from convnet_amd import _lib; print(_lib.lib.convnet_hip_get_matrix_path(), _lib.lib.convnet_hip_get_patch_mode())"
    env = {k: v for k, v in os.environ.items() if k not in ("CONVNET_GG_SPLIT", "CONVNET_GG_PATCH")}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["0", "3"], out.stdout   # (the patch mode only matters on path 1: gpw_kernel where its launch policy applies)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, env=dict(env, CONVNET_GG_SPLIT="1"), timeout=300)
    assert out.stdout.split()[0] == "1", out.stdout


# ---- the binding is derived from the header (convnet_amd/_lib.py: header_signatures) ---------------------------------------------------
def test_every_prototype_is_bound_with_the_parsed_signature():
    import re
    text = open(_lib.HEADER_PATH).read()
    sigs = _lib.header_signatures(text)
    assert sorted(sigs) == _lib.declared_symbols() and len(sigs) >= 152
    # counted without the parser: every `name(...);` behind the comments is a prototype, and each one was parsed
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(re.findall(r"(\w+)\s*\([^;{]*\)\s*;", body[body.index('extern "C" {'):])) == sorted(sigs)
    for name, (res, args) in sigs.items():
        fn = getattr(_lib.lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == args and fn.restype is res, name


def test_pinned_signatures_cover_the_type_vocabulary():
    """Written out by hand from include/convnet_hip.h, not computed by the parser: together they use every entry of _lib._CTYPES."""
    C, P = ctypes, ctypes.POINTER
    I, F, M, S, Z = C.c_int, C.c_float, P(_lib.cudamat), P(_lib.Shape4D), C.c_size_t
    MM, FP = P(P(_lib.cudamat)), P(C.c_float)
    pins = {
        "dot": (I, [M, M, M, F, F]),
        "read_from": (F, [M, I, I, P(I)]),
        "get_slice": (I, [M, M, C.c_uint, C.c_uint]),
        "init_from_array": (None, [M, FP, I, I]),
        "convUpBiasAct": (None, [M, M, M, M, S, S, S, _lib.ConvDesc, F, I]),
        "ResponseNormCrossMap3DGemm": (None, [M, M, I, I, F, F, C.c_bool, I]),
        "sgd_momentum_step_multi": (I, [I, MM, MM, MM, FP, FP, FP, FP]),
        "adagrad_momentum_step_multi": (I, [I, MM, MM, MM, MM, FP, FP, FP, FP, FP, FP]),
        "convnet_hip_probe_matrix_pipe": (I, [I, C.c_double, P(C.c_double)]),
        "convnet_hip_profile_report": (Z, [C.c_char_p, Z]),
        "convnet_hip_comm_init": (I, [I, I, C.c_char_p]),
        "convnet_hip_comm_allreduce_avg": (I, [M, Z, Z, I]),
        "cuda_create_event": (I, [P(C.c_void_p)]),
        "convnet_hip_set_stream": (None, [C.c_void_p]),
        "convnet_hip_get_stream": (C.c_void_p, []),
        "convnet_hip_version": (C.c_char_p, []),
        "convnet_hip_deferred_absorbed": (C.c_long, []),
        "convnet_hip_last_kernel_info": (None, [P(_lib.KernelInfo)]),
        "init_random": (I, [P(_lib.rnd_struct), I]),
    }
    for name, (res, args) in pins.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    used = {t for res, args in pins.values() for t in [res] + args}
    assert used == set(_lib._CTYPES.values())


def test_a_type_outside_the_vocabulary_fails_the_parse_and_names_the_prototype():
    header = 'extern "C" {\nint fine(cudamat* mat, int n);\nint scale_rows(cudamat* mat, half* factors);\n}\n'
    with pytest.raises(ImportError, match=r"scale_rows\(.*half\*"):
        _lib.header_signatures(header)
    with pytest.raises(ImportError, match=r"unsigned long.*counter"):
        _lib.header_signatures('extern "C" {\nunsigned long counter(void);\n}\n')


def test_parser_handles_unnamed_parameters_void_and_multi_line_lists():
    C, P = ctypes, ctypes.POINTER
    header = '''/* a comment with a prototype in it: int ghost(int); */
typedef struct before { int (*not_ours)(int); } before;
extern "C" {
#define SOME_CODE -1
void* handle(void);
    void nothing();
int unnamed(cudamat*, unsigned int, const char* name, float);   /* trailing comment */
float spread(cudamat* a,
             Shape4D*  shape,   /* between the lines */
             ConvDesc conv_desc , cudamat * * list,
             const float *scales);
}
'''
    assert _lib.header_signatures(header) == {
        "handle": (C.c_void_p, []),
        "nothing": (None, []),
        "unnamed": (C.c_int, [P(_lib.cudamat), C.c_uint, C.c_char_p, C.c_float]),
        "spread": (C.c_float, [P(_lib.cudamat), P(_lib.Shape4D), _lib.ConvDesc, P(P(_lib.cudamat)), P(C.c_float)]),
    }
