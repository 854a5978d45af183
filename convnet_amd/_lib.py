"""ctypes binding of libconvnet_hip.so — the same kind of binding the reference ships for its own
C ABI (cudamat/cudamat.py:9-135, cudamat/cudamat_conv_gemm.py:4-117), with every restype / argtypes read from the prototypes of
include/convnet_hip.h: a new entry needs its prototype there and nothing here, unless it brings a new type (_CTYPES).

The product path has NO CPU fallback: if the HIP library is missing, import raises."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libconvnet_hip.so")
# A/B runs of tools/ against another BUILD of the same library (e.g. the previous round's, lib/libconvnet_hip_r03.so): entry points
# that build lacks are skipped.  Never set by the product, the tests or bench.py's measured legs.
_ALT_LIB = os.environ.get("CONVNET_HIP_LIB")
if _ALT_LIB:
    LIB_PATH = _ALT_LIB if os.path.isabs(_ALT_LIB) else os.path.join(_HERE, "lib", _ALT_LIB)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "convnet_hip.h")

c_float_p = ctypes.POINTER(ctypes.c_float)


class cudamat(ctypes.Structure):
    """Mirror of ``struct cudamat`` (include/convnet_hip.h; reference cudamat/cudamat.py:127-135)."""
    _fields_ = [("data_host", c_float_p),
                ("data_device", ctypes.c_void_p),
                ("on_device", ctypes.c_int),
                ("on_host", ctypes.c_int),
                ("size", ctypes.c_int * 2),
                ("is_trans", ctypes.c_int),
                ("owns_data", ctypes.c_int),
                ("tex_obj", ctypes.c_ulonglong)]


class Shape4D(ctypes.Structure):
    _fields_ = [("shape", ctypes.c_int * 4)]


class ConvDesc(ctypes.Structure):
    """Mirror of ``struct ConvDesc`` (reference cudamat/cudamat.py:137-190)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "num_input_channels", "num_output_channels", "kernel_size_y", "kernel_size_x", "kernel_size_t",
        "stride_y", "stride_x", "stride_t", "padding_y", "padding_x", "padding_t",
        "input_channel_begin", "input_channel_end", "output_channel_begin", "output_channel_end", "num_groups")]

    def copy(self):
        c = ConvDesc()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(self), ctypes.sizeof(ConvDesc))
        return c


class rnd_struct(ctypes.Structure):
    _fields_ = [("dev_mults", ctypes.c_void_p), ("dev_words", ctypes.c_void_p)]


class KernelInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("flops", ctypes.c_double), ("grid_blocks", ctypes.c_int), ("split_k", ctypes.c_int)]


# C type spelling (whitespace normalised, `*` attached to the type) -> ctypes type: the whole type vocabulary of include/convnet_hip.h.
# A prototype that uses a spelling missing here fails the import (header_signatures): there is no default.
_CTYPES = {
    "void": None, "int": ctypes.c_int, "unsigned int": ctypes.c_uint, "long": ctypes.c_long, "size_t": ctypes.c_size_t,
    "float": ctypes.c_float, "double": ctypes.c_double, "bool": ctypes.c_bool,
    "void*": ctypes.c_void_p, "void**": ctypes.POINTER(ctypes.c_void_p), "char*": ctypes.c_char_p, "const char*": ctypes.c_char_p,
    "int*": ctypes.POINTER(ctypes.c_int), "float*": c_float_p, "const float*": c_float_p, "double*": ctypes.POINTER(ctypes.c_double),
    "cudamat*": ctypes.POINTER(cudamat), "cudamat**": ctypes.POINTER(ctypes.POINTER(cudamat)), "Shape4D*": ctypes.POINTER(Shape4D),
    "ConvDesc": ConvDesc, "rnd_struct*": ctypes.POINTER(rnd_struct), "ConvnetHipKernelInfo*": ctypes.POINTER(KernelInfo)}


def _ctype(decl, named, proto):
    """The ctypes type of a return type (named=False) or of a parameter declaration.  A parameter's type is the text before its
    trailing identifier.  An unnamed parameter has none, so the last token is dropped only when it can be a name: when there is more
    than one token, the text does not end in `*`, and the whole text is not itself a known type (`unsigned int`)."""
    tok = decl.replace("*", " * ").split()
    spell = lambda t: " ".join(t).replace(" *", "*")   # noqa: E731
    if named and len(tok) > 1 and tok[-1] != "*" and spell(tok) not in _CTYPES:
        tok = tok[:-1]
    if spell(tok) not in _CTYPES:
        raise ImportError(f"include/convnet_hip.h: '{proto}' uses the type '{spell(tok)}', which convnet_amd/_lib.py (_CTYPES) does not map")
    return _CTYPES[spell(tok)]


def header_signatures(text):
    """{name: (restype, [argtypes])} of every prototype in the extern "C" block of a header like include/convnet_hip.h, whose prototypes
    hold no function pointers, arrays or macros."""
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = body[body.index('extern "C" {'):]
    sigs = {}
    for res, name, args in re.findall(r"^[ \t]*([A-Za-z_][\w \t*]*?)\s*\b(\w+)\s*\(([^();{}]*)\)\s*;", body, flags=re.M):
        proto = f"{' '.join(res.split())} {name}({' '.join(args.split())})"
        args = [a for a in args.split(",") if a.split() not in ([], ["void"])]
        sigs[name] = (_ctype(res, False, proto), [_ctype(a, True, proto) for a in args])
    return sigs


def declared_symbols(header_path=HEADER_PATH):
    """Every function name declared in include/convnet_hip.h."""
    return sorted(header_signatures(open(header_path).read()))


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    # torch must be imported BEFORE the dlopen: the library's libamdhip64 dependency then resolves (by
    # SONAME) to the HIP runtime torch already loaded, so both share ONE runtime — required, because torch
    # streams and device pointers are handed straight to the library.  Loading ours first pulls in
    # /opt/rocm's copy and hipSetDevice later fails with two runtimes in the process.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in header_signatures(open(HEADER_PATH).read()).items():
        if _ALT_LIB and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()

_ERRORS = {  # reference src/util.cc:226-246 GetStringError
    -1: "Incompatible matrix dimensions.", -2: "CUBLAS error.", -3: "CUDA error: ", -4: "Operation not supported on views.",
    -5: "Operation not supported on transposed matrices.", -6: "Generic error.",
    -7: "Incompatible transposedness.", -8: "Matrix is not in device memory.", -9: "Operation not supported."}


def profile_enable(on=True):
    lib.convnet_hip_profile_enable(1 if on else 0)


def profile_report():
    """[{kernel, op, launches, ms, flops, bytes, executed}] for launches since the last report (flops = algorithmic work,
    executed = MFMA work issued, which is larger for dgrad gathers that run border taps on the zero page)."""
    buf = ctypes.create_string_buffer(1 << 16)
    n = lib.convnet_hip_profile_report(buf, len(buf))
    rows = []
    for line in buf.value.decode().splitlines() if n else []:
        k, op, cnt, ms, fl, by, ex = line.split("|")
        rows.append({"kernel": k, "op": op, "launches": int(cnt), "ms": float(ms), "flops": float(fl), "bytes": float(by), "executed": float(ex)})
    return rows


def GetStringError(err_code):
    msg = _ERRORS.get(err_code, "Unknown error")
    if err_code == -3:
        msg += lib.get_last_cuda_error().decode()
    return msg


def probe_matrix_pipe(random_operands=True, seconds=0.05):
    """{bf16_tflops, tflops_eq, ghz_counter, ghz_issue}: the sustained rate of a pure v_mfma_f32_32x32x16_bf16 stream on this chip
    (csrc/probe.hip: one wave per SIMD, register operands, nothing else issued) — the power-limited ceiling of the bf16-split kernels."""
    out = (ctypes.c_double * 4)()
    rc = lib.convnet_hip_probe_matrix_pipe(1 if random_operands else 0, float(seconds), out)
    if rc != 0:
        raise RuntimeError(f"convnet_hip_probe_matrix_pipe failed: {rc}")
    return {"bf16_tflops": out[0], "tflops_eq": out[1], "ghz_counter": out[2], "ghz_issue": out[3]}
