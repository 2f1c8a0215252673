"""ctypes binding of libacr_hip.so.  Prototypes, enumerators and structs are read from the C ABI's one statement,
include/acr_hip.h (_abi.py): nothing of it is restated here.

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  If the shared object is
missing, or a call returns a negative status, this module raises -- loudly -- instead of degrading.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C acr_wsss_amd/csrc``.
"""
import ctypes
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# ACR_LIB_PATH: a lab build of the same library (scripts/lab/_build/*.so, e.g. EXTRA=-DLAB_TL stamps) for A/B runs
LIB_PATH = os.environ.get("ACR_LIB_PATH") or os.path.join(_HERE, "libacr_hip.so")

_C = _abi.constants
ACR_F32, ACR_BF16, ACR_BF16_F32MATH, ACR_F32_BF16X3 = (_C[k] for k in ("ACR_F32", "ACR_BF16", "ACR_BF16_F32MATH", "ACR_F32_BF16X3"))
# acr_math: how an fp32 entry point multiplies -- a per-call argument.  "f32": exact-fp32 MFMA; "f32_split": six bf16-MFMA terms
# of a three-way operand split (fp32 tensors, fp32 accumulate, fp32-accurate)
MATH = {"f32": _C["ACR_MATH_F32"], "f32_split": _C["ACR_MATH_BF16X3"], "f32_fp16x2": _C["ACR_MATH_FP16X2"]}
BF16_F32MATH = False      # True: bf16 tensors take the exact-fp32 MFMA kernels (reference for the bf16-MFMA ones)
GETAM_FUNCS = {k: _C["ACR_GETAM_" + k.upper()] for k in ("grad", "cam_grad", "grad_s", "cam_grad_s")}

c_void_p, c_int32, c_int64, c_float, c_size_t = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                  ctypes.c_float, ctypes.c_size_t)

AttnDesc = _abi.structs["acr_attn_desc"]
# name -> (restype, argtypes) of every entry point the header declares
SIGNATURES = _abi.prototypes

# acr_option: the kernel-variant selector of the library's explicit option table, name -> code.  Set through set_option() by a
# test only (it cross-checks two delta kernels that both ship); every other A/B the table once served is settled and retired
#  -- the library itself never reads the environment.
OPTIONS = {"attn_delta_1head": _C["ACR_OPT_ATTN_DELTA_1HEAD"]}

_lib = None


def set_option(name, value):
    """Select a kernel variant (A/B measurement switch; acr_set_option in include/acr_hip.h)."""
    check(load().acr_set_option(OPTIONS[name], int(value)), "acr_set_option")


class AcrHipError(RuntimeError):
    pass


def load():
    """Load libacr_hip.so (once).  Raises AcrHipError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AcrHipError(
                "libacr_hip.so not found at %s -- the HIP extension is the product path and there is no "
                "fallback.  Build it: python -c 'import __graft_entry__ as g; g.build()'" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        if lib.acr_version() != _C["ACR_ABI_VERSION"]:
            raise AcrHipError("libacr_hip.so ABI version %d != %d (rebuild it: __graft_entry__.build())"
                              % (lib.acr_version(), _C["ACR_ABI_VERSION"]))
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise AcrHipError("%s failed (%d): %s" % (what, rc, load().acr_last_error().decode()))


def workspace(query, *dims, device, dtype=torch.uint8):
    """(tensor, nbytes) of the workspace the size query ``query`` (an ``acr_*_ws_bytes``) asks for at ``dims``: allocated on
    ``device`` as ``dtype`` elements.  A negative answer is the library's refusal and raises with its message, before anything
    is allocated."""
    nbytes = getattr(load(), query)(*dims)
    if nbytes < 0:
        check(-1, query)
    return torch.empty(nbytes // dtype.itemsize, dtype=dtype, device=device), nbytes


def stream_ptr():
    """Raw hipStream_t of torch's current stream (kernels are enqueued there; graph-capturable)."""
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def dtype_code(dt):
    if dt == torch.float32:
        return ACR_F32
    if dt == torch.bfloat16:
        return ACR_BF16_F32MATH if BF16_F32MATH else ACR_BF16
    raise AcrHipError("unsupported dtype %s (fp32 and bf16 are built)" % dt)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise AcrHipError("acr_wsss_amd ops run on the GPU only (got a %s tensor); there is no CPU path"
                              % t.device)
