"""ctypes binding of libvqa_mi355x.so (C ABI: include/vqa_mi355x.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent,
``lib()`` raises.  Build it with ``python __graft_entry__.py build`` (hipcc, gfx950).
"""
import ctypes
import os
import threading

from . import _abi, _srchash

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VQA_LIB_PATH", os.path.join(_HERE, "libvqa_mi355x.so"))  # env override: profiling builds


class VqaLibraryError(RuntimeError):
    """libvqa_mi355x.so or its header is missing, stale, or a call returned an error code."""


def _read_header():
    path = os.path.join(_srchash.INCLUDE, "vqa_mi355x.h")
    if not os.path.exists(path):
        raise VqaLibraryError(
            "C ABI header %s not found: the binding of libvqa_mi355x.so is derived from it (signatures, structs, constants).  "
            "There is no handwritten copy to fall back to." % path)
    with open(path, "r") as fh:
        return _abi.parse(fh.read())


_functions, _structs, DEFINES = _read_header()          # DEFINES: name -> int, every integer #define VQA_* of the header
# SIGNATURES: name -> (restype, argtypes) and PARAMS: name -> parameter names, every symbol the header declares, in its order
SIGNATURES, PARAMS = _abi.signatures(_functions)
# STRUCTS: header name -> its ctypes.Structure (`VqaGemmProblem`), fields in the header's names and order
STRUCTS = {name: _abi.struct_class(name, fields) for name, fields in _structs.items()}
ABI_VERSION = DEFINES["VQA_ABI_VERSION"]

_lock = threading.Lock()
_lib = None


def lib():
    """Load (once) and return the ctypes handle.  Raises VqaLibraryError -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise VqaLibraryError(
                "HIP extension %s not found: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU or PyTorch fallback for this path." % LIB_PATH)
        try:
            handle = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the host's ROCm install
            raise VqaLibraryError("cannot load %s: %s" % (LIB_PATH, e)) from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise VqaLibraryError("%s does not export %s (stale build?)" % (LIB_PATH, name)) from e
            fn.restype = res
            fn.argtypes = args
        if handle.vqa_version() != ABI_VERSION:
            raise VqaLibraryError("ABI version mismatch: library %d, binding %d" % (handle.vqa_version(), ABI_VERSION))
        _lib = handle
    return _lib


def set_option(name, value):
    """Override (str / int) or clear (None) one of the library's VQA_* knobs for the rest of the process.  The library
    reads each knob from the environment once, at its first use; this is the explicit way to change one afterwards
    (tests, tools) -- never between the forward and the backward of an op."""
    v = None if value is None else str(value).encode()
    check(lib().vqa_set_option(name.encode(), v), "set_option")


def check(rc, what):
    if rc != 0:
        msg = lib().vqa_last_error()
        raise VqaLibraryError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def built_from_this_tree():
    """(library's vqa_source_hash(), hash of the source tree beside it): equal when the loaded binary was built from the sources
    in vqa_playground_pytorch_amd/csrc + include/ as they are now.  __graft_entry__.smoke() and tests/test_host_cpu.py assert
    it, so a stale .so that travelled to the GPU box is seen there."""
    return (lib().vqa_source_hash() or b"").decode(), _srchash.source_hash()
