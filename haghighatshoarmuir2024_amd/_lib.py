"""ctypes binding of libmicloc_hip.so (the C-ABI declared in include/micloc_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, this module raises.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmicloc_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "micloc_hip.h")


class MiclocError(RuntimeError):
    pass


c_double_p = ctypes.POINTER(ctypes.c_double)
c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_size_t = ctypes.c_size_t


class MiclocConfig(ctypes.Structure):
    _fields_ = [
        ("device", c_int),
        ("num_mic", c_int),
        ("stht_len", c_int),
        ("stht_kernel", c_double_p),
        ("iir_len", c_int),
        ("iir_b", c_double_p),
        ("iir_a", c_double_p),
        ("robust_width", c_int),
        ("bipolar", c_int),
    ]


class MiclocSynthArgs(ctypes.Structure):
    _fields_ = [
        ("time", c_void_p), ("sig", c_void_p), ("slopes", c_void_p),
        ("T", c_int), ("B", c_int), ("K", c_int), ("M", c_int),
        ("delays", c_void_p),
        ("doa", c_void_p),
        ("moving", c_int),
        ("r_vec", c_void_p), ("theta_vec", c_void_p),
        ("speed", ctypes.c_double),
        ("shift", c_void_p),
        ("gain", c_void_p),
        ("mode", c_int),
        ("fs", ctypes.c_double),
        ("x", c_void_p),
    ]


_SCALARS = {"int": c_int, "size_t": c_size_t, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
_PROTOTYPE = re.compile(r"\b((?:const\s+)?\w+[\s*]+)(micloc_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, symbol, is_return=False):
    """The ctypes type of a return type or of a parameter (its type, then its name) as the header spells it.  There is no default: a type
    outside the mapping raises."""
    ctype = decl if is_return else re.sub(r"\w+\s*$", "", decl)
    stars = ctype.count("*")
    base = " ".join(w for w in ctype.replace("*", " ").split() if w != "const")
    if stars >= 2:  # T **, T *const *: an array of handles or an out-handle
        return ctypes.POINTER(c_void_p)
    if stars == 1:  # host or device memory: the header cannot say which
        return ctypes.c_char_p if is_return and base == "char" else c_void_p
    if is_return and base == "void":
        return None
    if base not in _SCALARS:
        raise MiclocError(f"{symbol}: no ctypes mapping for '{' '.join(decl.split())}'")
    return _SCALARS[base]


def parse_header(text):
    """(symbols, constants) of the header text: name -> (restype, argtypes) for every prototype, and the value of every integer
    `#define MICLOC_*` and `micloc_status` enumerator."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    symbols = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        params = [] if params.strip() == "void" else params.split(",")
        symbols[name] = (_ctype(ret, name, True), [_ctype(p, name) for p in params])
    constants = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MICLOC_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)
    status = re.search(r"enum\s*\{([^}]*)\}\s*micloc_status\b", text)
    constants += re.findall(r"(MICLOC_\w+)\s*=\s*(-?\d+)", status.group(1)) if status else []
    return symbols, {name: int(value) for name, value in constants}


if not os.path.exists(HEADER_PATH):
    raise MiclocError(f"{HEADER_PATH} not found: the binding is derived from the header, which lies next to the package")
with open(HEADER_PATH) as _f:
    # SYMBOLS: every symbol include/micloc_hip.h declares, name -> (restype, argtypes); the MICLOC_* constants become attributes
    SYMBOLS, _constants = parse_header(_f.read())
globals().update(_constants)

_lib = None


def load():
    """Load libmicloc_hip.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MiclocError(
                f"{LIB_PATH} not found: build it with `make -C haghighatshoarmuir2024_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback"
            )
        # PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64; it must be in the process BEFORE this library
        # is loaded so that both resolve to ONE HIP runtime (same SONAME).  Loaded the other way round, the two
        # runtimes each try to own the device and hipGetDeviceCount() fails in the second one.
        import torch  # noqa: F401

        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(status, what=""):
    if status == MICLOC_OK:
        return
    lib = load()
    msg = lib.micloc_status_string(status).decode()
    if status == MICLOC_ERR_HIP:
        msg += f" [hipError_t {lib.micloc_last_hip_error()}]"
    if status == MICLOC_ERR_SHAPE:
        raise ValueError(f"micloc {what}: {msg}")
    raise MiclocError(f"micloc {what}: {msg} (status {status})")
