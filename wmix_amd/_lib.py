"""ctypes binding of libwmix_amd.so (the only compute path; no fallback)."""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
# WMIX_AMD_LIB: another build of the same library (developer A/B runs of an experiment variant, tools_dev/); never a fallback
LIB_PATH = os.path.abspath(os.environ["WMIX_AMD_LIB"]) if os.environ.get("WMIX_AMD_LIB") else os.path.join(HERE, "libwmix_amd.so")
INCLUDE_DIR = os.path.join(os.path.dirname(HERE), "include")

# wmx_version() of the library these mirrors were written against (wmix_amd/csrc/wmx_core.hip)
EXPECTED_VERSION = 400

_lib = None


class WmxError(RuntimeError):
    pass


def lib():
    """Load libwmix_amd.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WmxError(
                "libwmix_amd.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C wmix_amd/csrc` (there is no CPU fallback)")
        # One HIP runtime per process: PyTorch-ROCm brings its own copy of libamdhip64 and loads it by path.  Loaded AFTER torch, this
        # library's `libamdhip64.so.N` dependency binds to that copy (same SONAME) and both sides share devices, streams and pointers;
        # loaded BEFORE torch, /opt/rocm's copy comes in as a second runtime, and the one that initialises second finds no device
        # ("no ROCm-capable device is detected").  The mirrors here always work next to torch (device memory, streams), so torch goes
        # first.  A C host has no torch and none of this (examples/*.c).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        # a library older than these bindings (a stale build, a path given in WMIX_AMD_LIB) must say so, not die in ctypes
        # (round-5 ADVICE): both checks come before anything else is read from it
        if getattr(L, "wmx_build_info", None) is None or getattr(L, "wmx_version", None) is None:
            raise WmxError("%s is older than these bindings (no wmx_build_info / wmx_version): rebuild it with `make -C wmix_amd/csrc`" % LIB_PATH)
        L.wmx_version.restype = C.c_int
        if L.wmx_version() != EXPECTED_VERSION:
            raise WmxError("%s is wmx_version %d, these bindings expect %d: rebuild it with `make -C wmix_amd/csrc`"
                           % (LIB_PATH, L.wmx_version(), EXPECTED_VERSION))
        L.wmx_build_info.restype = C.c_char_p
        L.wmx_build_info.argtypes = []
        info = L.wmx_build_info().decode(errors="replace")
        if info != "default" and os.environ.get("WMIX_AMD_ALLOW_VARIANT_BUILD") != "1":
            raise WmxError("%s is not the product build: wmx_build_info() = %r (a developer variant; set WMIX_AMD_ALLOW_VARIANT_BUILD=1 to "
                           "load it on purpose)" % (LIB_PATH, info))
        _bind(L)
        _lib = L
    return _lib


def build_info():
    """wmx_build_info() of the loaded library: "default", or the developer flags of a variant build."""
    return lib().wmx_build_info().decode(errors="replace")


def check(rc, what=""):
    if rc != 0:
        msg = lib().wmx_last_error().decode(errors="replace")
        raise WmxError("%s failed (rc=%d): %s" % (what or "wmx call", rc, msg))


def host_rows(ptr, shape, dtype):
    """numpy view of a pinned host buffer the library owns (the slots' rows of wmx_pipe, wmx_rt and wmx_conf): valid until the handle
    is destroyed"""
    import numpy as np
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=dtype).reshape(shape)


# ---------------------------------------------------------------- the signatures: read from include/*.h, bound once by lib()
# The scalar types the headers use.  Every pointer (`T *name`, `name[]`) is c_void_p whatever it points to -- None, an address
# (.data_ptr(), .ctypes.data), byref(...), pointer(...) and ctypes arrays all pass -- except a returned `const char *`: c_char_p.
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long": C.c_long, "size_t": C.c_size_t,
            "double": C.c_double, "float": C.c_float, "unsigned char": C.c_ubyte,
            "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16,
            "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}


class WMix_Point(C.Union):  # include/wmix_compat.h, field for field
    _fields_ = [("S8", C.c_void_p), ("U8", C.c_void_p), ("S16", C.c_void_p), ("U16", C.c_void_p), ("S32", C.c_void_p), ("U32", C.c_void_p)]


class WMix_Struct_Head(C.Structure):  # include/wmix_compat.h, field for field
    _fields_ = [("objAo", C.c_void_p), ("objAi", C.c_void_p), ("buff", C.c_void_p), ("start", WMix_Point), ("end", WMix_Point),
                ("head", WMix_Point), ("tail", WMix_Point), ("run", C.c_bool), ("loopWord", C.c_uint8), ("loopWordRecord", C.c_uint8),
                ("loopWordFifo", C.c_uint8), ("loopWordRtp", C.c_uint8), ("tick", C.c_uint32), ("thread_sys", C.c_uint32),
                ("thread_record", C.c_uint32), ("thread_play", C.c_uint32), ("playRun", C.c_bool), ("recordRun", C.c_bool),
                ("shmemRun", C.c_int), ("msg_key", C.c_int), ("msg_fd", C.c_int), ("reduceMode", C.c_uint8)]


# the aggregates that cross the boundary by value (wmix_load_data, wmx_compat_load_data)
_AGGREGATES = {"WMix_Point": WMix_Point, "WMix_Struct_Head": WMix_Struct_Head}
_TYPES = dict(_SCALARS, **_AGGREGATES)
_TYPE_WORDS = {w for t in _TYPES for w in t.split()}

_signatures = None
# names include/*.h declares that the loaded library does not export (a WMIX_AMD_LIB variant built from an older tree); empty for
# the product build (tests/test_abi.py)
unbound = []


def _ctype(func, decl, is_return=False):
    """One C type as it stands in a prototype -- a return type, or a parameter with or without its name -- as a ctypes type."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words or "[" in decl:
        return C.c_char_p if is_return and words == ["char", "*"] else C.c_void_p
    if is_return and words == ["void"]:
        return None
    if not is_return and len(words) > 1 and words[-1] not in _TYPE_WORDS:
        words = words[:-1]  # the parameter's name
    t = " ".join(words)
    if t not in _TYPES:
        raise WmxError("include/*.h: %s(): no ctypes type for %r (wmix_amd/_lib.py: _SCALARS, _AGGREGATES)" % (func, t))
    return _TYPES[t]


def parse_prototypes(src):
    """{name: (restype, [argtypes])} of every function prototype in the text of a header."""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r'extern\s*"C"\s*\{(.*)\}', r"\1", src, flags=re.S)
    src = re.sub(r"\btypedef\b[^;{]*(\{[^{}]*\})?[^;{]*;", "", src)
    table = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?)\b([A-Za-z_]\w*) ?\((.*)\)", stmt)
        if m is None:
            raise WmxError("include/*.h: not a function prototype: %r" % stmt)
        ret, name, params = m.groups()
        if "(" in params or ")" in params or not params.strip():
            raise WmxError("include/*.h: %s(): cannot split the parameter list %r" % (name, params))
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        if not all(params):
            raise WmxError("include/*.h: %s(): cannot split the parameter list %r" % (name, m.group(3)))
        table[name] = (_ctype(name, ret, is_return=True), [_ctype(name, p) for p in params])
    return table


def signatures():
    """{name: (restype, [argtypes])} of every function include/*.h declares; read once."""
    global _signatures
    if _signatures is None:
        try:
            headers = sorted(fn for fn in os.listdir(INCLUDE_DIR) if fn.endswith(".h"))
        except OSError as e:
            raise WmxError("the headers of libwmix_amd.so are not where these bindings read the signatures from: %s" % e)
        table = {}
        for fn in headers:
            with open(os.path.join(INCLUDE_DIR, fn)) as f:
                table.update(parse_prototypes(f.read()))
        _signatures = table
    return _signatures


def declared_symbols():
    """Every function name declared in include/*.h (used by the ABI test)."""
    return sorted(signatures())


def _bind(L):
    del unbound[:]
    for name, (restype, argtypes) in signatures().items():
        f = getattr(L, name, None)
        if f is None:
            unbound.append(name)
            continue
        f.restype = restype
        f.argtypes = argtypes
