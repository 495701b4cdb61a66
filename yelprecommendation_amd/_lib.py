"""ctypes binding of the C-ABI engine, read from its header (include/yelprec_engine.h).

The header is the one written record of the ABI: it is parsed once at import into ``SIGNATURES`` (argument types),
``RESTYPES`` (return types other than ``int``) and ``DEFINES`` (the integer ``#define YR_*`` values), so a declaration
or constant added there needs no second entry here.

The library is built in-tree by ``__graft_entry__.build()`` (or
``make -C yelprecommendation_amd/csrc``) as
``yelprecommendation_amd/libyelprec_engine.so``.  There is NO fallback: if the
header or the library is missing or an entry point is absent, loading raises, and every op in
:mod:`yelprecommendation_amd.engine` raises with it.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# YR_ENGINE_LIB: measurement hook — an instrumented build of the same sources (scratch/inst_build.sh writes it to
# a temp directory so that the product objects and library are never overwritten); unset in every product run.
LIB_PATH = os.environ.get("YR_ENGINE_LIB") or os.path.join(_HERE, "libyelprec_engine.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "yelprec_engine.h")


class EngineError(RuntimeError):
    pass


# the scalar types of the ABI; every argument with a `*` is a pointer
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_RETURNS = dict(_SCALARS, **{"const char *": C.c_char_p})


def _argtype(arg, decl):
    if "*" in arg:
        return C.c_void_p
    words = [w for w in arg.split() if w != "const"]
    if len(words) == 2 and words[1].isidentifier():         # "type name"
        words.pop()
    if len(words) != 1 or words[0] not in _SCALARS:
        raise EngineError(f"{decl}: no ctypes mapping for the argument {' '.join(arg.split())!r}")
    return _SCALARS[words[0]]


def parse_header(text):
    """(signatures, restypes, defines) of a header in the style of include/yelprec_engine.h, where every ``yr_*``
    declaration starts a line with its return type: name -> argtypes, name -> restype where it is not ``int``, and
    the integer ``#define YR_*`` values (plain or parenthesised).  Comments of both kinds are dropped first; a type
    that is neither a pointer nor one of the known scalars raises EngineError naming the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    define = r"^[ \t]*#[ \t]*define[ \t]+(YR_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$"
    defines = {name: int(value) for name, value in re.findall(define, text, flags=re.M)}
    declaration = r"^[ \t]*(\w[\w \t]*?[\s*]+)(yr_\w+)\s*\(([^()]*)\)\s*;"     # return type, name, argument list
    signatures, restypes = {}, {}
    for ret, name, args in re.findall(declaration, text, flags=re.M):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise EngineError(f"{name}: no ctypes mapping for the return type {ret!r}")
        if _RETURNS[ret] is not C.c_int:
            restypes[name] = _RETURNS[ret]
        signatures[name] = [] if args.strip() in ("", "void") else [_argtype(a, name) for a in args.split(",")]
    unparsed = set(re.findall(r"\b(yr_\w+)\s*\(", text)) - set(signatures)
    if unparsed:
        raise EngineError(f"cannot parse the declaration of {sorted(unparsed)}")
    return signatures, restypes, defines


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise EngineError(f"engine header not found at {HEADER_PATH}: {e}. The binding is read from it; there is no "
                          "fallback table.") from e


SIGNATURES, RESTYPES, DEFINES = _read_header()
ENGINE_VERSION = DEFINES["YR_ENGINE_VERSION"]

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises EngineError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64 (same SONAME as /opt/rocm's).  It must be the first HIP
    # runtime mapped into the process so that this library and torch share ONE runtime (and
    # one set of streams / device pointers); loading ours first leaves torch with no device.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            f"HIP engine library not found at {LIB_PATH}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C yelprecommendation_amd/csrc`. There is no CPU/PyTorch fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime etc.
        raise EngineError(f"cannot load {LIB_PATH}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise EngineError(f"{LIB_PATH} does not export {name}") from e
        fn.argtypes = argtypes
        fn.restype = RESTYPES.get(name, C.c_int)
    v = lib.yr_engine_version()
    if v != ENGINE_VERSION:
        raise EngineError(f"engine ABI version {v} != expected {ENGINE_VERSION}; rebuild the library")
    _lib = lib
    return lib


def check(status: int, what: str):
    if status == 0:
        return
    if status == DEFINES["YR_ERR_UNSUPPORTED"]:
        raise EngineError(f"{what}: unsupported configuration (embedding width must be 16/32/64/128, or 256/512/1024 on the BPR-MF push, evaluation and score paths; top-k above 16 needs a width up to 64)")
    if status == DEFINES["YR_ERR_BADARG"]:
        raise EngineError(f"{what}: bad argument (null pointer, negative size or misaligned buffer)")
    raise EngineError(f"{what}: HIP error {status}")


def query_size(name: str, *args) -> int:
    """A size the engine answers on the host (``*_workspace_bytes`` and the like): the non-negative count, or
    EngineError for the negative YR_ERR_* of a refused shape."""
    n = int(getattr(load(), name)(*(int(a) for a in args)))
    if n < 0:
        check(n, name)
    return n
