"""ctypes binding of libkoaf.so (the C ABI declared in include/koaf.h).

Struct layouts, prototypes and constants are all parsed from the header itself, so the Python side cannot drift from the C
side, and `lib()` refuses a library whose koaf_version() is not the header's KOAF_VERSION: a stale build read through newer
descriptors would shift arguments and write through wild device pointers.
There is no CPU fallback: if the library is missing, `lib()` raises -- the product path must fail
loudly rather than silently run something else.
"""
import ctypes
import functools
import os
import re
from pathlib import Path

_ROOT = Path(__file__).resolve().parent
HEADER = _ROOT.parent / "include" / "koaf.h"
LIB_PATH = _ROOT / "csrc" / "libkoaf.so"


class KoafError(RuntimeError):
    pass


_SCALARS = {
    "char": ctypes.c_char,
    "int": ctypes.c_int,
    "int32_t": ctypes.c_int32,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "uint32_t": ctypes.c_uint32,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
}


@functools.lru_cache(maxsize=None)
def _text(path):
    """the header without its comments (read once per process)"""
    return re.sub(r"/\*.*?\*/", " ", Path(path).read_text(), flags=re.S)


_TYPEDEF = r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;"


def _parse_structs(text):
    """-> {name: ctypes.Structure subclass} for every `typedef struct NAME { ... } NAME;`, in declaration order"""
    structs = {}
    for m in re.finditer(_TYPEDEF, text):
        name, fields = m.group(1), []
        if name != m.group(3):
            raise KoafError(f"koaf.h: typedef struct {name} is named {m.group(3)}")
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            base, rest = re.match(r"\s*(\w*)(.*)", re.sub(r"\bconst\b", " ", decl), flags=re.S).groups()
            for d in rest.split(","):               # `int32_t H, W, C;`  `const float* ptr;`  `char variant[24];`
                dm = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", d)
                if dm is None or not (dm.group(1) or base in structs or base in _SCALARS):
                    raise KoafError(f"koaf.h: cannot read field `{decl}` of {name}")
                t = ctypes.c_void_p if dm.group(1) else structs.get(base) or _SCALARS[base]
                fields.append((dm.group(2), t * int(dm.group(3)) if dm.group(3) else t))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    if len(structs) != len(re.findall(r"\btypedef\b", text)):
        raise KoafError(f"koaf.h: only {sorted(structs)} of its typedefs could be read")
    return structs


STRUCTS = _parse_structs(_text(HEADER))
KoafOperand = STRUCTS["KoafOperand"]
KoafGemm = STRUCTS["KoafGemm"]
KoafLaunchRec = STRUCTS["KoafLaunchRec"]
KoafWPlane = STRUCTS["KoafWPlane"]
KoafWImg = STRUCTS["KoafWImg"]
KoafBnApply = STRUCTS["KoafBnApply"]
KoafTail = STRUCTS["KoafTail"]
KoafEmit = STRUCTS["KoafEmit"]
KoafBnb = STRUCTS["KoafBnb"]


def _ctype(decl: str):
    toks = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
    if "*" in toks:
        if toks[0] in STRUCTS:
            return ctypes.POINTER(STRUCTS[toks[0]])
        return ctypes.c_char_p if toks[0] == "char" else ctypes.c_void_p
    return _SCALARS[toks[0]]


def defines(path=None):
    """-> {name: int | float} for every numeric `#define KOAF_...` of koaf.h (KOAF_OK, KOAF_VERSION, KOAF_ACT_SCALE, ...)"""
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(KOAF_\w+)[ \t]+\(?(-?\d+(\.\d*f?)?)\)?[ \t]*$", _text(path or HEADER), flags=re.M)
    return {name: float(val.rstrip("f")) if frac else int(val) for name, val, frac in found}


def parse_header(path=None):
    """-> {name: (restype, [argtypes])} for every function prototype in koaf.h"""
    text = re.sub(_TYPEDEF, " ", _text(path or HEADER))
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)          # preprocessor lines
    protos = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(koaf_\w+)\s*\(([^)]*)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if args in ("void", ""):
            argtypes = []
        else:
            argtypes = []
            for a in args.split(","):
                a = a.strip()
                # drop the parameter name (last identifier) unless it is part of the type
                mm = re.match(r"(.*?)(\w+)$", a)
                argtypes.append(_ctype(mm.group(1) if mm.group(1).strip() else a))
        protos[name] = (_ctype(ret) if ret != "void" else None, argtypes)
    return protos


_LIB = None


def lib():
    """Load libkoaf.so (once).  Raises if the HIP extension has not been built, or was built from another koaf.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = Path(os.environ.get("KOAF_LIB", LIB_PATH))
    if not path.exists():
        raise KoafError(
            f"libkoaf.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C oaprogressionmmf_amd/csrc` -- there is no CPU fallback")
    handle = ctypes.CDLL(str(path))
    # koaf_version(void) is the one signature that can never move: ask it before any other prototype is trusted
    handle.koaf_version.restype, handle.koaf_version.argtypes = ctypes.c_int, []
    want, got = defines()["KOAF_VERSION"], handle.koaf_version()
    if got != want:
        raise KoafError(
            f"{path} is ABI version {got}, {HEADER} declares {want}: the descriptors would not line up -- rebuild the "
            f"library with `make -C oaprogressionmmf_amd/csrc`")
    for name, (restype, argtypes) in parse_header().items():
        fn = getattr(handle, name)  # AttributeError if a declared symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    _LIB = handle
    return _LIB


def check(rc, what=""):
    if rc != 0:
        msg = lib().koaf_last_error()
        raise KoafError(f"{what}: rc={rc}: {msg.decode() if msg else '?'}")
