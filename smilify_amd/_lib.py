"""ctypes binding of ``libsmilfit.so``, derived from its specification include/smilfit.h.

The header is read when this module is imported: every ``typedef struct { ... } SmilName;`` becomes the ctypes Structure ``Name``,
every ``#define SMIL_X <integer>`` the constant ``X``, every prototype the ``restype`` / ``argtypes`` of its function, and ``EXPORTS``
lists the prototypes' names.  Nothing about the ABI is written down a second time here.  A declaration the parser cannot read raises
``SmilError`` naming it; none is ever skipped.

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C smilify_amd/csrc``.  There is NO fallback: if the shared
object or the header is missing, or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
import re
import types
from ctypes import POINTER, c_char_p, c_int32, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMILFIT_LIB: load another build of the same library (instrumented builds under tools/dbg); never a CPU path
LIB_PATH = os.environ.get("SMILFIT_LIB") or os.path.join(_HERE, "lib", "libsmilfit.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "smilfit.h")


class SmilError(RuntimeError):
    pass


_SCALARS = {"int32_t": c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": c_size_t, "int": c_int32}
_POINTEES = {"void", "char", "uint8_t"}  # known, but only behind a pointer
_RESTYPES = {"int": c_int32, "size_t": c_size_t, "void": None, "const char *": c_char_p}
_INTEGER = re.compile(r"\(\s*(-?(?:0|[1-9]\d*))\s*\)|(-?(?:0|[1-9]\d*))")  # decimal, optionally in parentheses
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+SMIL_(\w+)(.*)$", re.M)
_BASE = re.compile(r"(?:const\s+)?(\w+)\s*(.*)", re.S)  # [const] T <declarators>
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\s+)?)*)(\w+)\s*(\[\s*\d+\s*\])?")  # *x, **x, *const *x, x[4]
_STATEMENT = re.compile(r"""\s*(?:
      typedef\s+struct\s+(?P<opaque>\w+)\s+(?P=opaque)\s*;
    | typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
    | (?P<ret>const\s+char\s*\*|\w+)\s*(?P<fn>smil_\w+)\s*\((?P<params>[^()]*)\)\s*;
    | extern\s+"C"\s*\{ | \}(?=\s*$) )""", re.X)


def _declarations(statement: str, structs: dict, known: set, field: bool):
    """``[const] T a, *b, c[4]`` -> [(name, ctype)].  Fields: every pointer is c_void_p and an array is refused (none is used);
    parameters: an array is the pointer C makes of it, and one level of pointer to a struct of this header is POINTER(Struct)."""
    statement = " ".join(statement.split())
    bad = SmilError(f"smilfit.h: cannot read the declaration '{statement}' (unknown type, function pointer, bit-field, nested struct, "
                    "array field or value of a non-scalar type?)")
    m = _BASE.fullmatch(statement)
    if not m or not (m.group(1) in _SCALARS or m.group(1) in known):
        raise bad
    base, out = m.group(1), []
    for declarator in m.group(2).split(","):
        d = _DECLARATOR.fullmatch(declarator.strip())
        if not d or (field and d.group(3)):
            raise bad
        levels = d.group(1).count("*") + bool(d.group(3))
        if levels == 0 and base not in _SCALARS:
            raise bad
        out.append((d.group(2), _SCALARS[base] if levels == 0 else
                    POINTER(structs[base]) if levels == 1 and base in structs and not field else c_void_p))
    return out


def parse_header(text: str):
    """-> (constants {X: int}, structs {Name: Structure}, prototypes {smil_x: (restype, argtypes)}), each in the header's order."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants, structs, c_structs, prototypes, known = {}, {}, {}, {}, set(_POINTEES)
    for name, value in _DEFINE.findall(text):
        m = _INTEGER.fullmatch(value.strip())
        if m:
            constants[name] = int(m.group(1) or m.group(2))
        elif value.strip():  # a define without a value is a header guard
            raise SmilError(f"smilfit.h: the value of SMIL_{name} is not an integer: '{value.strip()}'")
    text, pos = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).rstrip(), 0
    while pos < len(text):
        m = _STATEMENT.match(text, pos)
        if not m:
            raise SmilError(f"smilfit.h: cannot read the declaration that starts '{' '.join(text[pos:pos + 160].split())}'")
        pos = m.end()
        if m.group("opaque"):
            known.add(m.group("opaque"))
        elif m.group("struct"):
            c_name = m.group("struct")
            if not c_name.startswith("Smil") or c_name in known:
                raise SmilError(f"smilfit.h: struct '{c_name}' is not a new Smil* name")
            fields = [f for s in m.group("body").split(";") if s.strip() for f in _declarations(s, c_structs, known, field=True)]
            c_structs[c_name] = structs[c_name[4:]] = type(c_name[4:], (ctypes.Structure,), {"_fields_": fields})
            known.add(c_name)
        elif m.group("fn"):
            ret = " ".join(m.group("ret").replace("*", " * ").split())
            if ret not in _RESTYPES or m.group("fn") in prototypes:
                raise SmilError(f"smilfit.h: cannot read the prototype '{' '.join(m.group(0).split())}'")
            params = [] if m.group("params").strip() in ("", "void") else m.group("params").split(",")
            prototypes[m.group("fn")] = (_RESTYPES[ret], [_declarations(p, c_structs, known, field=False)[0][1] for p in params])
    return constants, structs, prototypes


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise SmilError(f"{HEADER_PATH} not found: the binding of libsmilfit.so is derived from it")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


CONSTANTS, STRUCTS, PROTOTYPES = _read_header()
EXPORTS = list(PROTOTYPES)
globals().update(CONSTANTS)  # KNN_MAX_K, E_UNSUPPORTED, TRI_RANSAC, ...
globals().update(STRUCTS)    # ModelDesc, LbsInputs, Cameras, ...

_lib = None
_checked = None


def _bind(fn, name, errcheck=None):
    fn.restype, fn.argtypes = PROTOTYPES[name]
    if errcheck is not None and fn.restype is c_int32:
        fn.errcheck = errcheck
    return fn


def load():
    """Load the shared library once; raise loudly when it has not been built.  Status codes come back as plain integers."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SmilError(
            f"{LIB_PATH} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C smilify_amd/csrc). There is no CPU fallback.")
    import torch  # noqa: F401  the library must bind to the HIP runtime torch has loaded, not bring up a second one
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        _bind(getattr(lib, name), name)  # raises AttributeError if the symbol is missing
    _lib = lib
    return lib


def check(rc: int, what: str = "libsmilfit call") -> None:
    if rc != 0:
        msg = load().smil_last_error()
        raise SmilError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def _errcheck(rc, fn, args):
    if rc != 0:
        check(rc, fn.__name__)
    return rc


def checked():
    """The same entry points, but every ``int``-returning one raises SmilError on a non-zero status (``check`` under the function's own
    name): ctypes hands each status to ``_errcheck``, so no wrapper function stands around a call.  ``lib[name]`` is a function object of
    its own, so ``load()`` keeps returning plain status codes.  size_t, void and char * functions behave as on ``load()``."""
    global _checked
    if _checked is None:
        lib = load()
        _checked = types.SimpleNamespace(**{name: _bind(lib[name], name, _errcheck) for name in EXPORTS})
    return _checked
