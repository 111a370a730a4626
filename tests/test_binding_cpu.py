"""The ctypes binding is derived from include/smilfit.h (smilify_amd/_lib.py): the parser on small snippets, the derived layouts and
constants against a C compiler, its completeness against independent counts, and the checked accessor next to the raw library."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import pytest
from conftest import REPO

from smilify_amd import _lib

HEADER = os.path.join(REPO, "include", "smilfit.h")

SNIPPET = """
#ifndef SMIL_SNIPPET_H_
#define SMIL_SNIPPET_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SMIL_THREE 3
#define SMIL_MINUS (-1)   /* a comment; with ( and smil_x( in it */
typedef struct SmilModel SmilModel; /* opaque */
typedef struct {
    int32_t V, F;
    const float *a, *b; int32_t n;   /* two statements; one line */
    uint32_t *range;
    const void *src;
    int64_t count;
    float lr; double tol; uint64_t seed; size_t bytes; int flag; uint32_t bits;
} SmilThing; /* a comment after the brace
                over two lines; smil_y( */
int smil_make(const SmilThing *t, SmilModel **out);
size_t smil_bytes(const SmilModel *m, int32_t N, int64_t rows, uint64_t seed, float a, double b, size_t c, int d, uint32_t e);
void smil_free(SmilModel *m);
const char *smil_name(void);
int smil_many(const float rgb[3], int32_t dims[4], int32_t *const *out, const uint8_t *mask, const SmilThing *const *list,
              void *stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_declarator_form():
    constants, structs, protos = _lib.parse_header(SNIPPET)
    assert constants == {"THREE": 3, "MINUS": -1}  # the guard SMIL_SNIPPET_H_ has no value and is no constant
    assert list(structs) == ["Thing"]
    Thing = structs["Thing"]
    assert Thing._fields_ == [("V", c_int32), ("F", c_int32), ("a", c_void_p), ("b", c_void_p), ("n", c_int32), ("range", c_void_p),
                              ("src", c_void_p), ("count", c_int64), ("lr", c_float), ("tol", c_double), ("seed", c_uint64),
                              ("bytes", c_size_t), ("flag", c_int32), ("bits", c_uint32)]
    assert list(protos) == ["smil_make", "smil_bytes", "smil_free", "smil_name", "smil_many"]
    assert protos["smil_make"] == (c_int32, [POINTER(Thing), c_void_p])
    assert protos["smil_bytes"] == (c_size_t, [c_void_p, c_int32, c_int64, c_uint64, c_float, c_double, c_size_t, c_int32, c_uint32])
    assert protos["smil_free"] == (None, [c_void_p])
    assert protos["smil_name"] == (c_char_p, [])
    assert protos["smil_many"] == (c_int32, [c_void_p] * 6)


@pytest.mark.parametrize("bad, named", [
    ("int smil_f(int16_t x);", "int16_t x"),                                        # an unknown type name
    ("typedef struct { wchar_t *p; } SmilA;", "wchar_t *p"),
    ("int smil_f(SmilNobody *p);", "SmilNobody *p"),
    ("int smil_f(void (*cb)(int), void *stream);", "smil_f"),                       # a function pointer
    ("typedef struct { void (*cb)(int); } SmilA;", "(*cb)(int)"),
    ("typedef struct { int32_t a : 3; } SmilA;", "int32_t a : 3"),                  # a bit-field
    ("typedef struct { union { int32_t a; float b; } u; } SmilA;", "union"),        # a union
    ("typedef struct { struct { int32_t a; } in; } SmilA;", "typedef struct"),      # a nested struct
    ("typedef struct { int32_t a; } SmilA;\ntypedef struct { SmilA in; } SmilB;", "SmilA in"),
    ("typedef struct { int32_t a;\nint smil_f(void);", "typedef struct"),           # a struct that is never closed
    ("typedef struct { int32_t a[4]; } SmilA;", "int32_t a[4]"),                    # an array FIELD (a parameter form only)
    ("#define SMIL_HALF 0.5", "SMIL_HALF"),                                         # values that are no integers
    ("#define SMIL_SUM (SMIL_A + 1)", "SMIL_SUM"),
    ("#define SMIL_F(x) 3", "SMIL_F"),
    ("float smil_f(void);", "smil_f"),                                              # smil_...( outside a readable prototype
    ("int smil_f(void)\nint smil_g(void);", "smil_f"),
    ("static inline int smil_f(void) { return 0; }", "smil_f"),
    ("int smil_f(void);\nint smil_f(void);", "smil_f"),
    ("int smil_f(int32_t);", "int32_t"),
    ("int other(void);", "other"),
])
def test_parser_raises_and_names_what_it_cannot_read(bad, named):
    with pytest.raises(_lib.SmilError) as e:
        _lib.parse_header("int smil_before(void);\n" + bad + "\nint smil_after(void);\n")
    assert named in str(e.value), str(e.value)


def test_a_missing_header_raises(monkeypatch):
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(REPO, "include", "no_such.h"))
    with pytest.raises(_lib.SmilError, match="no_such.h not found"):
        _lib._read_header()


def test_nothing_in_the_header_is_skipped():
    """Independent counts of the header's text (as the name test of test_abi_cpu.py does for the prototypes)."""
    header = open(HEADER).read()
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+SMIL_(\w+)", header, re.M)
    assert len(defines) == len(set(defines)) and set(defines) == set(_lib.CONSTANTS), set(defines) ^ set(_lib.CONSTANTS)
    closed = re.findall(r"^\}\s*(Smil\w+)\s*;", header, re.M)
    assert len(closed) == header.count("typedef struct {") == len(_lib.STRUCTS)
    assert closed == ["Smil" + name for name in _lib.STRUCTS]
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == len(_lib.PROTOTYPES)
    for name, value in _lib.CONSTANTS.items():
        assert getattr(_lib, name) == value
    for name, struct in _lib.STRUCTS.items():
        assert getattr(_lib, name) is struct
    assert (_lib.OK, _lib.E_INVALID, _lib.E_UNSUPPORTED, _lib.TIE_REFERENCE_QUEUE, _lib.MAX_FACES_PER_PIXEL, _lib.EDT_NONE) == \
        (0, -1, -3, 1, 128, 2147483647)


def test_layouts_and_constants_against_the_c_compiler(tmp_path):
    """sizeof / offsetof of every struct and field and the value of every #define, as a C compiler sees smilfit.h."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "smilfit.h"', "int main(void) {"]
    for name, struct in _lib.STRUCTS.items():
        lines.append(f'printf("S {name} %zu\\n", sizeof(Smil{name}));')
        for field, _ in struct._fields_:
            lines.append(f'printf("F {name}.{field} %zu %zu\\n", offsetof(Smil{name}, {field}), sizeof(((Smil{name} *)0)->{field}));')
    for name in _lib.CONSTANTS:
        lines.append(f'printf("D {name} %lld\\n", (long long)(SMIL_{name}));')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    printed = [line.split(" ", 2) for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    seen = {f"{kind} {name}": value for kind, name, value in printed}
    assert len(seen) == len(lines) - 5
    for name, struct in _lib.STRUCTS.items():
        assert int(seen.pop(f"S {name}")) == ctypes.sizeof(struct), name
        for field, _ in struct._fields_:
            d = getattr(struct, field)
            assert seen.pop(f"F {name}.{field}") == f"{d.offset} {d.size}", (name, field)
    for name, value in _lib.CONSTANTS.items():
        assert int(seen.pop(f"D {name}")) == value, name
    assert not seen


def test_checked_raises_where_the_raw_library_returns_a_code():
    raw, checked = _lib.load(), _lib.checked()
    assert raw.smil_model_dims(None, None) == -1
    with pytest.raises(_lib.SmilError) as e:
        checked.smil_model_dims(None, None)
    assert str(e.value).startswith("smil_model_dims failed (code -1): ")
    assert str(e.value).endswith(raw.smil_last_error().decode()) and raw.smil_last_error()
    assert raw.smil_model_dims(None, None) == -1  # the raw function object is not the checked one
    assert raw.smil_raster_workspace_bytes(None, 1, 64) == 0 and checked.smil_raster_workspace_bytes(None, 1, 64) == 0
    assert raw.smil_version() == checked.smil_version()
    for name in _lib.EXPORTS:
        r, c = getattr(raw, name), getattr(checked, name)
        assert r is not c and (r.restype, r.argtypes) == (c.restype, c.argtypes) == _lib.PROTOTYPES[name]
        assert r.errcheck is None and (c.errcheck is not None) == (c.restype is c_int32), name
