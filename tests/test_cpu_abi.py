"""The binding is a function of include/hig.h (hig_amd/_abi.py reads it, hig_amd/_lib.py is built from the reading).  CPU only:
the reader on literal snippets, its refusals, and the host compiler as the oracle for what the reader made of the real header --
struct layouts, constants and the class of every parameter and return type."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hig_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hig.h")


def test_reader_on_literal_declarations():
    consts, structs, callbacks, protos = _abi.parse_header("""
        #ifndef HIG_H
        #define HIG_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define HIG_OK 0
        #define HIG_X (-3)   /* parenthesised, negative */
        #define HIG_D32_COUNT(L) (HIG_D32_NLAYER * (L) + 1)
        enum { HIG_A = 4, HIG_B, /* implicit */ HIG_C = -2, HIG_D, HIG_E };
        enum {
          HIG_F = 0, HIG_G, // two on a line
          HIG_H2
        };
        typedef void* hig_stream_t; /* hipStream_t */
        typedef struct hig_pt {
          int32_t B, N;          /* two fields, one declaration */
          const float* X; int64_t ldx;
          void* Y;
        } hig_pt;
        typedef void (*hig_layer_hook)(void* user, int32_t layer);
        int hig_version(void);
        int64_t hig_bytes(const hig_pt* p, int training);
        int hig_three_lines(const hig_pt* p, const void* const* params,
                            float* loss /* device scalar, (nullable); */, int64_t* pred,
                            float scale, hig_stream_t stream, hig_layer_hook hook, char* buf);
        void hig_nothing(int32_t);
        typedef int (*hig_progress)(void*, int64_t done);   /* a callback with an unnamed parameter */
        int hig_mixed(const float*, int64_t n, hig_progress, const int64_t* const*);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert consts == {"HIG_OK": 0, "HIG_X": -3, "HIG_A": 4, "HIG_B": 5, "HIG_C": -2, "HIG_D": -1, "HIG_E": 0, "HIG_F": 0, "HIG_G": 1,
                      "HIG_H2": 2}
    assert structs == {"hig_pt": [("B", "int32_t"), ("N", "int32_t"), ("X", "const float*"), ("ldx", "int64_t"), ("Y", "void*")]}
    def types(decl):                                     # (return C type, [parameter C types]); the names are held to below
        return decl[0], [t for _, t in decl[1]]

    def names(decl):
        return [n for n, _ in decl[1]]

    assert {n: types(d) for n, d in callbacks.items()} == {"hig_layer_hook": ("void", ["void*", "int32_t"]),
                                                           "hig_progress": ("int", ["void*", "int64_t"])}
    assert list(protos) == ["hig_version", "hig_bytes", "hig_three_lines", "hig_nothing", "hig_mixed"]  # the header's order
    assert types(protos["hig_version"]) == ("int", []) and types(protos["hig_bytes"]) == ("int64_t", ["const hig_pt*", "int"])
    assert types(protos["hig_three_lines"]) == ("int", ["const hig_pt*", "const void* const*", "float*", "int64_t*", "float", "hig_stream_t",
                                                        "hig_layer_hook", "char*"])
    assert types(protos["hig_nothing"]) == ("void", ["int32_t"])
    assert types(protos["hig_mixed"]) == ("int", ["const float*", "int64_t", "hig_progress", "const int64_t* const*"])
    # the names: the header's own, `arg<i>` by position where it gives none
    assert names(callbacks["hig_layer_hook"]) == ["user", "layer"] and names(callbacks["hig_progress"]) == ["arg0", "done"]
    assert names(protos["hig_version"]) == [] and names(protos["hig_bytes"]) == ["p", "training"]
    assert names(protos["hig_three_lines"]) == ["p", "params", "loss", "pred", "scale", "stream", "hook", "buf"]
    assert names(protos["hig_nothing"]) == ["arg0"] and names(protos["hig_mixed"]) == ["arg0", "n", "arg2", "arg3"]

    classes, hooks, sigs = _abi.bind(structs, callbacks, protos, {"hig_pt": "Pt"})
    Pt, hook = classes["Pt"], hooks["hig_layer_hook"]
    assert Pt.__name__ == "Pt" and Pt._fields_ == [("B", C.c_int32), ("N", C.c_int32), ("X", C.c_void_p), ("ldx", C.c_int64), ("Y", C.c_void_p)]
    assert Pt(B=3, ldx=1 << 40).ldx == 1 << 40
    assert (hook._restype_, hook._argtypes_) == (None, (C.c_void_p, C.c_int32))
    assert (hooks["hig_progress"]._restype_, hooks["hig_progress"]._argtypes_) == (C.c_int32, (C.c_void_p, C.c_int64))
    assert sigs["hig_mixed"] == (C.c_int32, [C.c_void_p, C.c_int64, hooks["hig_progress"], C.c_void_p])
    assert sigs["hig_version"] == (C.c_int32, []) and sigs["hig_nothing"] == (None, [C.c_int32])
    assert sigs["hig_bytes"] == (C.c_int64, [C.POINTER(Pt), C.c_int32])
    assert sigs["hig_three_lines"] == (C.c_int32, [C.POINTER(Pt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, hook, C.c_char_p])
    # what the callers of the plan functions pass for an `int32_t*` host out-parameter
    assert C.c_void_p.from_param(C.byref(C.c_int32())) is not None and C.c_void_p.from_param((C.c_int32 * 4)()) is not None


PT = "typedef struct hig_pt { int32_t B; } hig_pt;\n"


@pytest.mark.parametrize("text, named", [
    ("int hig_takes_double(double x);", "hig_takes_double"),                       # unknown by-value types
    ("int hig_takes_size(size_t n);", "hig_takes_size"),
    ("double hig_returns_double(void);", "hig_returns_double"),
    ("typedef struct hig_pt { uint8_t flag; } hig_pt;", "hig_pt.flag"),
    ("typedef void (*hig_layer_hook)(void* user, long layer);", "hig_layer_hook"),
    (PT + "int hig_by_value(hig_pt p);", "hig_by_value"),                          # a struct by value
    (PT + "hig_pt hig_returns_struct(void);", "hig_returns_struct"),
    ("int hig_variadic(const char* fmt, ...);", "hig_variadic"),
    ("int hig_takes_void(void x, int y);", "hig_takes_void"),
    ("#define HIG_SCALE 0.5f", "HIG_SCALE"),                                       # #define HIG_* that is no integer
    ("#define HIG_TWICE(x) (2 * (x))", "HIG_TWICE"),
    ("#define HIG_ALIAS HIG_OK", "HIG_ALIAS"),
    ("enum { HIG_M = 1 << 3 };", "HIG_M"),
    ("#define HIG_OK 0\nenum { HIG_OK };", "HIG_OK"),                              # one name, two definitions
    ("int hig_twice(void);\nint hig_twice(void);", "hig_twice"),
    ("typedef struct hig_unnamed { int32_t B; } hig_unnamed;", "hig_unnamed"),     # a struct without a Python name
    ("typedef struct hig_arr { int32_t B[4]; } hig_arr;", "hig_arr"),              # field forms outside the subset
    ("typedef struct hig_bits { int32_t B : 3; } hig_bits;", "hig_bits"),
    ("typedef int32_t hig_index_t;", "hig_index_t"),                               # declarations outside the subset
    ("static inline int hig_inline(void) { return 0; }", "hig_inline"),
])
def test_reader_refuses_what_it_does_not_understand_by_name(text, named):
    with pytest.raises(_abi.HeaderError, match=re.escape(named)):
        _abi.bind(*_abi.parse_header(text)[1:], {"hig_pt": "Pt"})


def test_binding_follows_the_header():
    """_lib holds the reading of include/hig.h and nothing of its own: the symbols, the five Structures, every constant."""
    consts, structs, callbacks, protos = _abi.parse_header(open(HEADER).read())
    assert len(protos) >= 130 and _lib.SYMBOLS == tuple(protos) == tuple(_lib.SIGNATURES)
    assert set(structs) == set(_lib.STRUCT_NAMES) and list(callbacks) == ["hig_layer_hook"]
    for cname, pyname in _lib.STRUCT_NAMES.items():
        assert [f for f, _ in getattr(_lib, pyname)._fields_] == [f for f, _ in structs[cname]]
    assert all(getattr(_lib, n[len("HIG_"):]) == v for n, v in consts.items())
    assert (_lib.T_NGLOBAL, _lib.T_NLAYER, _lib.EV_NGLOBAL) == (consts["HIG_T_NGLOBAL"], consts["HIG_TL_NLAYER"], consts["HIG_EV_NGLOBAL"])
    assert len(_lib.DN_SWITCHES) == len(_lib.DN_SWITCH_DEFAULTS) == _lib.DN_NSWITCHES and len(_lib.DN_PLAN_SLOTS) == _lib.DN_PLAN_NSLOTS
    assert [s.lower() for s in _lib.DN_PLAN_SLOTS] == [n[len("HIG_DN_PLAN_"):].lower() for n in consts if n.startswith("HIG_DN_PLAN_")][:-1]
    lib = _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():                    # one loop set them all, hig_version included
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.hig_version.argtypes == [] and lib.hig_workspace_bytes.restype is C.c_int64


def test_library_older_than_the_header_and_missing_header_are_refused(monkeypatch, tmp_path):
    import _ctypes
    import importlib
    import shutil
    import sys
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", _ctypes.__file__)                       # a shared library with no hig_* symbol
    with pytest.raises(RuntimeError, match=r"libhig\.so is older than include/hig\.h: rebuild"):
        _lib.lib()
    pkg = tmp_path / "hig_copy"                                                   # the package without an include/ next to it
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    for f in ("_abi.py", "_lib.py"):
        shutil.copy(os.path.join(os.path.dirname(_lib.__file__), f), pkg / f)
    monkeypatch.syspath_prepend(str(tmp_path))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "include" / "hig.h"))):
        importlib.import_module("hig_copy._lib")
    for m in [m for m in sys.modules if m.startswith("hig_copy")]:
        del sys.modules[m]


# ---- the compiler as the oracle ----------------------------------------------------------------------------------------------

_PROBE = r"""
#include "hig.h"
#include <cstddef>
#include <cstdio>
#include <type_traits>
template <class T> constexpr char kind() {
  return std::is_void_v<T> ? 'v' : std::is_pointer_v<T> ? 'p' : std::is_floating_point_v<T> ? 'f' : std::is_integral_v<T> ? 'i' : '?';
}
template <class T> constexpr int size() { if constexpr (std::is_void_v<T>) return 0; else return int(sizeof(T)); }
template <class F> struct Proto;
template <class R, class... A> struct Proto<R (*)(A...)> {
  static void print(const char* name) {
    std::printf("proto %s %d %c%d", name, int(sizeof...(A)), kind<R>(), size<R>());
    ((std::printf(" %c%d", kind<A>(), size<A>())), ...);
    std::printf("\n");
  }
};
#define FIELD(S, F) std::printf("field " #S "." #F " %d %d\n", int(offsetof(S, F)), int(sizeof(((S*)0)->F)))
int main() {
@BODY@  return 0;
}
"""


def _compiler():
    makefile = open(os.path.join(ROOT, "human-interaction-generation_amd", "csrc", "Makefile")).read()
    return os.environ.get("CLANGXX") or re.search(r"^CLANGXX\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)


def compiler_lines(include_dir, parsed, tag):
    """What the host compiler makes of <include_dir>/hig.h, one line per struct, field, constant and prototype `parsed` names."""
    consts, structs, _, protos = parsed
    body = []
    for s, fields in structs.items():
        body.append('  std::printf("struct %s %%d\\n", int(sizeof(%s)));\n' % (s, s))
        body += ["  FIELD(%s, %s);\n" % (s, f) for f, _ in fields]
    body += ['  std::printf("const %s %%lld\\n", (long long)(%s));\n' % (n, n) for n in consts]
    body += ['  Proto<decltype(&%s)>::print("%s");\n' % (n, n) for n in protos]
    out = os.path.join(ROOT, "build", "abi_probe")
    os.makedirs(out, exist_ok=True)
    src, exe = os.path.join(out, tag + ".cpp"), os.path.join(out, tag)
    with open(src, "w") as f:
        f.write(_PROBE.replace("@BODY@", "".join(body)))
    b = subprocess.run([_compiler(), "-std=c++17", "-O0", "-I", include_dir, src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def _ctype_class(t):
    if t is None:
        return "v0"
    pointer = issubclass(t, (C._Pointer, C._CFuncPtr, C.c_void_p, C.c_char_p))
    return ("p" if pointer else "f" if issubclass(t, (C.c_float, C.c_double)) else "i") + str(C.sizeof(t))


def ctypes_lines(parsed, classes, signatures, constant):
    """The same lines from the ctypes side: Structure sizes and field offsets, the exported constants, every restype / argtypes."""
    consts, structs, _, protos = parsed
    lines = []
    for s, fields in structs.items():
        cls = classes[s]
        lines.append("struct %s %d" % (s, C.sizeof(cls)))
        lines += ["field %s.%s %d %d" % (s, f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in fields]
    lines += ["const %s %d" % (n, constant(n)) for n in consts]
    for n in protos:
        restype, argtypes = signatures[n]
        lines.append(" ".join(["proto", n, str(len(argtypes)), _ctype_class(restype)] + [_ctype_class(a) for a in argtypes]))
    return lines


@pytest.fixture(scope="module")
def parsed():
    return _abi.parse_header(open(HEADER).read())


def test_compiler_agrees_with_the_binding_on_layouts_constants_and_signatures(parsed):
    """sizeof / offsetof of the five structs, the value of every constant, and arity plus (kind, size) of the return type and of
    every parameter of every prototype, as the host compiler sees include/hig.h, against ctypes.sizeof, Structure.field.offset,
    _lib's constants and the classes lib() hands to ctypes.  Line for line: a swapped i32 / i64, a lost `restype = c_int64`, a
    field out of order or a misread constant shows as the line that differs."""
    lib = _lib.lib()
    loaded = {n: (getattr(lib, n).restype, list(getattr(lib, n).argtypes)) for n in parsed[3]}
    classes = {c: getattr(_lib, py) for c, py in _lib.STRUCT_NAMES.items()}
    ours = ctypes_lines(parsed, classes, loaded, lambda n: getattr(_lib, n[len("HIG_"):]))
    theirs = compiler_lines(os.path.join(ROOT, "include"), parsed, "hig")
    assert len(theirs) == 5 + sum(len(f) for f in parsed[1].values()) + len(parsed[0]) + len(parsed[3]) and len(parsed[3]) >= 130
    assert "?" not in "".join(theirs)
    differ = [(a, b) for a, b in zip(ours, theirs) if a != b]
    assert not differ and len(ours) == len(theirs), "binding vs compiler: %s" % differ[:10]


def test_compiler_oracle_sees_one_narrowed_integer(parsed, tmp_path):
    """The oracle is sensitive: a copy of the header in which ONE int64_t parameter became int32_t compiles to a report that differs
    from the binding in exactly that prototype's line."""
    text = open(HEADER).read()
    before = "int hig_cast_bf16(const float* src, void* dst, int64_t n, hig_stream_t stream);"
    assert text.count(before) == 1
    (tmp_path / "hig.h").write_text(text.replace(before, before.replace("int64_t n", "int32_t n")))
    classes = {c: getattr(_lib, py) for c, py in _lib.STRUCT_NAMES.items()}
    ours = ctypes_lines(parsed, classes, _lib.SIGNATURES, lambda n: getattr(_lib, n[len("HIG_"):]))
    theirs = compiler_lines(str(tmp_path), parsed, "hig_narrowed")
    assert [(a, b) for a, b in zip(ours, theirs) if a != b] == [("proto hig_cast_bf16 4 i4 p8 p8 i8 p8", "proto hig_cast_bf16 4 i4 p8 p8 i4 p8")]
