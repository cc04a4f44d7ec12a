"""The ctypes binding is derived from include/act3d_hip.h (lib.read_header).  These tests hold the derived table to the host C++
compiler's own reading of the header -- kind, signedness and size of every return type and parameter, size and field offsets of
every parameter block -- and the reader to its rules on synthetic text: what it must accept, and what it must refuse by name
instead of guessing.  A wrong entry would raise nothing in Python; it would shift or truncate an argument of a kernel launch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "act3d_hip.h")
BLOCKS = {"a3d_dn_head_params": "DnHeadParams", "a3d_dn_cross_params": "DnCrossParams", "a3d_dn_rest_params": "DnRestParams",
          "a3d_dn_layer_params": "DnLayerParams", "a3d_dn_tail_params": "DnTailParams", "a3d_qs_params": "QsParams",
          "a3d_qs_grads": "QsGrads", "A3dGradReduceRec": "GradReduceRec"}

# prints one line per prototype ("F name ret arg arg ..") and per struct ("S name size field:offset:type ..") with every type as
# kind + sizeof: p pointer, f floating point, i / u signed / unsigned integer, v void, ? anything else (a struct by value).
# decltype(&f) is unevaluated, so the program references no symbol of the library.
PROLOGUE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "act3d_hip.h"
template <class T> struct K {
  static void p() {
    std::printf(" %s%zu", std::is_floating_point<T>::value ? "f" : !std::is_integral<T>::value ? "?" : std::is_signed<T>::value ? "i" : "u",
                sizeof(T));
  }
};
template <class T> struct K<T*> { static void p() { std::printf(" p%zu", sizeof(T*)); } };
template <> struct K<void> { static void p() { std::printf(" v0"); } };
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
  static void p(const char* name) { std::printf("F %s", name); K<R>::p(); (K<A>::p(), ...); std::printf("\n"); }
};
#define FIELD(S, f) std::printf(" %s:%zu:", #f, offsetof(S, f)); K<decltype(S::f)>::p();
int main() {
"""


def _kind(t):
    """The compiler program's spelling of a ctypes type."""
    if t is None:
        return "v0"
    if issubclass(t, ctypes.Structure):
        return "?%d" % ctypes.sizeof(t)
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return "p%d" % ctypes.sizeof(t)
    if t in (ctypes.c_float, ctypes.c_double):
        return "f%d" % ctypes.sizeof(t)
    return ("i" if t(-1).value < 0 else "u") + str(ctypes.sizeof(t))


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{"F": {name: [ret, args..]}, "S": {name: (size, [(field, offset, type)..])}} as the host C++ compiler reads the header."""
    cxx = next((c for c in (shutil.which("g++"), shutil.which("c++"), shutil.which("clang++")) if c), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    L = load_pkg().lib
    body = ['  Sig<decltype(&%s)>::p("%s");' % (n, n) for n in L.SIGNATURES]
    for cname, pyname in BLOCKS.items():
        body.append('  std::printf("S %s %%zu", sizeof(%s));' % (cname, cname))
        body += ["  FIELD(%s, %s)" % (cname, f[0]) for f in getattr(L, pyname)._fields_]
        body.append('  std::printf("\\n");')
    d = tmp_path_factory.mktemp("abi")
    src, exe = str(d / "abi_probe.cpp"), str(d / "abi_probe")
    with open(src, "w") as f:
        f.write(PROLOGUE + "\n".join(body) + "\n  return 0;\n}\n")
    r = subprocess.run([cxx, "-std=c++17", "-O0", "-Wno-invalid-offsetof", "-I", os.path.dirname(HEADER), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    res = {"F": {}, "S": {}}
    for line in out.splitlines():
        tag, name, *rest = line.split()
        if tag == "F":
            res["F"][name] = rest
        else:
            fields = [rest[i].split(":")[:2] + [rest[i + 1]] for i in range(1, len(rest), 2)]
            res["S"][name] = (int(rest[0]), [(f, int(off), t) for f, off, t in fields])
    return res


def test_signatures_equal_the_compilers_reading_of_the_header(compiled):
    L = load_pkg().lib
    assert len(L.SIGNATURES) >= 80 and set(compiled["F"]) == set(L.SIGNATURES)
    for name, (res, args) in L.SIGNATURES.items():
        want = compiled["F"][name]
        assert len(args) == len(want) - 1, f"{name}: header has {len(want) - 1} parameters, the derived table {len(args)}"
        got = [_kind(res)] + [_kind(t) for t in args]
        assert got == want, f"{name}({L.PARAM_NAMES[name]}): compiler {want}, derived {got}"
        assert len(L.PARAM_NAMES[name]) == len(args)
    assert L.SIGNATURES["a3d_last_error_string"] == (ctypes.c_char_p, [])
    assert L.SIGNATURES["a3d_sincos_host"][0] is None and L.SIGNATURES["a3d_version"] == (ctypes.c_int, [])
    assert L.PARAM_NAMES["a3d_silu_fwd"] == ["x", "y", "n", "stream"]


def test_parameter_blocks_equal_the_compilers_layout(compiled):
    L = load_pkg().lib
    assert set(compiled["S"]) == set(BLOCKS)
    for cname, pyname in BLOCKS.items():
        cls = getattr(L, pyname)
        size, fields = compiled["S"][cname]
        assert ctypes.sizeof(cls) == size, f"{cname}: sizeof {size}, ctypes {ctypes.sizeof(cls)}"
        got = [(f, getattr(cls, f).offset, _kind(t)) for f, t in cls._fields_]
        assert got == fields, f"{cname}: compiler {fields}, derived {got}"
    assert [ctypes.sizeof(getattr(L, p)) for p in BLOCKS.values()] == [104, 56, 176, 232, 128, 96, 96, 48]
    assert L.DnLayerParams._fields_ == [("cross", L.DnCrossParams), ("rest", L.DnRestParams)]


def test_no_declared_entry_is_missed_and_every_one_is_exported():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    header = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    declared = set(re.findall(r"\b(a3d_[a-z0-9_]+)\s*\(", header))                  # what __graft_entry__.build() counts
    assert declared == set(a3d.lib.SIGNATURES) == set(a3d.lib.exported_symbols()), sorted(declared ^ set(a3d.lib.SIGNATURES))
    for s in declared:
        assert hasattr(lib, s), f"{s} is declared in include/act3d_hip.h but not exported"
    assert a3d.lib.ADAMW_CLIP_WS_DOUBLES == 256 and a3d.lib.LR_DECAY_KINDS == {"constant": 0, "linear": 1, "cosine": 2}


def test_a_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    L = load_pkg().lib
    gone = str(tmp_path / "include" / "act3d_hip.h")
    monkeypatch.setattr(L, "HEADER_PATH", gone)
    with pytest.raises(RuntimeError, match=re.escape(gone)):
        L._read_own_header()


@pytest.mark.parametrize("text, names", [
    ("int a3d_bad(long x, void* stream);", ["a3d_bad", "long"]),                              # an unknown scalar type word
    ("int a3d_bad(int a[4]);", ["a3d_bad", "array"]),
    ("int a3d_bad(void (*cb)(int), int n);", ["a3d_bad", "function pointer"]),
    ("typedef struct { int n; } a3d_blk;\nint a3d_bad(a3d_blk b);", ["a3d_bad", "by value"]),
    ("typedef struct { int n; } a3d_blk;\nint a3d_bad(a3d_blk);", ["a3d_bad", "by value"]),
    ("typedef struct { a3d_missing m; int n; } a3d_blk;", ["a3d_blk", "a3d_missing"]),        # a field of an undeclared struct type
    ("typedef struct { unsigned flag : 1; } a3d_blk;", ["a3d_blk", "bit-field"]),
    ("int a3d_bad(int a,\n#if X\n int b,\n#endif\n int c);", ["a3d_bad", "preprocessor"]),
    ("short a3d_bad(void);", ["a3d_bad", "short"]),                                           # an unknown return type
    ("int a3d_bad(int a b);", ["a3d_bad"]),
    ("enum { A3D_X = 1 };", ["A3D_X"]),                                                       # not a prototype, not a block
    ("int a3d_bad(int a)", ["a3d_bad", "unterminated"]),
    ("int a3d_bad(int a);\nint a3d_bad(float a);", ["a3d_bad", "second declaration"]),
])
def test_reader_refuses_what_is_outside_its_rules(text, names):
    L = load_pkg().lib
    with pytest.raises(RuntimeError) as e:
        L.read_header(text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_reader_accepts_the_forms_the_header_uses():
    L = load_pkg().lib
    v, i, u, f, d, z, q = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
                           ctypes.c_ulonglong)
    sigs, names, structs, defines = L.read_header("""
        /* int a3d_commented_out(int a); */
        // int a3d_commented_out_too(int a);
        #ifndef GUARD_H
        #define GUARD_H
        #include <stddef.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define A3D_SOME_COUNT 256
        #define A3D_LR_LINEAR 1
        #define A3D_HEX 0x10
        typedef struct {
          const float *a, *b;        /* two pointers from one declaration */
          int nsplit, slab_stride;
          const unsigned char* mask;
          float eps; double w; size_t n; uint64_t seed;
          float* out;
        } a3d_inner;
        typedef struct {
          a3d_inner first;
          a3d_inner second;
          int F;
        } a3d_outer;
        int a3d_none(void);
        const char* a3d_text();
        void a3d_unnamed(const float*, int, unsigned int, float /* eps */, void* stream);
        size_t a3d_spread(const a3d_outer* p,
                          unsigned long long n, unsigned site,
                          uint32_t word, uint64_t big, double x,
                          const unsigned long long* state, size_t bytes);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert list(sigs) == ["a3d_none", "a3d_text", "a3d_unnamed", "a3d_spread"]           # neither commented-out prototype
    assert sigs["a3d_none"] == (i, []) and sigs["a3d_text"] == (ctypes.c_char_p, [])
    assert sigs["a3d_unnamed"] == (None, [v, i, u, f, v]) and names["a3d_unnamed"] == [None, None, None, None, "stream"]
    assert sigs["a3d_spread"] == (z, [v, q, u, u, q, d, v, z])
    assert names["a3d_spread"] == ["p", "n", "site", "word", "big", "x", "state", "bytes"]
    inner, outer = structs["a3d_inner"], structs["a3d_outer"]
    assert list(structs) == ["a3d_inner", "a3d_outer"] and issubclass(outer, ctypes.Structure)
    assert inner._fields_ == [("a", v), ("b", v), ("nsplit", i), ("slab_stride", i), ("mask", v), ("eps", f), ("w", d), ("n", z),
                              ("seed", q), ("out", v)]
    assert outer._fields_ == [("first", inner), ("second", inner), ("F", i)]
    assert outer.second.offset == ctypes.sizeof(inner) == 72 and ctypes.sizeof(outer) == 152
    assert defines == {"A3D_SOME_COUNT": 256, "A3D_LR_LINEAR": 1, "A3D_HEX": 16}
