"""ctypes binding of libact3d_hip.so, derived from include/act3d_hip.h.

The header is the only description of the C ABI.  read_header() turns its prototypes, parameter blocks (typedef struct) and integer
#defines into the ctypes signatures, Structure classes and constants below, once, at import; a new entry point needs no edit here.
A declaration outside the reader's rules is an error that quotes it, never a guess.
There is no CPU fallback: if the shared library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import re

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# development aid: A3D_LIB names another build of the same library inside the package directory (A/B builds made with
# A3D_HIPCC_FLAGS and A3D_LIB_OUT, e.g. libact3d_hip_occ3.so); the default library is the one build() makes
LIB_PATH = os.path.join(_PKG_DIR, os.path.basename(os.environ.get("A3D_LIB", "libact3d_hip.so")))
HEADER_PATH = os.path.join(os.path.dirname(_PKG_DIR), "include", "act3d_hip.h")       # build.INCLUDE

# by-value C types the ABI may use; anything with a `*` is a c_void_p
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "uint32_t": C.c_uint, "float": C.c_float,
            "double": C.c_double, "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong, "uint64_t": C.c_ulonglong}


def _refuse(why, decl):
    raise RuntimeError("act3d_hip.h: %s in `%s`" % (why, " ".join(decl.split())))


def _no_const(text):
    return " ".join(w for w in text.split() if w != "const")


def _declare(text, structs, whole):
    """[(name or None, ctypes type)] of one parameter or one field declaration, e.g. `const float *a, *b` or `int n`."""
    for mark, why in (("(", "a function pointer"), ("[", "an array"), (":", "a bit-field"), ("{", "a nested declaration")):
        if mark in text:
            _refuse(why, whole)
    first, *more = [d.strip() for d in text.split(",")]
    words = first.split()
    if not words:
        _refuse("an empty declaration", whole)
    if "*" in first:
        base, first = first.split("*", 1)[0], "*" + first.split("*", 1)[1]
    elif _no_const(first) in _SCALARS or _no_const(first) in structs:      # a whole type: an unnamed parameter
        base, first = first, ""
    else:
        base, first = " ".join(words[:-1]), words[-1]
    base, out = _no_const(base), []
    for d in [first] + more:
        name = _no_const(d.replace("*", " ")).split()
        if len(name) > 1 or (name and not re.fullmatch(r"[A-Za-z_]\w*", name[0])):
            _refuse("an unreadable declarator `%s`" % d, whole)
        if "*" not in d and base not in _SCALARS and base not in structs:
            _refuse("the unknown type `%s`" % base, whole)
        out.append((name[0] if name else None, C.c_void_p if "*" in d else _SCALARS.get(base) or structs[base]))
    return out


def read_header(text):
    """(signatures, param_names, structs, defines) of a C header's text: name -> (restype, argtypes), name -> parameter names (None
    for an unnamed one), typedef name -> ctypes.Structure class, A3D_* macro -> int."""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    signatures, param_names, structs, defines, decls, cur, depth = {}, {}, {}, {}, [], "", 0
    for line in text.splitlines():
        s = line.strip()
        if s.startswith("#"):
            if cur.strip() or s.endswith("\\"):
                _refuse("a preprocessor line inside a declaration", cur + " " + s)
            m = re.fullmatch(r"#\s*define\s+(A3D_\w+)\s+(-?(?:0[xX][0-9a-fA-F]+|\d+))", s)
            if m:
                defines[m.group(1)] = int(m.group(2), 0)
            continue
        if re.fullmatch(r'extern\s+"C"\s*\{', s) or (s == "}" and not cur.strip()):      # the linkage block's two lines
            continue
        for ch in s + " ":
            cur += ch
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                decls.append(cur[:-1].strip())
                cur = ""
    if cur.strip():
        _refuse("an unterminated declaration", cur)
    for decl in decls:
        block = re.fullmatch(r"typedef\s+struct\s*\w*\s*\{(.*)\}\s*(\w+)", decl, flags=re.S)
        proto = re.fullmatch(r"([\w\s*]+?)\b(a3d_\w+)\s*\((.*)\)", decl, flags=re.S)
        if (block and block.group(2) in structs) or (proto and proto.group(2) in signatures):
            _refuse("a second declaration of the same name", decl)
        if block:
            fields = [f for part in block.group(1).split(";") if part.strip() for f in _declare(part, structs, decl)]
            structs[block.group(2)] = type(block.group(2), (C.Structure,), {"_fields_": fields})
        elif proto:
            ret, name, params = _no_const(proto.group(1)), proto.group(2), proto.group(3).strip()
            if "*" in ret:
                res = C.c_char_p if ret.replace(" ", "") == "char*" else C.c_void_p
            elif ret != "void" and ret not in _SCALARS:
                _refuse("the unknown return type `%s`" % ret, decl)
            else:
                res = _SCALARS.get(ret)
            if "(" in params:
                _refuse("a function pointer", decl)
            args = [] if params in ("", "void") else [a for p in params.split(",") for a in _declare(p, structs, decl)]
            if any(issubclass(t, C.Structure) for _, t in args):
                _refuse("a struct passed by value", decl)
            signatures[name], param_names[name] = (res, [t for _, t in args]), [n for n, _ in args]
        else:
            _refuse("a declaration this reader does not know", decl)
    return signatures, param_names, structs, defines


def _read_own_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError("include/act3d_hip.h is missing (%s): the ctypes binding is derived from it" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return read_header(f.read())


# name -> (restype, argtypes), name -> parameter names; the header's structs and integer macros
SIGNATURES, PARAM_NAMES, _STRUCTS, _DEFINES = _read_own_header()

# parameter blocks of the fused denoise kernels, of the fused query-stream layer, and one record of the deferred
# gradient-reduction table, under their Python names
DnHeadParams = _STRUCTS["a3d_dn_head_params"]
DnCrossParams = _STRUCTS["a3d_dn_cross_params"]
DnRestParams = _STRUCTS["a3d_dn_rest_params"]
DnLayerParams = _STRUCTS["a3d_dn_layer_params"]
DnTailParams = _STRUCTS["a3d_dn_tail_params"]
QsParams = _STRUCTS["a3d_qs_params"]
QsGrads = _STRUCTS["a3d_qs_grads"]
GradReduceRec = _STRUCTS["A3dGradReduceRec"]

# doubles in a3d_adamw_clip_step's clip_ws = workgroups of its norm pass
ADAMW_CLIP_WS_DOUBLES = _DEFINES["A3D_ADAMW_CLIP_WS_DOUBLES"]
# a3d_adamw_sched_step's decay_kind: {"constant": A3D_LR_CONSTANT, "linear": .., "cosine": ..}
LR_DECAY_KINDS = {k[len("A3D_LR_"):].lower(): v for k, v in _DEFINES.items() if k.startswith("A3D_LR_")}

# pins per scene of one a3d_traj_pins call
TRAJ_PINS_MAX = _DEFINES["A3D_TRAJ_PINS_MAX"]
# spheres of one a3d_traj_body_clearance body
TRAJ_BODY_MAX_SPHERES = _DEFINES["A3D_TRAJ_BODY_MAX_SPHERES"]

_lib = None


def load():
    """Load (once) and return the ctypes handle.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libact3d_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(needs hipcc); there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError("libact3d_hip.so does not export %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return list(SIGNATURES.keys())


def last_error():
    s = load().a3d_last_error_string()
    return s.decode() if s else ""


def _failure(what, rc):
    return RuntimeError("%s failed with code %d: %s" % (what, rc, last_error()))


def check(rc, what):
    if rc != 0:
        raise _failure(what, rc)


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The tensor must be contiguous."""
    if t is None:
        return None
    assert t.is_contiguous(), "libact3d_hip needs contiguous tensors"
    return t.data_ptr()


def nz(t):
    """Device pointer of a tensor (None -> NULL), unchecked: for operands whose layout the caller has already established."""
    return None if t is None else t.data_ptr()


byref = C.byref


def stream():
    return torch.cuda.current_stream().cuda_stream


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("act3d_amd ops run on an MI355X device tensor; got a %s tensor "
                               "(there is no CPU fallback)" % t.device)


def call(name, *args):
    rc = getattr(load(), name)(*args)               # no call in between: this is the per-launch cost of every eager op
    if rc != 0:
        raise _failure(name, rc)
