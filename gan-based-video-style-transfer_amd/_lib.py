"""Loader for libvst_hip.so (the C ABI declared in include/vst_hip.h).

The product path has no fallback: if the shared library is missing or fails to load, importing the
ops raises.  The library is built in-tree (``_build/libvst_hip.so``) by :func:`build` with hipcc for
gfx950; it is loaded AFTER torch so that it binds to the HIP runtime torch already loaded
(both export soname libamdhip64.so.7), which keeps torch's streams valid inside the library.
"""
import ctypes
import glob
import os
import re
import subprocess

import torch  # noqa: F401  (must be loaded first: see module docstring)

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
BUILD = os.path.join(PKG, "_build")
LIB_PATH = os.path.join(BUILD, "libvst_hip.so")
# developer A/B runs only: load an alternative build (tools/build_variant.py) instead
LIB_PATH = os.environ.get("VST_LIB_VARIANT") or LIB_PATH
CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(REPO, "include", "vst_hip.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

_lib = None


def source_stamp():
    """Short hash of the kernel sources (csrc/* + include/vst_hip.h) plus the VST_* environment knobs
    that change what the kernels do: profiling records carry it, and a record whose stamp differs from
    the running code's is not used for its numbers."""
    import hashlib
    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(CSRC, "*"))) + [HEADER]:
        if f.endswith((".hip", ".h")):
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    knobs = sorted((k, v) for k, v in os.environ.items()
                   if k.startswith("VST_") and k not in ("VST_CONV_MATH", "VST_LIB_VARIANT"))
    h.update(repr(knobs).encode())
    return h.hexdigest()[:12]


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t}


def _ctype(decl, where, ret=False):
    """ctypes type of one C parameter, field or return type ('const float* x', 'long n', 'void'): every
    pointer is c_void_p (a `const char*` return c_char_p), a scalar outside _SCALARS raises."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return ctypes.c_char_p if ret and words[0] == "char" else ctypes.c_void_p
    if ret and words == ["void"]:
        return None
    if words and words[0] in _SCALARS and len(words) == (1 if ret else 2):
        return _SCALARS[words[0]]
    raise ValueError("vst_hip.h: %s: no ctypes mapping for %r" % (where, " ".join(decl.split())))


def parse_header(text):
    """The Python view of a C ABI header: (signatures, constants, structs).
    signatures: name -> (restype, argtypes) of every `<type> vst_name(<params>);`; constants: every
    `NAME = integer` of the anonymous enums; structs: name -> [(field, ctype)] of every typedef struct.
    Text that is none of these, and a type _ctype does not know, raises: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    constants, structs, signatures = {}, {}, {}

    def enum(m):
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            name, eq, val = (p.strip() for p in item.partition("="))
            if not (eq and re.fullmatch(r"\w+", name)):
                raise ValueError("vst_hip.h: enum member %r has no explicit value" % item)
            constants[name] = int(val, 0)
        return " "

    def struct(m):
        fields = structs[m.group(2)] = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            ctype, _, names = decl.partition(" ")  # `int N, H, W`: one type, several fields
            fields += [(n.strip(), _ctype(ctype + " " + n, "struct " + m.group(2))) for n in names.split(",")]
        return " "

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    *decls, rest = text.split(";")
    if rest.strip() not in ("", "}"):
        raise ValueError("vst_hip.h: text after the last declaration: %r" % rest.strip())
    for decl in decls:
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*", decl)
        if not m:
            raise ValueError("vst_hip.h: not a function declaration: %r" % " ".join(decl.split()))
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        signatures[name] = (_ctype(ret, name, ret=True), [_ctype(p, name) for p in params])
    return signatures, constants, structs


# name -> (restype, argtypes); VST_* enum values; struct fields: all read from the header the library is built from
SIGNATURES, CONSTANTS, STRUCTS = parse_header(open(HEADER).read())
MATH_MODES = {"fp32": CONSTANTS["VST_MATH_F32"], "bf16x3": CONSTANTS["VST_MATH_BF16X3"],
              "bf16x6": CONSTANTS["VST_MATH_BF16X6"]}


class VstConvDesc(ctypes.Structure):
    """include/vst_hip.h vst_conv_desc."""
    _fields_ = STRUCTS["vst_conv_desc"]


# Per-file compiler flags.  conv_bf.hip: no SLP vectorisation — it pairs the operand split's fp32
# subtractions into v_pk_add_f32, which costs ~22-26 extra cycles each beside MFMAs (MI355X_MICROARCH.md
# cycle constants); scalar v_sub_f32 there: x6 ResnetBlock forward 199 -> 193 us (A/B, same box).
FILE_FLAGS = {"conv_bf.hip": ["-fno-slp-vectorize"]}


def apply_route_overrides(module_name, g):
    """Developer A/B of the mirror's route selectors (module attributes the tests flip in-process): the one
    environment variable VST_ROUTES="ops.WGRAD_NHWC=0,networks.TAP_H=0" sets them at import (tools/ab_step.sh
    arms).  Unknown modules and names and an item without a value raise, so a stale or misspelled arm cannot
    silently measure the default."""
    spec = os.environ.get("VST_ROUTES", "").strip()
    if not spec:
        return
    short = module_name.rsplit(".", 1)[-1]
    for item in spec.split(","):
        name, eq, val = item.strip().partition("=")
        mod, _, flag = name.partition(".")
        if not eq:
            raise ValueError("VST_ROUTES: %r is not module.FLAG=value" % item.strip())
        if mod not in ("ops", "networks"):
            raise ValueError("VST_ROUTES: %r names neither ops nor networks" % item.strip())
        if mod != short:
            continue
        if flag not in g:
            raise ValueError("VST_ROUTES: %s has no route flag %s" % (short, flag))
        cur = g[flag]
        g[flag] = (val not in ("0", "false", "False")) if isinstance(cur, bool) else type(cur)(val)


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def build(force=False, verbose=False, out=None, defines=()):
    """Compile every HIP source into _build/libvst_hip.so for gfx950 (cross-compiles without a GPU).
    out/defines: developer variant builds (tools/build_variant.py)."""
    lib_path = out or os.path.join(BUILD, "libvst_hip.so")
    if out is None and any(d.split("=")[0] == "VST_DEV_VARIANT" for d in defines):
        raise ValueError("VST_DEV_VARIANT builds go to a variant path (tools/build_variant.py), never the product library")
    objdir = os.path.join(os.path.dirname(lib_path), "obj_" + os.path.basename(lib_path)[:-3])
    os.makedirs(objdir, exist_ok=True)
    srcs = sources()
    deps = srcs + glob.glob(os.path.join(CSRC, "*.h")) + [HEADER, os.path.abspath(__file__)]
    if not force and os.path.exists(lib_path):
        if os.path.getmtime(lib_path) >= max(os.path.getmtime(d) for d in deps):
            return lib_path
    objs = []
    procs = []
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s) + ".o")
        objs.append(o)
        cmd = [HIPCC, "-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-munsafe-fp-atomics",
               "-Wall", "-Wno-unused-function"] + FILE_FLAGS.get(os.path.basename(s), []) + \
            ["-D" + d for d in defines] + ["-c", s, "-o", o]
        if out is not None:  # developer variant builds only: extra compiler flags
            cmd[1:1] = os.environ.get("VST_VARIANT_HIPCC_FLAGS", "").split()
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode(errors="replace")))
        if verbose and out:
            print(out.decode(errors="replace"))
    tmp = lib_path + ".tmp"
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("link failed: %s\n%s" % (" ".join(cmd), r.stdout.decode(errors="replace")))
    os.replace(tmp, lib_path)
    return lib_path


def load():
    """Return the loaded ctypes library; raises if it is missing (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libvst_hip.so not found at {LIB_PATH}; run __graft_entry__.build() (hipcc, gfx950)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return list(SIGNATURES)


def check(rc, what=""):
    if rc != 0:
        msg = _lib.vst_last_error().decode(errors="replace") if _lib is not None else ""
        raise RuntimeError(f"libvst_hip {what} failed (status {rc}): {msg}")
