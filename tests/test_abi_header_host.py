"""CPU-only checks of the Python view of the C ABI, which _lib.parse_header reads from include/vst_hip.h:
the parser on literal header text, the parsed signatures and vst_conv_desc layout against the C++ compiler's
own reading of the header (a host syntax check: nothing is linked or run), and the constants the Python side
uses against the header's names and against the numbers they have always had."""
import ctypes
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P, I, L, F, D, SZ = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double,
                     ctypes.c_size_t)

SAMPLE = r"""
/* A block comment with call-like text: int vst_fake(int a); and an enum { VST_NOT = 7 };
 * spread over lines. */
#ifndef SAMPLE_H
#define SAMPLE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
enum { VST_A = 0, VST_B = 1 };
enum { VST_NEG = -1,   /* a comment between members, with a comma, and a ; */
       VST_BIG = 1024 };
// a line comment with a semicolon; and int vst_fake2(void);
typedef struct some_struct {
  int N, H, W;       /* several per line */
  int pad_mode;
  float slope;       /* the one float */
  int math;
} some_struct;
const char* vst_msg(void);
void vst_set(int a, int b);
int vst_wrapped(const float* x, float* y,
                long n, double scale,
                float eps, void* stream);
size_t vst_bytes(size_t have, int n);
long vst_ld(long P);
int vst_ptrs(const long* y, double* part, int* nsplit, const some_struct* d, float* const* pp);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_declaration_form():
    from gbvst import _lib
    sigs, consts, structs = _lib.parse_header(SAMPLE)
    assert sigs == {
        "vst_msg": (ctypes.c_char_p, []),
        "vst_set": (None, [I, I]),
        "vst_wrapped": (I, [P, P, L, D, F, P]),
        "vst_bytes": (SZ, [SZ, I]),
        "vst_ld": (L, [L]),
        "vst_ptrs": (I, [P, P, P, P, P]),
    }
    assert consts == {"VST_A": 0, "VST_B": 1, "VST_NEG": -1, "VST_BIG": 1024}
    assert structs == {"some_struct": [("N", I), ("H", I), ("W", I), ("pad_mode", I), ("slope", F), ("math", I)]}


@pytest.mark.parametrize("decl", ["int vst_bad(const float* x, unsigned n, void* stream);",
                                  "unsigned vst_bad(int n);",
                                  "int vst_bad(long long n);",
                                  "int vst_bad(int);",
                                  "int vst_bad();"])
def test_parser_refuses_a_type_it_does_not_know(decl):
    from gbvst import _lib
    with pytest.raises(ValueError, match="vst_bad"):
        _lib.parse_header(SAMPLE.replace("long vst_ld(long P);", decl))


@pytest.mark.parametrize("text", ["enum { VST_IMPLICIT, VST_NEXT };", "int vst_a(int n) int vst_b(int n);",
                                  "static const int vst_k = 3;"])
def test_parser_refuses_text_it_cannot_place(text):
    from gbvst import _lib
    with pytest.raises(ValueError):
        _lib.parse_header(text)


# ---- the compiler's reading of the header ---------------------------------------------------------------------
CHECKER = r"""
#include "vst_hip.h"
#include <cstddef>
#include <type_traits>
template <class T> constexpr char cls() {
  if constexpr (std::is_pointer_v<T>) return 'P';
  else if constexpr (std::is_same_v<T, int>) return 'I';
  else if constexpr (std::is_same_v<T, long>) return 'L';
  else if constexpr (std::is_same_v<T, float>) return 'F';
  else if constexpr (std::is_same_v<T, double>) return 'D';
  else if constexpr (std::is_same_v<T, size_t>) return 'Z';
  else if constexpr (std::is_void_v<T>) return 'V';
  else return '?';
}
/* want = the class of the return type, then of each parameter */
template <int M, class R, class... A> constexpr bool sig(R (*)(A...), const char (&want)[M]) {
  const char got[] = {cls<R>(), cls<A>()..., 0};
  if (M != int(sizeof...(A)) + 2) return false;
  for (int i = 0; i < M; ++i)
    if (got[i] != want[i]) return false;
  return true;
}
"""
CLASS = {ctypes.c_void_p: "P", ctypes.c_char_p: "P", ctypes.c_int: "I", ctypes.c_long: "L", ctypes.c_float: "F",
         ctypes.c_double: "D", ctypes.c_size_t: "Z", None: "V"}


def _checker_source(signatures, desc):
    lines = [CHECKER]
    for name, (res, args) in signatures.items():
        want = "".join(CLASS[t] for t in [res] + list(args))
        lines.append('static_assert(sig(&%s, "%s"), "%s");' % (name, want, name))
    lines.append('static_assert(sizeof(vst_conv_desc) == %d, "sizeof(vst_conv_desc)");' % ctypes.sizeof(desc))
    for field in ("slope", "math"):
        lines.append('static_assert(offsetof(vst_conv_desc, %s) == %d, "offsetof %s");'
                     % (field, getattr(desc, field).offset, field))
    return "\n".join(lines) + "\n"


def _compiles(tmp_path, name, source):
    from gbvst import _lib
    path = tmp_path / name
    path.write_text(source)
    r = subprocess.run([_lib.HIPCC, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(REPO, "include"),
                        str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return r.returncode == 0, r.stdout.decode(errors="replace")


def test_compiler_agrees_with_the_parsed_signatures_and_struct(tmp_path):
    from gbvst import _lib
    assert len(_lib.SIGNATURES) >= 177  # the header declares 177 entry points
    assert [n for n, _ in _lib.VstConvDesc._fields_][-2:] == ["slope", "math"]
    ok, out = _compiles(tmp_path, "abi_ok.cpp", _checker_source(_lib.SIGNATURES, _lib.VstConvDesc))
    assert ok, out
    # the same file with ONE wrong entry (vst_adam_step's `long n` as int) must be rejected, and for that entry:
    # a checker that accepts anything does not pass
    res, args = _lib.SIGNATURES["vst_adam_step"]
    assert args[4] is L
    wrong = dict(_lib.SIGNATURES, vst_adam_step=(res, args[:4] + [I] + args[5:]))
    ok, out = _compiles(tmp_path, "abi_wrong.cpp", _checker_source(wrong, _lib.VstConvDesc))
    assert not ok
    assert out.count("static assertion failed") == 1 and "vst_adam_step" in out, out
    # ... as must one argument too few, and a struct the wrong size
    short = dict(_lib.SIGNATURES, vst_adam_step=(res, args[:-1]))
    ok, out = _compiles(tmp_path, "abi_short.cpp", _checker_source(short, _lib.VstConvDesc))
    assert not ok and "vst_adam_step" in out, out

    class Shorter(ctypes.Structure):
        _fields_ = _lib.VstConvDesc._fields_[1:]
    ok, out = _compiles(tmp_path, "abi_desc.cpp", _checker_source(_lib.SIGNATURES, Shorter))
    assert not ok and "sizeof(vst_conv_desc)" in out, out


def test_constants_in_use_are_the_headers_and_keep_their_values():
    from gbvst import _lib, ops
    C = _lib.parse_header(open(os.path.join(REPO, "include", "vst_hip.h")).read())[1]
    in_use = [  # (value the Python side uses, the header's name, the number it has always been)
        (ops.PAD["zero"], "VST_PAD_ZERO", 0), (ops.PAD["reflect"], "VST_PAD_REFLECT", 1),
        (ops.ACT["none"], "VST_ACT_NONE", 0), (ops.ACT["relu"], "VST_ACT_RELU", 1),
        (ops.ACT["lrelu"], "VST_ACT_LRELU", 2), (ops.ACT["tanh"], "VST_ACT_TANH", 3),
        (ops.MERGE["same"], "VST_MERGE_SAME", 0), (ops.MERGE["pool"], "VST_MERGE_POOL", 1),
        (ops.MERGE["up"], "VST_MERGE_UP", 2),
        (ops.PACK_KC, "VST_PACK_KC", 0), (ops.PACK_CK, "VST_PACK_CK", 1), (ops.PACK_OK, "VST_PACK_OK", 2),
        (ops.PACK_IK, "VST_PACK_IK", 3), (ops.PACK_IKF, "VST_PACK_IKF", 4), (ops.PACK_SOK, "VST_PACK_SOK", 5),
        (ops.PACK_FWD, "VST_PACK_OK", 2), (ops.PACK_DGRAD, "VST_PACK_IK", 3),
        (_lib.MATH_MODES["fp32"], "VST_MATH_F32", 0), (_lib.MATH_MODES["bf16x3"], "VST_MATH_BF16X3", 1),
        (_lib.MATH_MODES["bf16x6"], "VST_MATH_BF16X6", 2),
        (ops.EUNSUPPORTED, "VST_EUNSUPPORTED", 2), (ops.WPLAN_BF, "VST_WPLAN_BF", 2),
        (ops.R1_PART_DOUBLES, "VST_R1_PART_DOUBLES", 1024),
        (ops.PLAN_RK, "VST_PLAN_RK", -1), (ops.PLAN_SKINNY, "VST_PLAN_SKINNY", -2),
        (ops.PLAN_C4_DIRECT, "VST_PLAN_C4_DIRECT", -3),
    ]
    for value, name, number in in_use:
        assert value == C[name] == number, (name, value, C[name], number)
    assert (len(ops.PAD), len(ops.ACT), len(ops.MERGE), len(_lib.MATH_MODES)) == (2, 4, 3, 3)
    assert sorted(ops.WPLAN_NAMES) == sorted(v for k, v in C.items() if k.startswith("VST_WPLAN_")) == [0, 1, 2, 3, 4]
