"""The binding's table is derived from include/rpst.h: rpst._lib.parse_header on small header
texts written here (every form the real header uses), then on the real header against counts
taken independently of the parser. No GPU and no built library needed."""
import ctypes
import re

import pytest

from rpst import _lib
from test_abi import HEADER, header_functions

P = ctypes.c_void_p
FRAME = """/* a header; mentions rpst_in_a_comment(int a, float b); and a stray ) */
#ifndef RPST_H_
#define RPST_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* rpst_stream_t;
%s
#ifdef __cplusplus
}  /* extern "C" */
#endif
#endif /* RPST_H_ */
"""


def parse(body):
    return _lib.parse_header(FRAME % body)


def test_one_prototype_per_mapped_type():
    sigs, consts = parse("""
int rpst_i(int a);
int rpst_i64(int64_t n);
int rpst_f(float eps);
int rpst_d(double scale);
int rpst_sz(size_t bytes);
int rpst_stream(rpst_stream_t stream);
int rpst_ptrs(const float* a, float* b, const uint8_t* c, int32_t* d, const double* e, void* ws,
              const void* cws, int* out);
size_t rpst_size(int N, int C);
int64_t rpst_threads(int N);
""")
    assert consts == {}
    assert sigs == {
        "rpst_i": (ctypes.c_int, [ctypes.c_int]),
        "rpst_i64": (ctypes.c_int, [ctypes.c_int64]),
        "rpst_f": (ctypes.c_int, [ctypes.c_float]),
        "rpst_d": (ctypes.c_int, [ctypes.c_double]),
        "rpst_sz": (ctypes.c_int, [ctypes.c_size_t]),
        "rpst_stream": (ctypes.c_int, [P]),
        "rpst_ptrs": (ctypes.c_int, [P] * 8),
        "rpst_size": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
        "rpst_threads": (ctypes.c_int64, [ctypes.c_int]),
    }
    assert _lib._P is P


def test_multi_line_prototype_with_comments():
    sigs, _ = parse("""
/* ---- out = f(x), see rpst_x(a, b) (and base.py:1-2) ---- */
int rpst_y(const float* x, /* (N, C, HW), contiguous */ float* out,   // written, all of it
           int N, int C,  /* as rpst_x(N, C) takes them */
           int64_t HW, float eps,
           rpst_stream_t stream);  /* ordered on stream, like rpst_x( */
// int rpst_commented_out(int a);
""")
    assert sigs == {"rpst_y": (ctypes.c_int, [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                              ctypes.c_float, P])}


def test_void_and_empty_argument_lists_and_char_return():
    sigs, _ = parse("int rpst_version(void);\nsize_t rpst_sq_diff_workspace_size();\n"
                    "const char* rpst_last_error(void);\nint rpst_text(const char* s);")
    assert sigs == {"rpst_version": (ctypes.c_int, []),
                    "rpst_sq_diff_workspace_size": (ctypes.c_size_t, []),
                    "rpst_last_error": (ctypes.c_char_p, []),
                    "rpst_text": (ctypes.c_int, [P])}


def test_defines():
    sigs, consts = parse("""
#define RPST_OK 0
#define RPST_EINVAL (-1)  /* bad argument (or shape), see rpst_x() */
#define RPST_IN_ADAIN 4 /* a comment that
                           goes on: #define RPST_NOT_THIS 9 */
#define RPST_WCT_TIMEOUT 4 // bit
#define OTHER_THING 3
int rpst_version(void);
""")
    # RPST_H_ (the guard in FRAME) has no value and is not a constant
    assert consts == {"RPST_OK": 0, "RPST_EINVAL": -1, "RPST_IN_ADAIN": 4, "RPST_WCT_TIMEOUT": 4}
    assert list(sigs) == ["rpst_version"]


@pytest.mark.parametrize("proto,kind", [
    ("int rpst_bad(const float* x, uint8_t flag, rpst_stream_t stream);", "uint8_t"),
    ("int rpst_bad(unsigned n);", "unsigned"),
    ("int rpst_bad(long long n);", "long long"),
    ("void rpst_bad(int n);", "void"),
])
def test_unknown_type_raises_naming_function_and_type(proto, kind):
    with pytest.raises(_lib.RpstError, match=rf"rpst_bad.*`{kind}`"):
        parse("int rpst_good(int a);\n" + proto)


@pytest.mark.parametrize("statement", ["int rpst_cb(void (*fn)(int), int n);",
                                       "int rpst_arr(const float w[9]);", "int rpst_global;"])
def test_what_is_no_plain_prototype_raises(statement):
    with pytest.raises(_lib.RpstError, match="rpst_"):
        parse(statement)


# ---- the real header ----------------------------------------------------------------------
def real_text():
    with open(HEADER) as f:
        return f.read()


def prototypes(text):
    """{name: number of parameters}, counted without the parser: comments out, each `name(...);`
    split on its top-level commas."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//.*", "", text)
    out = {}
    for m in re.finditer(r"\b(rpst_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", text):
        depth, commas = 0, 0
        for ch in m[2]:
            depth += (ch in "([") - (ch in ")]")
            commas += ch == "," and depth == 0
        out[m[1]] = 0 if m[2].strip() in ("", "void") else commas + 1
    return out


def test_real_header_every_prototype_with_its_arity():
    sigs, _ = _lib.parse_header(real_text())
    assert sorted(sigs) == header_functions() and len(sigs) == len(header_functions())
    counted = prototypes(real_text())
    assert sorted(counted) == sorted(sigs)
    assert {k: len(v[1]) for k, v in sigs.items()} == counted
    assert sigs == _lib.SIGNATURES and isinstance(_lib.SIGNATURES, dict)
    assert all(res in (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_char_p)
               for res, _ in sigs.values())


def test_argtype_follows_the_header():
    """`int64_t HW` -> `int HW` in rpst_calc_mean_std alone changes that one argtype alone."""
    text = real_text()
    m = re.search(r"int rpst_calc_mean_std\([^;]*;", text)
    assert m[0].count("int64_t HW") == 1
    edited = text[:m.start()] + m[0].replace("int64_t HW", "int HW") + text[m.end():]
    before, consts = _lib.parse_header(text)
    after, consts_after = _lib.parse_header(edited)
    assert consts == consts_after and list(before) == list(after)
    changed = [(name, i, a, b) for name in before
               for i, (a, b) in enumerate(zip(before[name][1], after[name][1])) if a is not b]
    assert changed == [("rpst_calc_mean_std", 5, ctypes.c_int64, ctypes.c_int)]
    assert all(before[n][0] is after[n][0] and len(before[n][1]) == len(after[n][1])
               for n in before)


# the one place the header's values are restated: renumbering a code shows up here
CONSTANTS = {
    "RPST_OK": 0, "RPST_EINVAL": -1, "RPST_EHIP": -2, "RPST_EWORKSPACE": -3,
    "RPST_PAD_ZERO": 0, "RPST_PAD_REFLECT": 1,
    "RPST_IN_NONE": 0, "RPST_IN_MAXPOOL2": 1, "RPST_IN_UPSAMPLE2": 2, "RPST_IN_ADD_UPSAMPLE2": 3,
    "RPST_IN_ADAIN": 4, "RPST_IN_ADD_ADAIN": 5,
    "RPST_ACT_NONE": 0, "RPST_ACT_RELU": 1, "RPST_ACT_LRELU": 2,
    "RPST_CONV_DIRECT": 0, "RPST_CONV_WINOGRAD": 1, "RPST_CONV_WINOGRAD4": 2,
    "RPST_CONV_NARROW": 3,
    "RPST_WCT_NOCONV": 1, "RPST_WCT_TIMEOUT": 4,
}


def test_real_header_constants():
    assert _lib.parse_header(real_text())[1] == CONSTANTS == _lib.CONSTANTS
    assert len(CONSTANTS) == 21
    assert _lib.constants("PAD_REFLECT", "WCT_TIMEOUT", "EINVAL") == (1, 4, -1)
    with pytest.raises(KeyError, match="RPST_NO_SUCH_CODE"):
        _lib.constants("NO_SUCH_CODE")


def test_ops_names_carry_the_header_values():
    from rpst import ops
    names = {"PAD_ZERO": "PAD_ZERO", "PAD_REFLECT": "PAD_REFLECT", "IN_NONE": "IN_NONE",
             "IN_MAXPOOL2": "IN_MAXPOOL2", "IN_UPSAMPLE2": "IN_UPSAMPLE2",
             "IN_ADD_UPSAMPLE2": "IN_ADD_UPSAMPLE2", "IN_ADAIN": "IN_ADAIN",
             "IN_ADD_ADAIN": "IN_ADD_ADAIN", "ACT_NONE": "ACT_NONE", "ACT_RELU": "ACT_RELU",
             "ACT_LRELU": "ACT_LRELU", "ALGO_DIRECT": "CONV_DIRECT",
             "ALGO_WINOGRAD": "CONV_WINOGRAD", "ALGO_WINOGRAD4": "CONV_WINOGRAD4",
             "ALGO_NARROW": "CONV_NARROW", "WCT_NOCONV": "WCT_NOCONV",
             "WCT_TIMEOUT": "WCT_TIMEOUT"}
    assert {k: getattr(ops, k) for k in names} == {k: CONSTANTS["RPST_" + v]
                                                   for k, v in names.items()}
    assert ops._ALGO_TAG == {0: "conv", 1: "wino", 2: "wino4", 3: "narrow"}


def test_missing_header_names_the_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "rpst.h"))
    with pytest.raises(_lib.RpstError, match=re.escape(str(tmp_path / "include" / "rpst.h"))):
        _lib._read_header()
