"""The header reader (vqa_playground_pytorch_amd/_abi.py) on a synthetic header that holds every construct it knows, and on
include/vqa_mi355x.h itself: what _lib.SIGNATURES, PARAMS, DEFINES and STRUCTS are derived from.  No GPU, no library call."""
import ctypes as C

import pytest

from vqa_playground_pytorch_amd import _abi, _lib, head, ops

SYNTHETIC = """
/* a comment with a prototype in it: int vqa_fake(int); and an unbalanced ( */
#ifndef VQA_SYNTHETIC_H
#define VQA_SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define VQA_ABI_VERSION 3
#define VQA_E_BAD (-7)   /* with parentheses */
#define VQA_NEG -2
#define VQA_PAREN (12)
typedef void* vqa_stream_t; // hipStream_t; int vqa_fake(int);
typedef uint16_t vqa_bf16_t;
int vqa_scalars(int i, long l, long long ll, unsigned long long ull, size_t sz, uint64_t u64, uint32_t u32, float f,
                double d, vqa_stream_t stream);
int vqa_pointers(const float* a, float* const* b, const float* const* c, void* ws, const void* table,
                 const vqa_bf16_t* h, const uint64_t* seed_ptr, unsigned long long* items,
                 const char* name);
void vqa_nothing(void);
const char* vqa_text(void);
long vqa_l(void);
long long vqa_ll(void);
unsigned long long vqa_ull(void);
size_t vqa_sz(int B);
uint64_t vqa_u64(void);
uint32_t vqa_u32(void);
float vqa_f(void);
double vqa_d(void);
vqa_stream_t vqa_s(void);
void* vqa_p(void);
typedef struct VqaThing {
  const float* A;
  float* const* rows;   /* a host array of device pointers */
  long long stride;
  int a, b;
  uint32_t base;
  float scale;
} VqaThing;
int vqa_things(const VqaThing* things, int n, vqa_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""

VP, CP = C.c_void_p, C.c_char_p


def test_synthetic_header():
    functions, structs, defines = _abi.parse(SYNTHETIC)
    sigs, names = _abi.signatures(functions)
    assert "vqa_fake" not in functions
    assert list(sigs) == ["vqa_scalars", "vqa_pointers", "vqa_nothing", "vqa_text", "vqa_l", "vqa_ll", "vqa_ull", "vqa_sz", "vqa_u64",
                          "vqa_u32", "vqa_f", "vqa_d", "vqa_s", "vqa_p", "vqa_things"]
    assert sigs["vqa_scalars"] == (C.c_int, [C.c_int, C.c_long, C.c_longlong, C.c_ulonglong, C.c_size_t, C.c_uint64, C.c_uint32, C.c_float,
                                             C.c_double, VP])
    assert names["vqa_scalars"] == ["i", "l", "ll", "ull", "sz", "u64", "u32", "f", "d", "stream"]          # (a multi-line prototype)
    assert sigs["vqa_pointers"] == (C.c_int, [VP] * 8 + [CP])
    assert names["vqa_pointers"] == ["a", "b", "c", "ws", "table", "h", "seed_ptr", "items", "name"]
    assert sigs["vqa_nothing"] == (None, []) and names["vqa_nothing"] == []
    assert [sigs[f] for f in list(sigs)[3:14]] == [(t, []) for t in (CP, C.c_long, C.c_longlong, C.c_ulonglong)] + [(C.c_size_t, [C.c_int])] + \
        [(t, []) for t in (C.c_uint64, C.c_uint32, C.c_float, C.c_double, VP, VP)]
    assert sigs["vqa_things"] == (C.c_int, [VP, C.c_int, VP])
    assert defines == {"VQA_ABI_VERSION": 3, "VQA_E_BAD": -7, "VQA_NEG": -2, "VQA_PAREN": 12}            # (not the include guard)
    assert list(structs) == ["VqaThing"]
    thing = _abi.struct_class("VqaThing", structs["VqaThing"])
    assert thing._fields_ == [("A", VP), ("rows", VP), ("stride", C.c_longlong), ("a", C.c_int), ("b", C.c_int), ("base", C.c_uint32),
                              ("scale", C.c_float)]
    assert C.sizeof(thing) == 40 and thing.b.offset == 28


@pytest.mark.parametrize("line,where,c_type", [
    ("int vqa_new(const float* x, short n);", r"vqa_new\(n\)", "short"),
    ("int vqa_new(unsigned n);", r"vqa_new\(n\)", "unsigned"),
    ("int vqa_new(void v);", r"vqa_new\(v\)", "void"),                       # (void is a return type only)
    ("bool vqa_new(void);", "vqa_new", "bool"),
    ("typedef struct VqaNew { float* p; char c; } VqaNew;", r"VqaNew\.c", "char"),
])
def test_an_unknown_type_raises_naming_the_function_and_the_type(line, where, c_type):
    functions, structs, _ = _abi.parse(line)
    with pytest.raises(_abi.AbiError, match="%s: no ctypes type for the C type '%s'" % (where, c_type)):
        _abi.signatures(functions)
        for name, fields in structs.items():
            _abi.struct_class(name, fields)


@pytest.mark.parametrize("text", ["int vqa_callback(void (*fn)(int), int n);", "struct VqaBare { int a; };", "int vqa_unfinished(int a"])
def test_text_the_reader_does_not_know_raises(text):
    with pytest.raises(_abi.AbiError, match="cannot read the header"):
        _abi.parse("int vqa_before(int a);\n%s\nint vqa_after(void);" % text)


# ---- the real header ---------------------------------------------------------------------------------------------------------
SIZES = {"*": 8, "long long": 8, "uint64_t": 8, "int": 4, "uint32_t": 4, "float": 4}          # the LP64 ABI the library is built for


def _natural_layout(fields):
    """-> ([offset of each field], sizeof) of a C struct under natural alignment: every field on a multiple of its own size, the whole
    on a multiple of the largest"""
    offsets, end = [], 0
    sizes = [SIZES["*" if t.endswith("*") else t] for _, t in fields]
    for size in sizes:
        end = -(-end // size) * size
        offsets.append(end)
        end += size
    return offsets, -(-end // max(sizes)) * max(sizes)


@pytest.mark.parametrize("name,count,size", [("VqaGemmProblem", 31, 168), ("VqaEpilogueJob", 24, 136)])
def test_struct_classes_have_the_headers_layout(name, count, size):
    fields = _lib._structs[name]
    cls = _lib.STRUCTS[name]
    assert cls in (head.GemmProblem, head.EpilogueJob)
    assert len(fields) == count and [f for f, _ in cls._fields_] == [f for f, _ in fields]
    offsets, total = _natural_layout(fields)
    assert [getattr(cls, f).offset for f, _ in fields] == offsets and C.sizeof(cls) == total == size
    assert [C.sizeof(t) for _, t in cls._fields_] == [SIZES["*" if t.endswith("*") else t] for _, t in fields]
    assert fields[0][1].endswith("*") and offsets[:2] == [0, 8]


def test_the_binding_is_the_headers():
    assert list(_lib.PARAMS) == list(_lib.SIGNATURES)
    assert all(len(_lib.PARAMS[f]) == len(_lib.SIGNATURES[f][1]) for f in _lib.SIGNATURES)
    assert _lib.SIGNATURES["vqa_launch_log"] == (C.c_int, [VP, C.c_int]) and _lib.PARAMS["vqa_launch_log"] == ["items", "capacity"]
    assert _lib.SIGNATURES["vqa_set_option"] == (C.c_int, [CP, CP]) and _lib.SIGNATURES["vqa_last_error"] == (CP, [])
    assert _lib.SIGNATURES["vqa_rmsprop_step"][1][5:8] == [C.c_float, C.c_double, C.c_float]
    assert _lib.PARAMS["vqa_softmax_attention_pool_len_fwd"][2] == "lens"
    stream_last = [f for f, p in _lib.PARAMS.items() if p and p[-1] == "stream"]
    assert len(stream_last) > 100 and all(_lib.SIGNATURES[f][1][-1] is VP for f in stream_last)
    assert _lib.ABI_VERSION == _lib.DEFINES["VQA_ABI_VERSION"] == 14
    assert (head.MAX_GROUP, head.MAX_GEMMS, ops.PACK_BLOCK) == tuple(_lib.DEFINES[k] for k in ("VQA_GROUPED_MAX", "VQA_GROUPED_GEMM_MAX",
                                                                                              "VQA_PACK_BLOCK"))
    assert [head.EPI_SUM, head.EPI_LINEAR, head.EPI_RANK_PRODUCT, head.EPI_GRAD, head.EPI_RANK_PRODUCT_BWD] == [
        _lib.DEFINES["VQA_EPI_" + k] for k in ("SUM", "LINEAR", "RANK_PRODUCT", "GRAD", "RANK_PRODUCT_BWD")] == [0, 1, 2, 3, 4]


def test_a_missing_header_is_a_library_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib._srchash, "INCLUDE", str(tmp_path))
    with pytest.raises(_lib.VqaLibraryError, match="vqa_mi355x.h not found"):
        _lib._read_header()
