"""The header parser (acr_wsss_amd/_abi.py) on short synthetic headers -- every construct it accepts, every refusal with the
offending line in the message --, the five device-table records byte for byte against struct formats written out here (the
test's own statement of the C layout), and the GPU-free halves of the five table builders on fake addresses."""
import ctypes
import struct

import numpy as np
import pytest

from acr_wsss_amd import _abi

A, B, C, D = 0x1122334455667788, 0x7FEEDDCCBBAA9988, 0x0123456789ABCDEF, 0x7EDCBA9876543210     # recognisable addresses


def test_guards_includes_and_cplusplus_lines_are_ignored():
    text = '#ifndef X_H\n#define X_H\n#include <stddef.h>\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n' \
           'int f(void);\n#ifdef __cplusplus\n}\n#endif\n#endif /* X_H */\n'
    protos, consts, structs = _abi.parse(text)
    assert protos == {"f": (ctypes.c_int32, [])} and consts == {} and structs == {}


def test_defines_and_enums_become_constants():
    text = "#define N 2      /* why */\n#define REL 2.5e-07\n#define NEG -3\n" \
           "typedef enum e { E_A = 0, E_B = -1,   /* note */\n E_C = 7, } e;\n"
    assert _abi.parse(text)[1] == {"N": 2, "REL": 2.5e-07, "NEG": -3, "E_A": 0, "E_B": -1, "E_C": 7}
    assert isinstance(_abi.parse(text)[1]["N"], int)


def test_struct_members_follow_the_header_in_order():
    text = "typedef struct rec {\n  const void* src;   /* pointer member */\n  float* dst;\n  int32_t rows, cols;\n" \
           "  uint64_t p0, p1;\n  uint8_t flag;\n  int64_t n;\n  float scale;\n  double eps;\n} rec;\n"
    rec = _abi.parse(text)[2]["rec"]
    assert issubclass(rec, ctypes.Structure)
    assert rec._fields_ == [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                            ("p0", ctypes.c_uint64), ("p1", ctypes.c_uint64), ("flag", ctypes.c_uint8), ("n", ctypes.c_int64),
                            ("scale", ctypes.c_float), ("eps", ctypes.c_double)]
    assert [getattr(rec, k).offset for k in ("src", "rows", "p0", "flag", "n", "eps")] == [0, 16, 24, 40, 48, 64]   # C's padding
    assert ctypes.sizeof(rec) == 72


def test_prototypes_over_the_closed_type_set():
    text = "typedef struct d { int32_t B; } d;\n" \
           "int         version(void);\nconst char* last_error(void);\nint64_t floats(const d* desc);\n" \
           "size_t ws(int32_t M, int N);\nint32_t chunk(void);\nvoid nothing(void);\n" \
           "int tables(void* ws, int32_t n, void** offsets,\n           void** weights);\n" \
           "int run(const d* desc, const float* x, float* y, const uint8_t* gt, int64_t* raw, const int32_t* cls, double* st,\n" \
           "        uint64_t key, uint8_t flag, int64_t ld, float lr, double eps, size_t n, void* stream);\n"
    p = _abi.parse(text)
    dp, vp = ctypes.POINTER(p[2]["d"]), ctypes.c_void_p
    assert p[0] == {
        "version": (ctypes.c_int32, []), "last_error": (ctypes.c_char_p, []), "floats": (ctypes.c_int64, [dp]),
        "ws": (ctypes.c_size_t, [ctypes.c_int32, ctypes.c_int32]), "chunk": (ctypes.c_int32, []), "nothing": (None, []),
        "tables": (ctypes.c_int32, [vp, ctypes.c_int32, ctypes.POINTER(vp), ctypes.POINTER(vp)]),
        "run": (ctypes.c_int32, [dp, vp, vp, vp, vp, vp, vp, ctypes.c_uint64, ctypes.c_uint8, ctypes.c_int64, ctypes.c_float,
                                 ctypes.c_double, ctypes.c_size_t, vp])}
    inst = p[2]["d"]()
    assert dp.from_param(inst) is not None                       # an instance is passed where a struct pointer is declared


@pytest.mark.parametrize("text, line", [
    ("int f(int32_t a);\nint g(long n, void* stream);\n", "int g(long n, void* stream)"),             # an unknown type
    ("int f(char* s);\n", "int f(char* s)"),                                                           # char only as a const char* return
    ("typedef struct s { unsigned n; } s;\n", "unsigned n"),
    ("typedef enum e { E_A, E_B = 1 } e;\n", "E_A"),                                                   # an enum without explicit values
    ("#define SQ(x) ((x) * (x))\n", "#define SQ(x) ((x) * (x))"),                                     # a function-like macro
    ("int f(int32_t a,\n#ifdef WIDE\n      int64_t b,\n#endif\n      void* stream);\n", "#ifdef WIDE"),   # a split prototype
    ("#define NAME other\n", "#define NAME other"),
    ("#ifdef WIDE\nint f(void);\n#endif\n", "#ifdef WIDE"),
    ("int f(int32_t);\n", "int f(int32_t)"),                                                           # a parameter without a name
    ("int f(void);\nint f(void);\n", "int f(void)"),
    ("typedef struct s { float *a, *b; } s;\n", "float *a, *b"),
    ("int f(void)\n", "int f(void)"),                                                                  # no ';'
    ("static inline int f(void) { return 0; }\n", "static inline int f(void)"),
    ('#ifdef __cplusplus\nextern "C" {\nint f(void);\n#endif\n', "int f(void);"),                    # nothing is skipped in a C++ block
    ("#define N 2\n#define N 3\n", "#define N 3"),                                                    # no name is defined twice
    ("#define E_A 2\ntypedef enum e { E_A = 1 } e;\n", "E_A = 1"),
    ("typedef struct s { int n; } s;\ntypedef struct s { float x; } s;\n", "float x"),
])
def test_what_does_not_fit_raises_and_names_the_line(text, line):
    with pytest.raises(_abi.HeaderError) as e:
        _abi.parse(text)
    assert line in str(e.value) and "line " in str(e.value)


def test_the_real_header_parses_whole():
    assert len(_abi.prototypes) >= 153 and all(k.startswith("acr_") for k in _abi.prototypes)
    assert _abi.constants["ACR_ABI_VERSION"] == 2 and _abi.constants["ACR_ERR_UNSUPPORTED"] == -3
    assert _abi.constants["ACR_FP16X2_REL"] == 2.0 ** -22 and _abi.constants["ACR_FP16X2_FLOOR"] == 2.0 ** -39
    assert set(_abi.structs) == {"acr_attn_desc", "acr_x3_many_desc", "acr_sgd_tensor", "acr_tr_tensor", "acr_wstd_desc", "acr_pre_image"}


# ---- the five device-table records: the format strings are this test's statement of the C layout ---------------------------------
RECORDS = {
    "acr_tr_tensor": ("<QQ4i", 32, (A, B, 130, 72, 6, 2)),
    "acr_sgd_tensor": ("<4Qq", 40, (A, B, C, D, 2 ** 40 + 5)),
    "acr_x3_many_desc": ("<QQ8i", 48, (A, B, 200, 72, 73, 8, -1, 9, 4, 5)),
    "acr_wstd_desc": ("<4Q4i", 48, (A, B, C, D, 64, 147, 320, 0)),
    "acr_pre_image": ("<q11i4x", 56, (2 ** 33 + 16, 375, 500, 448, 597, 1, 2, 3, 4, 5, 446, 445)),
}


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_record_bytes_equal_the_c_layout(name):
    fmt, size, values = RECORDS[name]
    dt = _abi.record_dtype(name)
    assert dt.itemsize == struct.calcsize(fmt) == size == ctypes.sizeof(_abi.structs[name])
    assert len(set(values)) == len(values) == len(dt.names)                 # a distinct value per field: a swap shows
    rec = np.zeros(1, dt)
    for k, v in zip(dt.names, values):
        rec[k] = v
    assert rec.tobytes() == struct.pack(fmt, *values)
    if name == "acr_pre_image":
        assert rec.tobytes()[-4:] == bytes(4) and [dt.fields[k][1] for k in ("offset", "h", "flip", "cw")] == [0, 8, 24, 48]


# ---- the five table builders' GPU-free halves, two records each ----- -----------------------------------------------------------
def test_sgd_table_is_the_five_int64_columns():
    from acr_wsss_amd import train
    host = np.zeros((2, 5), np.int64)                           # the pinned staging buffer's shape and type
    train.sgd_records(host, grad=[A, 0], master=[B, C], mom=[C, D], param=[D, A], n=[2 ** 40 + 5, 7])
    assert host.tobytes() == struct.pack("<4Qq", A, B, C, D, 2 ** 40 + 5) + struct.pack("<4Qq", 0, C, D, A, 7)
    assert host.tolist() == [[A, B, C, D, 2 ** 40 + 5], [0, C, D, A, 7]]              # grad, master, mom, param, n by column
    train.sgd_records(host, grad=[0, A], master=[B, C], mom=[0, D], param=0, n=(3, 4))   # the all-fp32 table: no param
    assert host.tolist() == [[0, B, 0, 0, 3], [A, C, D, 0, 4]]


def test_pre_image_table():
    from acr_wsss_amd import data
    assert data.PRE_IMAGE == _abi.record_dtype("acr_pre_image") and "_pad" not in data.PRE_IMAGE.names
    rec = np.zeros(2, data.PRE_IMAGE)
    rec[0] = (0, 375, 500, 448, 597, 1, 0, 0, 0, 75, 448, 448)
    rec[1] = (0, 30, 40, 24, 32, 0, 4, 0, 0, 0, 24, 32)
    raw = data.table_bytes(rec, [0, 562512], extra=[2 ** 33, -1])
    assert raw.dtype == np.uint8 and raw.tobytes() == (struct.pack("<q11i4x", 0, 375, 500, 448, 597, 1, 0, 0, 0, 75, 448, 448)
                                                      + struct.pack("<q11i4x", 562512, 30, 40, 24, 32, 0, 4, 0, 0, 0, 24, 32)
                                                      + struct.pack("<2q", 2 ** 33, -1))
    assert rec["offset"].tolist() == [0, 0]                     # the caller's records are not written


def test_transpose_table_and_its_running_tile0():
    from acr_wsss_amd import ops
    rec, blk, n = ops.transpose_records([A, C], [B, D], [(130, 72), (64, 200)])             # 3 x 2 and 1 x 4 tiles of 64 x 64
    assert rec.tobytes() == struct.pack("<QQ4i", A, B, 130, 72, 0, 2) + struct.pack("<QQ4i", C, D, 64, 200, 6, 4)
    assert blk.dtype == np.int32 and blk.tolist() == [0] * 6 + [1] * 4 and n == 10


def test_x3_many_table_and_its_running_wg0():
    from acr_wsss_amd import ops
    rec, blk, n = ops.x3_many_records([A, C], [B, D], [(200, 72, 73, 8, -1, 9), (64, 144, 144, 16, 16, 1)])
    assert rec.tobytes() == (struct.pack("<QQ8i", A, B, 200, 72, 73, 8, -1, 9, 0, 5)        # nkb 5: 2 row blocks x 2 groups of 4
                             + struct.pack("<QQ8i", C, D, 64, 144, 144, 16, 16, 1, 4, 9))   # nkb 9: 1 row block x 3 groups
    assert blk.dtype == np.int32 and blk.tolist() == [0] * 4 + [1] * 3 and n == 7
    with pytest.raises(AssertionError):
        ops.x3_many_records([A], [B], [(8, 12, 12, 8, 8, 1)])                               # K no multiple of 8


def test_wstd_table_and_its_ch_start_sums():
    from acr_wsss_amd import ops
    rec, total = ops.wstd_records([A, D], [B, A], [0, B], [C, 0], [64, 256], [147, 64])
    assert rec.tobytes() == struct.pack("<4Q4i", A, B, 0, C, 64, 147, 0, 0) + struct.pack("<4Q4i", D, A, B, 0, 256, 64, 64, 0)
    assert total == 320
