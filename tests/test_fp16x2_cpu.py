"""The opt-in fp16x2 arithmetic (math="f32_fp16x2") at the host level: the mode's name, its code and its documented contract."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_math_table_holds_the_fp16x2_mode():
    from acr_wsss_amd import _lib
    assert _lib.MATH == {"f32": 0, "f32_split": 1, "f32_fp16x2": 2}


def test_unknown_math_name_still_raises():
    from acr_wsss_amd.DPT.ACR import ACR
    with pytest.raises(ValueError):
        ACR.set_math(object.__new__(ACR), "f32_fp16")


def test_header_documents_fp16x2():
    with open(os.path.join(ROOT, "include", "acr_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"ACR_MATH_FP16X2\s*=\s*2", hdr)
    rel = float(re.search(r"#define ACR_FP16X2_REL\s+([0-9.e+-]+)", hdr).group(1))
    floor = float(re.search(r"#define ACR_FP16X2_FLOOR\s+([0-9.e+-]+)", hdr).group(1))
    assert rel == 2.0 ** -22 and floor == 2.0 ** -39
    for name in ("acr_h2_image", "acr_h2_image_cols", "acr_h2_image_t", "acr_gemm_h2"):
        assert re.search(r"\bint %s\(" % name, hdr), name
