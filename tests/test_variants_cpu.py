"""tests/variant_rules.py restates the choices the C entry points make; tests/test_variants_gpu.py relies on the restatements to
say which kernel variant a case reaches.  Without a GPU: every restated predicate still stands in the source it names, and every
case of the GPU file lands on the side it claims."""
import os
import re
from collections import Counter

import pytest

import test_variants_gpu as G
import variant_rules as VR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "acr_wsss_amd", "csrc")


def _normalised(text):
    return re.sub(r"\s+", " ", text).strip()


_SRC = {}


def _source(name):
    if name not in _SRC:
        with open(os.path.join(CSRC, name)) as f:
            _SRC[name] = _normalised(f.read())
    return _SRC[name]


@pytest.mark.parametrize("rule", sorted(VR.SOURCE))
def test_restated_predicate_lines_stand_in_the_source(rule):
    """As test_pseudo_sal_cpu.py ties OPEN_TILE to its #define: a predicate edited in the .hip file makes this fail."""
    assert VR.SOURCE[rule]
    for fname, line in VR.SOURCE[rule]:
        assert _normalised(line) in _source(fname), "%s: %r is no longer in %s -- restate the rule in tests/variant_rules.py" % (rule, line, fname)


def test_every_rule_function_has_its_source_lines():
    fns = {c[1].__name__ for c in G.claims()} | {"gemm_tail_plan", "c3_fwd_ksplit", "conv1x1_ksplit"}
    # the fp32 GroupNorm's plans: their cases are the shapes of tests/test_norm_conditions_gpu.py
    fns |= {"gnf_units", "gnf_reg_plan", "gnf_fwd_parts", "gnf_fwd_variant", "gnf_bwd_variant"}
    assert fns == set(VR.SOURCE)
    for name in fns:
        assert callable(getattr(VR, name))


def test_the_constants_are_the_source_s():
    for fname, name, value in (("gemm_bf16.hip", "GW_BM", VR.GW_BM), ("gemm_bf16.hip", "GB_BN", VR.GB_BN), ("gemm_f32.h", "F_BM", VR.F_BM),
                               ("gemm_f32.h", "F_BN", VR.F_BN), ("gemm_f32.h", "F_BK", VR.F_BK), ("gemm_f32.h", "S_BK", VR.S_BK),
                               ("conv3x3.hip", "C3_BM", VR.C3_BM), ("conv3x3.hip", "C3_BN", VR.C3_BN), ("conv3x3.hip", "C3_BK", VR.C3_BK),
                               ("optim.hip", "SGD_CHUNK", VR.SGD_CHUNK)):
        m = re.search(r"#define %s (\d+)\b" % name, _source(fname))
        assert m and int(m.group(1)) == value, (fname, name)
    assert "tilesw >= %d;" % VR.WIDE_MIN_TILES in _source("gemm_bf16.hip")


def test_every_gpu_case_lands_on_the_side_it_claims():
    cs = G.claims()
    ids = Counter(c[0] for c in cs)
    assert not [i for i, n in ids.items() if n > 1], "case ids must be unique"
    wrong = ["%s: claims %r, the rule says %r" % (cid, side, rule(**kw)) for cid, rule, kw, side in cs if rule(**kw) != side]
    assert not wrong, "\n".join(wrong)


def test_each_choice_has_cases_on_every_side():
    """The point of the GPU file: no rule is exercised on one side only."""
    sides = {}
    for _, rule, kw, side in G.claims():
        sides.setdefault(rule.__name__, set()).add(side)
    assert sides["linear_bf16_variant"] == {"scalar", "dma", "wide"}
    loops = {s[0] for s in sides["gemm_f32_variant"]}
    assert loops == {"planes", "split", "dma", "staged", "refused"}
    assert {s[1] for s in sides["gemm_f32_variant"]} >= {0, 1, 4, 17}        # no tail, one tile, all four tiles, behind whole rounds
    assert sides["sgd_variant"] == {"vec", "scalar"}
    assert sides["maxpool_fwd_variant"] == {"vec4", "scalar"}
    assert sides["maxpool_bwd_variant"] == {"2x8", "8wide", "scalar"}
    assert sides["subsample2_variant"] == {"vec", "scalar"}
    assert sides["conv_ksplit"] == {1, 2}
    assert sides["train_cam_variant"] == {"vec", "scalar"}
    assert sides["sal_pseudo_variant"] == {"vec", "scalar"}


def test_the_scalar_epilogue_cases_cover_all_four_instances():
    scalar = {(kw["bias"] is not None, kw["resid"] is not None) for _, rule, kw, side in G.claims()
              if rule is VR.linear_bf16_variant and side == "scalar"}
    assert scalar == {(False, False), (True, False), (False, True), (True, True)}


def test_tail_plan_edges_are_the_smallest():
    """K = 192 is the smallest contraction with a tail (three parts of two 32-deep chunks); every smaller K % 32 == 0 has none."""
    assert all(VR.gemm_tail_plan(5, 8, K)[0] == 0 for K in range(32, 192, 32))
    assert VR.gemm_tail_plan(5, 8, 192) == (1, 3, 64)
    assert VR.gemm_tail_plan(132, 132, 192) == (4, 3, 64) and VR.gemm_tail_plan(2893, 2900, 192) == (17, 3, 64)
    # the K-split convolutions: one step less of contraction and the launch is not split
    assert VR.c3_fwd_ksplit(2, 48, 32, 240, True) == 2 and VR.c3_fwd_ksplit(2, 48, 16, 240, True) == 1
    assert VR.conv1x1_ksplit(2, 20, 128, 48) == 2 and VR.conv1x1_ksplit(2, 20, 96, 48) == 1


def test_the_library_reports_the_same_workspaces():
    """Host-only queries: a workspace is asked for exactly where the restated plan splits."""
    from acr_wsss_amd import _lib as L
    lib = L.load()
    assert lib.acr_sgd_chunk_elems() == VR.SGD_CHUNK
    for (M, N, K) in [(5, 8, 192), (5, 8, 160), (132, 132, 192), (132, 132, 96), (2893, 2900, 192)]:
        ntail, nsplit, _ = VR.gemm_tail_plan(M, N, K)
        assert lib.acr_gemm_f32_ws_floats(VR.NT, 0, M, N, K) == (ntail * nsplit * VR.F_BM * VR.F_BN + 3) // 4 * 4
    for entry, s, couts, ntap in G.KSPLIT_ENTRIES:
        for cout in couts:
            hw = G._ksplit_hw(entry, s)
            ks = VR.conv_ksplit(entry, 0, s["N"], cout, s["cin"], hw, ntap)
            if entry == "acr_conv_taps_x3":
                n = lib.acr_conv_taps_ws_floats(s["N"], cout, s["cin"], s["H"] // 2, s["W"] // 2, ntap)
            elif entry.startswith("acr_conv3x3"):
                n = lib.acr_conv3x3_ws_floats(s["N"], cout, s["cin"], s["H"], s["W"])
            else:
                n = lib.acr_conv1x1_ws_floats(1, s["N"], cout, s["cin"], hw)
            assert ks == 2 and n == ks * s["N"] * cout * hw, (entry, cout)
