"""Host side of the class-centre feature-distance loss: the float64 restatement (tests/featdis_ref.py) reproduces the reference's
own float32 runs of compute_dis_no_batch recorded in tests/golden/featdis_{a..f}.npz (written by
tests/golden/make_featdis_golden.py), the C ABI is declared, bound and exported, bad arguments are refused on the host, the
product refuses to run without a GPU, and the sizes the device tests rely on are those of the kernel's source."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_checks
import featdis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("acr_featdis_ws_bytes", "acr_featdis_fwd", "acr_featdis_bwd")
# The restatement agreed with the reference's fp32 run within 1.6e-7 on the loss and 1e-6 of the gradient's largest element on the
# cases it was first checked on; a factor of four for other seeds.
LOSS_BOUND = 4 * 1.6e-7
GRAD_BOUND = 4 * 1e-6


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_reproduces_the_reference(tag):
    z = np.load(os.path.join(GOLDEN, "featdis_%s.npz" % tag))
    B, K, C, h, w = R.CASES[tag]
    assert z["seg"].shape == (B, K, h, w) and z["feat"].shape == (B, C, h, w) and z["feat"].dtype == np.float32
    seg, feat = R.fixture_case(tag)
    assert np.array_equal(seg, z["seg"]) and np.array_equal(feat, z["feat"])          # the file is the seeded case
    loss, dis, pix, grad, labels, counts = R.loss_and_grad(z["seg"], z["feat"], torch.float64)
    err_l = abs(loss - float(z["loss"]))
    err_g = float(np.abs(grad - z["d_feat"]).max() / np.abs(grad).max())
    print("featdis_%s: loss %.9f (reference %.9f, apart %.2e), gradient apart %.2e of its largest element" % (tag, loss, float(z["loss"]), err_l, err_g))
    assert abs(loss - (dis + pix)) < 1e-15
    assert err_l <= LOSS_BOUND and err_g <= GRAD_BOUND
    assert labels.dtype == np.uint8 and np.array_equal(labels, z["labels"])
    assert counts.dtype == np.int64 and np.array_equal(counts, z["counts"])
    assert counts.sum() == B * h * w
    assert os.path.getsize(os.path.join(GOLDEN, "featdis_%s.npz" % tag)) < 100 * 1024


def test_fixture_cases_are_what_their_names_say():
    lab = {t: np.load(os.path.join(GOLDEN, "featdis_%s.npz" % t))["labels"] for t in R.CASES}
    assert (lab["c"] != 0).all() and (lab["d"] == 0).all()
    assert (lab["e"][0] != 0).all() and (lab["e"][1] == 0).any() and (lab["e"][1] != 0).any()
    assert sorted(np.unique(lab["f"]).tolist()) == [0, 5] and (lab["f"] == 5).sum() == 2
    for t in "ab":
        assert all((lab[t][b] == 0).any() and (lab[t][b] != 0).any() for b in range(2))
    # the three cases of `dis`: no background -> ff / 2 + 1; no foreground -> 0
    z = np.load(os.path.join(GOLDEN, "featdis_d.npz"))
    assert R.loss_and_grad(z["seg"], z["feat"], torch.float64)[1] == 0.0
    z = np.load(os.path.join(GOLDEN, "featdis_c.npz"))
    assert R.loss_and_grad(z["seg"], z["feat"], torch.float64)[1] > 1.0


def test_restatement_treats_a_zero_vector_as_torch_norm_does():
    """d|x|/dx := 0 at x = 0: the gradient at an all-zero pixel is c_k / (Z cnt' eps) -- of order 1 / eps -- and finite"""
    seg, feat = R.fixture_case("a")
    feat[0, :, 0, 0] = 0
    grad = R.loss_and_grad(seg, feat, torch.float64)[3]
    assert np.isfinite(grad).all() and np.abs(grad[0, :, 0, 0]).max() > 1e3 > np.abs(grad[1]).max()


def test_symbols_are_declared_bound_and_exported():
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import featdis
    abi_checks.check_bound(NAMES, L.SIGNATURES)
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert hasattr(lib, name)
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    make = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()
    assert "featdis.hip" in make
    src = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "featdis.hip")).read()
    assert int(re.search(r"#define FD_SLAB (\d+)", src).group(1)) == featdis.SLAB
    assert "#define FD_MAX_K ACR_FEATDIS_MAX_K\n" in src                          # the kernels' limit is the header's
    assert int(abi_checks.defined("ACR_FEATDIS_MAX_K")) == featdis.MAX_CLASSES == 128
    assert re.search(r"#define FD_MAX_C \(1 << (\d+)\)", src).group(1) == "20" and featdis.MAX_CHANNELS == 1 << 20


def test_device_test_shapes_cross_the_sizes_of_the_source():
    """test_featdis_gpu.py's shapes are tied to the kernel's #defines here: the slab case has more than one slab per image and a
    ragged last one, the K cases lie on both sides of the class-sum kernel's width threshold and of a wave's 64 lanes"""
    from acr_wsss_amd import featdis
    import test_featdis_gpu as G
    src = open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "featdis.hip")).read()
    wide = int(re.search(r"#define FD_WIDE_MAX_K (\d+)", src).group(1))
    B, K, C, h, w = G.SHAPES["slabs"]
    assert featdis.slab_pixels(K) == featdis.SLAB < h * w < 2 * featdis.SLAB and (h * w) % featdis.SLAB and (h * w) % 64
    ks = sorted(s[1] for s in G.SHAPES.values())
    assert ks[0] == 2 and any(64 < k <= wide for k in ks) and any(k > wide for k in ks) and ks[-1] <= featdis.MAX_CLASSES
    assert featdis.slab_pixels(32) == featdis.SLAB and featdis.slab_pixels(33) == 2 * featdis.SLAB and featdis.slab_pixels(128) == 4 * featdis.SLAB
    wide_dot = int(re.search(r"#define FD_WIDE_DOT_MIN_TILES (\d+)", src).group(1))
    tiles = {n: s[0] * -(-s[3] * s[4] // 256) for n, s in G.SHAPES.items()}
    assert wide_dot <= tiles["many"] < wide_dot + 8 and all(t < wide_dot for n, t in tiles.items() if n != "many")
    cs = sorted(s[2] for s in G.SHAPES.values())
    assert cs[0] == 1 and 257 in cs
    assert any(s[0] == 1 for s in G.SHAPES.values()) and any(s[3] * s[4] < 64 for s in G.SHAPES.values())


def test_ws_bytes_is_a_host_only_query():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    f = lib.acr_featdis_ws_bytes
    small, big = f(1, 2, 1, 1, 1), f(16, 21, 256, 224, 224)
    feat_bytes = 16 * 256 * 224 * 224 * 4
    assert 0 < small < big
    assert 16 * 25 * 21 * 256 * 8 <= big <= feat_bytes // 16            # the slab partials and the rest: a few percent of the input
    assert f(65535, 128, 1, 1, 1) > 0 and f(1, 128, 1 << 20, 1, 1) > 0 and f(4, 21, 1024, 56, 56) > 0
    for bad in ((0, 21, 8, 4, 4), (65536, 21, 8, 4, 4), (1, 1, 8, 4, 4), (1, 129, 8, 4, 4), (1, 21, 0, 4, 4), (1, 21, (1 << 20) + 1, 4, 4),
                (1, 21, 8, 0, 4), (1, 21, 8, 4, 0), (2, 21, 8, 1 << 15, 1 << 15), (1, 21, 8, 1 << 16, 1 << 15)):
        assert f(*bad) < 0, bad
        assert b"acr_featdis_ws_bytes" in lib.acr_last_error()


def test_argument_errors_return_minus_one_with_a_message():
    """every refusal happens on the host before anything is launched: no GPU is needed, the pointers are never followed"""
    from acr_wsss_amd import _lib as L
    lib = L.load()
    p = L.c_void_p(4096)                                 # non-null, aligned; never dereferenced
    odd = L.c_void_p(4104)
    need = lib.acr_featdis_ws_bytes(2, 21, 8, 4, 4)

    def fwd(seg=p, feat=p, B=2, K=21, C=8, h=4, w=4, ws=p, wsb=need, loss=p, labels=p, counts=p, pix=p, cst=p):
        return lib.acr_featdis_fwd(seg, feat, B, K, C, h, w, ws, wsb, loss, labels, counts, pix, cst, None)

    def bwd(feat=p, labels=p, pix=p, cst=p, g=p, B=2, K=21, C=8, h=4, w=4, dfeat=p):
        return lib.acr_featdis_bwd(feat, labels, pix, cst, g, B, K, C, h, w, dfeat, None)
    for kw in (dict(seg=None), dict(feat=None), dict(ws=None), dict(ws=odd), dict(wsb=need - 1), dict(loss=None), dict(labels=None),
               dict(counts=None), dict(pix=None), dict(pix=odd), dict(cst=None), dict(cst=odd), dict(B=0), dict(K=1), dict(K=129), dict(C=0),
               dict(h=0), dict(w=0), dict(h=1 << 15, w=1 << 15)):
        assert fwd(**kw) == -1, kw
        assert b"acr_featdis_fwd" in lib.acr_last_error(), kw
    for kw in (dict(feat=None), dict(labels=None), dict(pix=None), dict(pix=odd), dict(cst=None), dict(g=None), dict(dfeat=None), dict(B=0),
               dict(K=1), dict(K=129), dict(C=0), dict(h=0), dict(w=0)):
        assert bwd(**kw) == -1, kw
        assert b"acr_featdis_bwd" in lib.acr_last_error(), kw


def test_python_validates_before_it_asks_for_a_device():
    from acr_wsss_amd import featdis
    from acr_wsss_amd._lib import AcrHipError
    assert featdis.compute_dis_no_batch is featdis.feature_distance_loss
    seg, feat = torch.zeros(2, 21, 4, 5), torch.zeros(2, 8, 4, 5)
    bad = [(seg.numpy(), feat), (seg, None), (seg.double(), feat), (seg, feat.half()), (seg[0], feat), (seg, feat[0]),
           (seg[:, :1], feat), (torch.zeros(2, 129, 4, 5), feat), (seg, torch.zeros(1, 8, 4, 5)), (seg, torch.zeros(2, 8, 5, 4)),
           (torch.zeros(2, 21, 0, 5), torch.zeros(2, 8, 0, 5))]
    for s, f in bad:
        with pytest.raises(ValueError):
            featdis.feature_distance_loss(s, f)
    if not torch.cuda.is_available():
        with pytest.raises(AcrHipError):                 # good arguments: only now is the device asked for; there is no CPU path
            featdis.feature_distance_loss(seg, feat)


def test_the_steps_take_the_weight_as_a_keyword_that_defaults_to_off():
    from acr_wsss_amd import decoder, segtrain
    for fn in (segtrain.seg_train_step, segtrain.joint_train_step):
        par = inspect.signature(fn).parameters["dis_weight"]
        assert par.default == 0.0 and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(decoder.SegmentationHead.forward_features).parameters) == ["self", "x"]
