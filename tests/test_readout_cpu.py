"""The read-out heads of the plain ViT backbones off the GPU: the restatement tests/readout_ref.py against torch's float64
``Conv2d -> ConvTranspose2d`` autograd, the fixtures of tests/golden/make_decoder_vit_golden.py against the weight recipe, the
``seg=True`` layout of ``vitl`` against the reference's, and what the ``acr_reassemble_*`` entry points refuse on the host."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import abi_checks
import readout_ref as RR
from conftest import GOLDEN, load_golden
from recipe import recipe_tensor, weights_checksum

FIXTURES = {"decoder_vitb_64x96": "vitb", "decoder_distil_96x64": "deit_distilled"}


@pytest.mark.parametrize("start", [1, 2])
@pytest.mark.parametrize("s", [1, 2, 4])
def test_restatement_against_torch_float64(s, start):
    """matrix product + pixel shuffle against the convolutions themselves: the same sums of the same products, so the two agree to
    summation order (1e-12 of the maximum)"""
    rng = np.random.default_rng(10 * s + start)
    B, D, f, gh, gw = 2, 12, 5, 3, 4
    T = start + gh * gw
    conv1 = nn.Conv2d(D, f, 1).double()
    deconv = nn.ConvTranspose2d(f, f, s, stride=s).double() if s > 1 else None
    tok = torch.from_numpy(rng.standard_normal((B, T, D))).requires_grad_(True)
    x = tok[:, start:].transpose(1, 2).unflatten(2, (gh, gw))            # Slice, Transpose, Unflatten (DPT/vit.py:117-141)
    out = conv1(x) if deconv is None else deconv(conv1(x))
    dout = rng.standard_normal(tuple(out.shape))
    out.backward(torch.from_numpy(dout))
    p = lambda t: t.detach().numpy()
    got, cache = RR.readout_fwd(p(tok), p(conv1.weight), p(conv1.bias), None if deconv is None else p(deconv.weight),
                                None if deconv is None else p(deconv.bias), start, gh, gw)
    g = RR.readout_bwd(cache, dout)
    want = {"out": p(out), "tok": p(tok.grad), "w1": p(conv1.weight.grad), "b1": p(conv1.bias.grad)}
    have = {"out": got, "tok": g["tok"], "w1": g["w1"], "b1": g["b1"]}
    if deconv is not None:
        want.update(wt=p(deconv.weight.grad), bt=p(deconv.bias.grad))
        have.update(wt=g["wt"], bt=g["bt"])
    assert tuple(got.shape) == (B, f, gh * s, gw * s)
    for k in want:
        assert have[k].shape == want[k].shape, k
        assert np.abs(have[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    assert np.array_equal(g["tok"][:, :start], np.zeros((B, start, D)))          # the skipped tokens


def test_reassemble_keeps_float32_and_ignores_row_padding():
    rng = np.random.default_rng(3)
    B, start, gh, gw, C, s = 2, 1, 2, 3, 5, 2
    T = start + gh * gw
    y = rng.standard_normal((B * T, C * s * s + 3)).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    out = RR.reassemble(y, bias, B, T, start, gh, gw, C, s)
    assert out.dtype == np.float32
    for b, co, i, j, di, dj in [(0, 0, 0, 0, 0, 0), (1, 4, 1, 2, 1, 1), (1, 2, 0, 1, 1, 0)]:
        assert out[b, co, i * s + di, j * s + dj] == y[b * T + start + i * gw + j, (co * s + di) * s + dj] + bias[co]
    dy, db = RR.reassemble_bwd(out, B, T, start, gh, gw, C, s)
    assert dy.dtype == np.float32 and np.array_equal(dy.reshape(B, T, -1)[:, :start], np.zeros((B, start, C * s * s), np.float32))
    assert np.array_equal(dy.reshape(B, T, -1)[:, start:], (y[:, :C * s * s].reshape(B, T, C, s, s)
                                                            + bias.reshape(1, 1, C, 1, 1)).reshape(B, T, -1)[:, start:])


class _Lazy(dict):
    """key -> the recipe's tensor, made when asked for (weights_checksum touches a handful of keys)"""

    def __getitem__(self, k):
        return recipe_tensor(k, dict.__getitem__(self, k), 0)


@pytest.mark.parametrize("fname", sorted(FIXTURES))
def test_fixture_weights_are_the_recipe(fname):
    from acr_wsss_amd.DPT.ACR import ACR
    fx = load_golden(fname)
    h, w, batch, ncls, seed, features, stride = [int(v) for v in fx["meta"]]
    with torch.device("meta"):
        m = ACR(ncls, FIXTURES[fname], seg=True, features=features, use_pretrain=False)
    sd = m.state_dict()
    layout = _Lazy({k: tuple(v.shape) for k, v in sd.items() if "running_" not in k and torch.is_floating_point(v)})
    want = float(fx["weights_checksum"])
    assert abs(weights_checksum(layout) - want) < 1e-3 * want
    running = [k for k in sd if "running_" in k]
    assert running and all("before:" + k in fx and "after:" + k in fx for k in running)
    gh, gw = h // 16, w // 16
    for i, (c, up) in enumerate(zip((96, 192, 384, 768), (4, 2, 1, 0.5))):
        assert tuple(fx["layer_%d_shape" % (i + 1)]) == (batch, c, int(gh * up), int(gw * up))
        assert tuple(fx["layer_%d_rn_shape" % (i + 1)]) == (batch, features, int(gh * up), int(gw * up))
    assert tuple(fx["path_1_shape"]) == (batch, features, h // 2, w // 2) and gh != gw


def test_vitl_seg_true_layout_matches_the_reference():
    from acr_wsss_amd.DPT.ACR import ACR
    with open(os.path.join(GOLDEN, "state_dict_layout_seg_vitl.json")) as f:
        want = json.load(f)
    with torch.device("meta"):
        m = ACR(20, "vitl", seg=True, use_pretrain=False)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want)                               # the reference's key order too
    # the one exception test_model_gpu.py::test_plain_vit_backbones_train_step documents: the reference hard-wires
    # cls_head = Linear(768, C) (DPT/ACR.py:88), which cannot take vitl's 1024-wide tokens; here the head follows the encoder
    assert want.pop("cls_head.weight") == [20, 768] and got.pop("cls_head.weight") == [20, 1024]
    assert got == want
    assert got["pretrained.act_postprocess1.4.weight"] == [256, 256, 4, 4] and got["pretrained.act_postprocess4.4.weight"] == [1024, 1024, 3, 3]
    vit = m.pretrained.model
    assert (vit.tap1, vit.tap2, vit.tap3, vit.tap4) == (5, 11, 17, 23)


@pytest.mark.parametrize("name,hooks", [("vitb", (2, 5, 8, 11)), ("deit_distilled", (2, 5, 8, 11)), ("vitb_hybrid", (None, None, 8, 11))])
def test_hooks_follow_the_reference(name, hooks):
    from acr_wsss_amd.DPT.ACR import ACR
    with torch.device("meta"):
        vit = ACR(20, name, use_pretrain=False).pretrained.model
    assert (vit.tap1, vit.tap2, vit.tap3, vit.tap4) == hooks      # the hybrid's "1" and "2" are stem stages


def test_entry_points_are_declared_and_refuse_bad_arguments():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    for name, nargs in (("acr_reassemble_ws_bytes", 5), ("acr_reassemble_fwd", 12), ("acr_reassemble_bwd", 14)):
        assert len(abi_checks.declared(name)[1]) == len(L.SIGNATURES[name][1]) == nargs and getattr(lib, name) is not None
    p = ctypes.c_void_p(64)                                      # never dereferenced: the arguments are refused first

    def fwd(B=2, T=7, start=1, gh=2, gw=3, C=5, s=2, ldy=None):
        return lib.acr_reassemble_fwd(p, C * s * s if ldy is None else ldy, p, B, T, start, gh, gw, C, s, p, None)

    def bwd(B=2, T=7, start=1, gh=2, gw=3, C=5, s=2, lddy=None, ws=None, ws_bytes=0, dbias=None):
        return lib.acr_reassemble_bwd(p, B, T, start, gh, gw, C, s, p, C * s * s if lddy is None else lddy, dbias, ws, ws_bytes, None)

    for call, kw, word in ((fwd, dict(s=3), "s must be"), (bwd, dict(s=3), "s must be"), (fwd, dict(s=0), "s must be"),
                           (fwd, dict(T=8), "start + gh * gw"), (bwd, dict(T=6), "start + gh * gw"),
                           (fwd, dict(ldy=19), "ldy"), (bwd, dict(lddy=19), "lddy"),
                           (fwd, dict(start=9, T=15), "start"), (bwd, dict(start=-1, T=5), "start"),
                           (fwd, dict(C=0), "bad shape"), (bwd, dict(gh=0, T=1), "bad shape"), (fwd, dict(B=0), "bad shape"),
                           (bwd, dict(dbias=p), "workspace"), (bwd, dict(dbias=p, ws=p, ws_bytes=4), "workspace")):
        assert call(**kw) == -1 and word in lib.acr_last_error().decode(), (kw, lib.acr_last_error().decode())
    assert lib.acr_reassemble_ws_bytes(2, 2, 3, 5, 3) == 0 and lib.acr_reassemble_ws_bytes(0, 2, 3, 5, 2) == 0
    # one fp32 partial per (sample, grid row, 32-column tile, channel); s = 1 runs as one row of gh * gw positions in tiles of 64
    assert lib.acr_reassemble_ws_bytes(2, 2, 3, 5, 2) == 4 * 2 * 2 * 1 * 5
    assert lib.acr_reassemble_ws_bytes(16, 24, 24, 96, 4) == 4 * 16 * 24 * 1 * 96
    assert lib.acr_reassemble_ws_bytes(3, 10, 13, 7, 1) == 4 * 3 * 1 * 3 * 7


def test_cpu_tensors_and_bad_arguments_raise():
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd._lib import AcrHipError
    with pytest.raises(AcrHipError):
        D.reassemble(torch.zeros(14, 20), None, 2, 7, 1, 2, 3, 5, 2)
    with pytest.raises(AcrHipError):
        D.readout(torch.zeros(2, 7, 32), 1, 2, 3, nn.Conv2d(32, 32, 1), None)
    with pytest.raises(ValueError):
        D.reassemble(np.zeros((14, 20), np.float32), None, 2, 7, 1, 2, 3, 5, 2)
    with pytest.raises(ValueError):
        D.readout([[0.0]], 1, 2, 3, nn.Conv2d(32, 32, 1), None)
