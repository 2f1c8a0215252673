"""The read-out heads of the plain ViT backbones on the device: csrc/reassemble.hip behind ``acr_reassemble_fwd`` / ``_bwd``,
``decoder.reassemble`` / ``decoder.readout`` and ``decoder.layers_rn`` for vitb and the distilled DeiT.

Kernel level: forward and backward are copies plus one fp32 add, so they must equal the numpy restatement (tests/readout_ref.py,
pinned to torch's float64 convolutions by test_readout_cpu.py) computed in fp32 from the same values BIT FOR BIT; the skipped rows of
the gradient are exactly 0 and the row padding keeps the value the test put there.  The bias gradient is a sum: the rule of
test_decoder_gpu.py ``compare`` -- the device's error against float64 at most 2x the error of torch's own fp32 sum on the same case,
floor 4 fp32 ulps of the largest value -- and bit-identical over two runs.
Model level: the bounds test_decoder_gpu.py::test_decode_against_the_reference_fixture uses for reference fixtures, 2e-4 of the
maximum for activations (and the running statistics after the pass) and 2e-3 for gradients; the fixtures are the reference's own
results (tests/golden/make_decoder_vit_golden.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import decoder_ref as R
import readout_ref as RR
from conftest import load_golden
from kernel_checks import Cmp
from recipe import make_inputs, recipe_tensor
from test_decoder_gpu import compare

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 12345.0
# (B, start, gh, gw, C, s, row padding): the smallest legal call; odd everything, two skipped tokens; tap-1 channels with padded rows;
# the pure transpose with C off any tile; start = 0; one sample at the 384^2 production geometry (3.5 MB)
KERNEL_CASES = [(1, 1, 1, 1, 1, 1, 0), (2, 2, 3, 5, 7, 4, 0), (2, 1, 5, 3, 96, 2, 8), (1, 2, 4, 6, 33, 1, 0), (3, 0, 2, 9, 40, 4, 0),
                (1, 1, 24, 24, 96, 4, 0)]
FIXTURES = {"decoder_vitb_64x96": "vitb", "decoder_distil_96x64": "deit_distilled"}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


# ------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_case(case):
    """inputs (fp32 numpy), the fp32 restatement and torch's CPU fp32 bias-gradient sum of one case; treat as read-only"""
    B, start, gh, gw, C, s, pad = case
    T = start + gh * gw
    rng = np.random.default_rng(sum(case) + 31 * C)
    y = rng.standard_normal((B * T, C * s * s + pad)).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    dout = rng.standard_normal((B, C, gh * s, gw * s)).astype(np.float32)
    dy, db64 = RR.reassemble_bwd(dout, B, T, start, gh, gw, C, s)
    return dict(T=T, y=y, bias=bias, dout=dout, out=RR.reassemble(y, bias, B, T, start, gh, gw, C, s),
                out_nobias=RR.reassemble(y, None, B, T, start, gh, gw, C, s), dy=dy, db64=db64,
                db_torch=torch.from_numpy(dout).sum(dim=(0, 2, 3)))


def device_bwd(case, k):
    """acr_reassemble_bwd through the C ABI into a poisoned (B T, C s^2 + pad) buffer -> (dy buffer, dbias) on the host"""
    from acr_wsss_amd import _lib as L
    B, start, gh, gw, C, s, pad = case
    lib = L.load()
    dout = torch.from_numpy(k["dout"]).to(DEV)
    buf = torch.full((B * k["T"], C * s * s + pad), POISON, dtype=torch.float32, device=DEV)
    dbias = torch.full((C,), POISON, dtype=torch.float32, device=DEV)
    nbytes = lib.acr_reassemble_ws_bytes(B, gh, gw, C, s)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    L.check(lib.acr_reassemble_bwd(L.ptr(dout), B, k["T"], start, gh, gw, C, s, L.ptr(buf), buf.stride(0), L.ptr(dbias), L.ptr(ws), nbytes,
                                   L.stream_ptr()), "acr_reassemble_bwd")
    return buf.cpu().numpy(), dbias.cpu()


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_reassemble_kernels(case):
    from acr_wsss_amd import decoder as D
    B, start, gh, gw, C, s, pad = case
    k = kernel_case(case)
    T, n = k["T"], C * s * s
    # forward: the padded rows travel as a strided view (ldy = C s^2 + pad)
    yd = torch.from_numpy(k["y"]).to(DEV)
    out = D.reassemble(yd[:, :n], torch.from_numpy(k["bias"]).to(DEV), B, T, start, gh, gw, C, s)
    assert tuple(out.shape) == (B, C, gh * s, gw * s) and out.is_contiguous()
    assert out.cpu().numpy().tobytes() == k["out"].tobytes()
    assert D.reassemble(yd[:, :n], None, B, T, start, gh, gw, C, s).cpu().numpy().tobytes() == k["out_nobias"].tobytes()
    # backward
    buf, dbias = device_bwd(case, k)
    assert buf[:, :n].tobytes() == k["dy"].tobytes()
    assert np.array_equal(buf.reshape(B, T, -1)[:, :start, :n], np.zeros((B, start, n), np.float32))
    assert np.array_equal(buf[:, n:], np.full((B * T, pad), POISON, np.float32))
    cmp = Cmp()
    cmp.where = "reassemble %s" % (case,)
    compare(cmp, "dbias", dbias, k["db_torch"], k["db64"])
    assert not cmp.failures, "\n".join(cmp.failures)
    buf2, dbias2 = device_bwd(case, k)
    assert dbias2.numpy().tobytes() == dbias.numpy().tobytes() and buf2.tobytes() == buf.tobytes()
    # and through autograd: the same bits, the bias gradient included
    yl = yd[:, :n].clone().requires_grad_(True)
    bl = torch.from_numpy(k["bias"]).to(DEV).requires_grad_(True)
    D.reassemble(yl, bl, B, T, start, gh, gw, C, s).backward(torch.from_numpy(k["dout"]).to(DEV))
    assert yl.grad.cpu().numpy().tobytes() == k["dy"].tobytes() and bl.grad.cpu().numpy().tobytes() == dbias.numpy().tobytes()


def test_reassemble_without_a_bias_gradient_needs_no_workspace():
    from acr_wsss_amd import _lib as L
    case = KERNEL_CASES[1]
    B, start, gh, gw, C, s, pad = case
    k = kernel_case(case)
    dout = torch.from_numpy(k["dout"]).to(DEV)
    dy = torch.empty((B * k["T"], C * s * s), dtype=torch.float32, device=DEV)
    L.check(L.load().acr_reassemble_bwd(L.ptr(dout), B, k["T"], start, gh, gw, C, s, L.ptr(dy), dy.stride(0), None, None, 0, L.stream_ptr()),
            "acr_reassemble_bwd")
    assert dy.cpu().numpy().tobytes() == k["dy"].tobytes()


# ------------------------------------------------------------------------------------------------
# readout against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["f32", "f32_split"])
@pytest.mark.parametrize("tap", [1, 2, 3])
@pytest.mark.parametrize("fname", sorted(FIXTURES))
def test_readout_forward_and_gradients(fname, tap, math):
    """at the fixture's tap shapes (vitb: start 1, a 4 x 6 grid; distilled: start 2, 6 x 4), weights by the recipe"""
    from acr_wsss_amd import _lib as L
    from acr_wsss_amd import decoder as D
    fx = load_golden(fname)
    h, w = int(fx["meta"][0]), int(fx["meta"][1])
    gh, gw, start = h // 16, w // 16, 2 if "distil" in fname else 1
    Dm, f, s = 768, (96, 192, 384)[tap - 1], (4, 2, 1)[tap - 1]
    key = "pretrained.act_postprocess%d." % tap
    conv1 = nn.Conv2d(Dm, f, 1)
    deconv = nn.ConvTranspose2d(f, f, s, stride=s) if s > 1 else None
    with torch.no_grad():
        for m, idx in ((conv1, 3), (deconv, 4)):
            if m is not None:
                m.weight.copy_(recipe_tensor(key + "%d.weight" % idx, m.weight.shape, 0))
                m.bias.copy_(recipe_tensor(key + "%d.bias" % idx, m.bias.shape, 0))
    g = torch.Generator().manual_seed(70 + tap)
    tok = torch.randn(2, start + gh * gw, Dm, generator=g)
    p = lambda t: None if t is None else t.detach().numpy()
    ref, cache = RR.readout_fwd(p(tok), p(conv1.weight), p(conv1.bias), p(deconv.weight) if deconv else None,
                                p(deconv.bias) if deconv else None, start, gh, gw)
    dout = torch.randn(ref.shape, generator=g)
    gref = RR.readout_bwd(cache, dout.numpy())
    conv1 = conv1.to(DEV)
    deconv = deconv.to(DEV) if deconv else None
    td = tok.to(DEV).requires_grad_(True)
    out = D.readout(td, start, gh, gw, conv1, deconv, L.MATH[math])
    out.backward(dout.to(DEV))
    assert tuple(out.shape) == (2, f, gh * s, gw * s)
    worst = {"out": _rel(out.detach().cpu().numpy(), ref)}
    assert worst["out"] <= 2e-4, worst
    got = {"tok": td.grad, "w1": conv1.weight.grad, "b1": conv1.bias.grad}
    if deconv is not None:
        got.update(wt=deconv.weight.grad, bt=deconv.bias.grad)
    assert set(got) == set(gref)
    for name, t in got.items():
        worst[name] = _rel(t.cpu().numpy(), gref[name])
        assert worst[name] <= 2e-3, (name, worst)
    assert torch.equal(td.grad[:, :start], torch.zeros_like(td.grad[:, :start]))
    print("readout %s tap %d %s: %s" % (fname, tap, math, {k: "%.2e" % v for k, v in worst.items()}))


def test_readout_refuses_what_it_is_not_built_for():
    from acr_wsss_amd import decoder as D
    tok = torch.zeros(2, 7, 64, device=DEV)
    conv1 = nn.Conv2d(64, 32, 1).to(DEV)
    with pytest.raises(ValueError):
        D.readout(tok, 2, 2, 3, conv1, None)                    # 7 tokens are not 2 + 2 x 3
    with pytest.raises(ValueError):
        D.readout(tok, 1, 2, 3, nn.Conv2d(64, 32, 3, padding=1).to(DEV), None)
    with pytest.raises(NotImplementedError):
        D.readout(tok, 1, 2, 3, conv1, nn.ConvTranspose2d(32, 32, 3, stride=3).to(DEV))
    with pytest.raises(NotImplementedError):
        D.readout(tok, 1, 2, 3, conv1, nn.ConvTranspose2d(32, 32, 4, stride=2, padding=1).to(DEV))
    with pytest.raises(ValueError):
        D.reassemble(torch.zeros(14, 20, device=DEV), None, 2, 7, 1, 2, 3, 5, 3)
    with pytest.raises(ValueError):
        D.reassemble(torch.zeros(14, 21, device=DEV), None, 2, 7, 1, 2, 3, 5, 2)
    assert tuple(D.readout(tok, 1, 2, 3, conv1, None, 2).shape) == (2, 32, 2, 3)       # fp16x2 runs as exact fp32 here


# ------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vit_model(fname):
    """the model built the way test_decoder_gpu.py's seg_model builds the hybrid one: weights by the recipe, running statistics from
    the fixture"""
    from acr_wsss_amd.DPT.ACR import ACR
    fx = load_golden(fname)
    m = ACR(int(fx["meta"][3]), FIXTURES[fname], seg=True, features=int(fx["meta"][5]), use_pretrain=False)
    sd = {}
    for k, v in m.state_dict().items():
        if "running_" in k:
            sd[k] = torch.from_numpy(fx["before:" + k])
        elif torch.is_floating_point(v):
            sd[k] = recipe_tensor(k, v.shape, 0)
        else:
            sd[k] = torch.zeros_like(v)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), fx, {k: v for k, v in sd.items() if "running_" in k or k.endswith("num_batches_tracked")}


def _reset(m, sd):
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k in sd:
                v.copy_(sd[k])


def _image(fx):
    h, w, batch, ncls, seed = [int(v) for v in fx["meta"][:5]]
    return make_inputs(batch, max(h, w), ncls, seed)[0][:, :, :h, :w].contiguous()


@pytest.mark.parametrize("math", ["f32", "f32_split"])
@pytest.mark.parametrize("fname", sorted(FIXTURES))
def test_decode_against_the_reference_fixture(fname, math):
    from acr_wsss_amd import decoder as D
    m, fx, sd = vit_model(fname)
    _reset(m, sd)
    m.set_math(math).train()
    h, w, batch = [int(v) for v in fx["meta"][:3]]
    features, stride = int(fx["meta"][5]), int(fx["meta"][6])
    img = _image(fx).to(DEV)
    with torch.no_grad():
        rn = D.layers_rn(m, img)
        path_1 = D.fuse(m, *rn)
        # forward_vit's own four maps, from the tokens that pass recorded
        taps, pp, vit = m.pretrained.activations, m.pretrained, m.pretrained.model
        assert sorted(taps) == ["1", "2", "3", "4"]
        geo = (vit.num_tokens, h // 16, w // 16)
        maps = [D.readout(taps["1"], *geo, pp.act_postprocess1[3], pp.act_postprocess1[4], vit.acr_math),
                D.readout(taps["2"], *geo, pp.act_postprocess2[3], pp.act_postprocess2[4], vit.acr_math),
                D.readout(taps["3"], *geo, pp.act_postprocess3[3], None, vit.acr_math),
                D.conv(pp.act_postprocess4[4], D.readout(taps["4"], *geo, pp.act_postprocess4[3], None, vit.acr_math), vit.acr_math)]
    for i, (t, mp) in enumerate(zip(rn, maps)):
        assert tuple(mp.shape) == tuple(fx["layer_%d_shape" % (i + 1)]) and tuple(t.shape) == tuple(fx["layer_%d_rn_shape" % (i + 1)])
        rm = _rel(R.sample(mp.cpu().numpy(), stride), fx["layer_%d" % (i + 1)])
        r = _rel(R.sample(t.cpu().numpy(), stride), fx["layer_%d_rn" % (i + 1)])
        print("decode %s %s layer_%d %.2e layer_%d_rn %.2e" % (fname, math, i + 1, rm, i + 1, r))
        assert rm <= 2e-4 and r <= 2e-4, (i, rm, r)
    r = _rel(R.sample(path_1.cpu().numpy(), stride), fx["path_1"])
    print("decode %s %s path_1 %.2e" % (fname, math, r))
    assert tuple(path_1.shape) == (batch, features, h // 2, w // 2) and r <= 2e-4, r
    for k, v in m.state_dict().items():
        if "running_" in k:
            assert _rel(v.cpu().numpy(), fx["after:" + k]) <= 2e-4, k
    m.set_math("f32")


def test_head_loss_and_backward_end_to_end_repeat_bit_for_bit():
    """SegmentationHead(decode(vitb model, x)) into segloss.split_cross_entropy, then backward(): all 14 read-out tensors and every
    parameter of the ViT blocks (all lie below tap 4) receive a finite, non-zero gradient, and the whole thing repeats bit for bit"""
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd import segloss as S
    from acr_wsss_amd.backbone import set_math
    m, fx, sd = vit_model("decoder_vitb_64x96")
    m.set_math("f32_split").train()
    torch.manual_seed(5)
    head = D.SegmentationHead(16, 20).to(DEV).train()
    set_math(head, "f32_split")
    img = _image(fx).to(DEV)
    rng = np.random.default_rng(44)
    label = rng.integers(0, 21, (2, 64, 96)).astype(np.uint8)
    label[rng.random(label.shape) < 0.1] = 255
    runs = []
    for _ in range(2):
        _reset(m, sd)
        m.zero_grad()
        head.zero_grad()
        torch.manual_seed(6)                                 # the head's Dropout
        logits = head(D.decode(m, img))
        assert tuple(logits.shape) == (2, 21, 64, 96)
        ce, bg, fg = S.split_cross_entropy(logits, label)
        ce.backward()
        named = dict(m.named_parameters())
        readouts = [k for k in named if k.startswith("pretrained.act_postprocess")]
        blocks = [k for k in named if k.startswith("pretrained.model.blocks.")]
        assert len(readouts) == 14 and len(blocks) == 12 * 12
        grads = {k: named[k].grad for k in readouts + blocks + [k for k in named if k.startswith("scratch.layer")]}
        grads.update({"head." + k: p.grad for k, p in head.named_parameters()})
        for k, g in grads.items():
            assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, k
        runs.append((ce.detach().cpu(), {k: g.cpu().clone() for k, g in grads.items()}))
    assert torch.isfinite(runs[0][0]) and runs[0][0].numpy().tobytes() == runs[1][0].numpy().tobytes()
    for k in runs[0][1]:
        assert runs[0][1][k].numpy().tobytes() == runs[1][1][k].numpy().tobytes(), k
    m.set_math("f32")
    m.zero_grad(set_to_none=True)


def test_seg_train_step_on_the_distilled_deit():
    """one segtrain.seg_train_step at 96 x 64: a finite loss, and the read-out parameters move"""
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd.backbone import set_math
    from acr_wsss_amd.segtrain import seg_train_step
    from acr_wsss_amd.train import PolyOptimizer
    m, fx, sd = vit_model("decoder_distil_96x64")
    _reset(m, sd)
    m.set_math("f32_split").train()
    torch.manual_seed(5)
    head = D.SegmentationHead(16, 20).to(DEV).train()
    set_math(head, "f32_split")
    keep = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(45)
    label = rng.integers(0, 21, (2, 96, 64)).astype(np.uint8)
    label[rng.random(label.shape) < 0.1] = 255
    params = list(m.parameters()) + list(head.parameters())
    opt = PolyOptimizer(params, lr=1e-2, weight_decay=5e-4, max_step=100)
    try:
        loss, terms = seg_train_step(m, head, opt, _image(fx).to(DEV), None, None, torch.from_numpy(label).to(DEV), None)
        assert torch.isfinite(loss) and float(terms["dloss"]) == 0.0
        moved = [k for k, v in m.state_dict().items() if k.startswith("pretrained.act_postprocess") and not torch.equal(v, keep[k])]
        assert len(moved) == 14, moved
        assert all(torch.isfinite(v).all() for v in m.state_dict().values())
    finally:                                                # the model is shared with the fixture tests: put the weights back
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(keep[k])
        m.invalidate_caches()
        m.zero_grad(set_to_none=True)
        m.set_math("f32")
