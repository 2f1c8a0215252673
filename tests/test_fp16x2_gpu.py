"""The opt-in fp16x2 arithmetic (math = ACR_MATH_FP16X2, model mode "f32_fp16x2"): block Linears as three fp16-MFMA terms of a
scaled two-piece operand split (include/acr_hip.h acr_math).  Split pass against its documented bound, the products against the
exact-fp32 kernel's own error, the Linears against fp64, the parts of the model the mode must not touch, model parity."""
import numpy as np
import pytest
import torch

import kernel_checks as KC
from conftest import load_golden, recipe_sd
from recipe import make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, FLOOR = 2.0 ** -22, 2.0 ** -39          # ACR_FP16X2_REL / ACR_FP16X2_FLOOR


def _lib():
    from acr_wsss_amd import _lib as L
    return L, L.load()


def _h2_image(x, how):
    """fp16x2 image of x (how = "rows" | "cols") or of x^T ("t") through the C ABI; returns (image, colsum or None)."""
    L, lib = _lib()
    rows, cols = x.shape
    ir, ic = (cols, rows) if how == "t" else (rows, cols)
    img = torch.empty(lib.acr_h2_image_floats(ir, ic), dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.acr_h2_ws_floats(rows, cols), dtype=torch.float32, device=x.device)
    cs = torch.empty(cols, dtype=torch.float32, device=x.device) if how != "t" else None
    if how == "rows":
        L.check(lib.acr_h2_image(L.ptr(x), x.stride(0), rows, cols, L.ptr(img), L.ptr(cs), L.ptr(ws), L.stream_ptr()), "acr_h2_image")
    elif how == "cols":
        L.check(lib.acr_h2_image_cols(L.ptr(x), x.stride(0), rows, cols, L.ptr(img), L.ptr(cs), L.ptr(ws), L.stream_ptr()), "acr_h2_image_cols")
    else:
        L.check(lib.acr_h2_image_t(L.ptr(x), x.stride(0), rows, cols, L.ptr(img), L.ptr(ws), L.stream_ptr()), "acr_h2_image_t")
    return img, cs


def _decode(img, rows, cols):
    """(value represented by the planes, exponents, direction flag) of an fp16x2 image of a rows x cols matrix."""
    nrb, nkb = (rows + 127) // 128, (cols + 15) // 16
    nexp = max(nrb, (cols + 127) // 128) * 128
    raw = img.cpu().numpy()
    npl = nrb * nkb * 2048
    p = raw[:npl].view(np.float16).reshape(nrb, nkb, 2, 128, 2, 8).astype(np.float64)
    rr = np.arange(128)
    # stored half = contraction half ^ bit 3 of the row
    sw = np.stack([p[:, :, :, rr, (kh ^ ((rr >> 3) & 1)), :] for kh in range(2)], axis=4)      # (nrb, nkb, 2, 128, kh, 8)
    v = sw.sum(axis=2).transpose(0, 2, 1, 3, 4).reshape(nrb * 128, nkb * 16)[:rows, :cols]
    ex = raw[npl:npl + nexp].view(np.int32)
    flag = int(raw[npl + nexp:npl + nexp + 1].view(np.int32)[0])
    return v, ex, flag


def _rows_case(kind, R, C, g):
    x = torch.randn(R, C, generator=g)
    if kind == "wide":
        x = x * torch.exp2(torch.randint(-40, 41, (R, C), generator=g).float())
    elif kind == "zero":
        x[::3] = 0.0
    elif kind == "subnormal":
        x[1::2] = x[1::2] * 2.0 ** -140                     # fp32-subnormal rows
    return x


@pytest.mark.parametrize("kind", ["random", "wide", "zero", "subnormal"])
@pytest.mark.parametrize("how", ["rows", "cols", "t"])
def test_split_pass_meets_the_documented_bound(kind, how):
    g = torch.Generator(device="cpu").manual_seed(7)
    R, C = 300, 200
    x = _rows_case(kind, R, C, g)
    if how == "cols":
        x = x.t().contiguous()                              # the group is a column: make the special groups columns
    xd = x.to(DEV)
    img, cs = _h2_image(xd, how)
    torch.cuda.synchronize()
    xn = x.double().numpy()
    if how == "t":
        xn = xn.T
    r, c = xn.shape
    v, ex, flag = _decode(img, r, c)
    assert flag == (1 if how == "cols" else 0)
    scaled_axis = 0 if how == "cols" else 1                 # reduce over this axis for the group maximum
    gmax = np.abs(xn).max(axis=scaled_axis, keepdims=True)
    e = ex[:c] if how == "cols" else ex[:r]
    assert (e[gmax.reshape(-1) == 0] == 0).all()
    nz = gmax.reshape(-1) > 0
    m_scaled = np.ldexp(gmax.reshape(-1)[nz], e[nz])
    assert ((m_scaled >= 2.0 ** 14) & (m_scaled < 2.0 ** 15)).all()
    dec = np.ldexp(v, -(e.reshape(1, -1) if how == "cols" else e.reshape(-1, 1)))
    err = np.abs(xn - dec)
    assert (err <= REL * np.abs(xn) + FLOOR * gmax).all(), float((err - REL * np.abs(xn) - FLOOR * gmax).max())
    if cs is not None:
        assert (np.abs(cs.cpu().numpy() - xn.sum(0)) <= 1e-5 * np.abs(xn).sum(0)).all()


def _gemm3(mode, a, b, shape):
    """(exact-fp32 result, fp16x2 result, fp64 reference, sum_k |a||b|) of acr_gemm_f32 under math 0 and math 2."""
    from acr_wsss_amd import ops
    outs = []
    for math in (0, 2):
        c = torch.empty(shape, dtype=torch.float32, device=a.device)
        ops.gemm_f32_raw(mode, a, b, c, math=math)
        outs.append(c.double())
    ad, bd = a.double(), b.double()
    if mode == "nt":
        ref, scale = ad @ bd.t(), ad.abs() @ bd.abs().t()
    elif mode == "nn":
        ref, scale = ad @ bd, ad.abs() @ bd.abs()
    else:
        ref, scale = ad.t() @ bd, ad.abs().t() @ bd.abs()
    return outs[0], outs[1], ref, scale


def _operands(mode, case, M, N, K, g):
    am, bm = ((M, K), (N, K)) if mode == "nt" else (((M, K), (K, N)) if mode == "nn" else ((K, M), (K, N)))
    ka, kb = (1 if mode in ("nt", "nn") else 0), (1 if mode == "nt" else 0)
    a, b = torch.randn(am, generator=g), torch.randn(bm, generator=g)
    if case == "range":
        a = a * torch.exp2(torch.randint(-40, 41, am, generator=g).float())
        b = b * torch.exp2(torch.randint(-20, 21, bm, generator=g).float())
    elif case == "cancel":
        h = K // 2
        ia, ib = [slice(None)] * 2, [slice(None)] * 2
        ia2, ib2 = list(ia), list(ib)
        ia[ka], ia2[ka], ib[kb], ib2[kb] = slice(0, h), slice(h, K), slice(0, h), slice(h, K)
        a[tuple(ia2)] = a[tuple(ia)]
        b[tuple(ib2)] = -b[tuple(ib)] * (1 + 1e-6 * torch.randn(b[tuple(ib)].shape, generator=g))
    elif case == "underflow":
        a = a * 2.0 ** -112
    return a, b, ka, kb


def _floor_term(a, b, ka, kb, scale):
    """FLOOR per operand element, carried through the product and normalised as the errors are."""
    if ka == 1:                                              # a rows are the groups (nt / nn)
        amax = a.double().abs().amax(1).reshape(-1, 1)
    else:                                                    # tn: a columns
        amax = a.double().abs().amax(0).reshape(-1, 1)
    if kb == 1:                                              # nt: b rows
        bmax = b.double().abs().amax(1).reshape(1, -1)
        bsum = b.double().abs().sum(1).reshape(1, -1)
    else:                                                    # nn: groups = columns of b (rows of b^T); tn: columns of b
        bmax = b.double().abs().amax(0).reshape(1, -1)
        bsum = b.double().abs().sum(0).reshape(1, -1)
    asum = a.double().abs().sum(ka).reshape(-1, 1)
    return FLOOR * (amax * bsum + bmax * asum) / scale


@pytest.mark.parametrize("mode", ["nt", "nn", "tn"])
@pytest.mark.parametrize("case", ["plain", "range", "cancel", "underflow"])
def test_fp16x2_adversarial_operands(mode, case):
    g = torch.Generator(device="cpu").manual_seed(13)
    M, N, K = 384, 256, 768
    a, b, ka, kb = _operands(mode, case, M, N, K, g)
    a, b = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    exact, h2, ref, scale = _gemm3(mode, a, b, (M, N))
    assert torch.isfinite(exact).all() and torch.isfinite(h2).all()
    e_exact, e_h2 = (exact - ref).abs() / scale, (h2 - ref).abs() / scale
    floor = float(_floor_term(a, b, ka, kb, scale).max())
    print("%s/%s: max normalised error exact %.3e fp16x2 %.3e; rms exact %.3e fp16x2 %.3e (floor %.1e)" % (
        mode, case, float(e_exact.max()), float(e_h2.max()), float(e_exact.pow(2).mean().sqrt()), float(e_h2.pow(2).mean().sqrt()), floor))
    assert float(e_h2.max()) <= 2 * float(e_exact.max()) + floor
    assert float(e_h2.pow(2).mean().sqrt()) <= 2 * float(e_exact.pow(2).mean().sqrt()) + floor


@pytest.mark.parametrize("mode", ["nt", "tn"])
def test_quiet_row_or_column_keeps_its_accuracy(mode):
    """One token row (NT) / one feature column (TN) at 2^-30 of the tensor maximum: a per-tensor scale would push it into fp16's
    subnormals; the per-group scale keeps its normalised error within 2x the exact kernel's."""
    g = torch.Generator(device="cpu").manual_seed(17)
    M, N, K = 256, 256, 512
    if mode == "nt":
        a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
        a[5] *= 2.0 ** -30
    else:
        a, b = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
        a[:, 5] *= 2.0 ** -30
    exact, h2, ref, scale = _gemm3(mode, a.to(DEV), b.to(DEV), (M, N))
    e_exact, e_h2 = ((exact - ref).abs() / scale)[5], ((h2 - ref).abs() / scale)[5]
    assert float(e_h2.max()) <= 2 * float(e_exact.max()), (float(e_h2.max()), float(e_exact.max()))


def test_fp16x2_propagates_non_finite_values():
    g = torch.Generator(device="cpu").manual_seed(5)
    M, N, K = 256, 128, 256
    a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    a[3, 17], a[40, 200], a[77, 5] = float("inf"), float("nan"), float("-inf")
    b[9, 100] = float("nan")
    exact, h2, ref, _ = _gemm3("nt", a.to(DEV), b.to(DEV), (M, N))
    bad = ~torch.isfinite(ref)
    assert (~torch.isfinite(h2))[bad].all()
    assert torch.isnan(h2[40]).all() and torch.isnan(h2[:, 9]).all()
    ok = ~bad
    assert torch.isfinite(h2[ok]).all()
    assert float((h2[ok] - ref[ok]).abs().max()) <= 2 * float((exact[ok] - ref[ok]).abs().max()) + 1e-6


def test_gemm_h2_refuses_a_mismatched_scale_direction():
    L, lib = _lib()
    g = torch.Generator(device="cpu").manual_seed(3)
    M, N, K = 256, 128, 192
    a, b = torch.randn(M, K, generator=g).to(DEV), torch.randn(N, K, generator=g).to(DEV)
    ai, _ = _h2_image(a, "rows")
    bi, _ = _h2_image(b, "rows")
    bc, _ = _h2_image(b, "cols")
    ws = torch.empty(max(1, lib.acr_gemm_h2_ws_floats(0, 0, M, N, K)), dtype=torch.float32, device=DEV)
    c = torch.empty(M, N, dtype=torch.float32, device=DEV)
    assert lib.acr_gemm_h2(0, 0, L.ptr(ai), L.ptr(bi), None, None, 0, L.ptr(c), N, None, M, N, K, L.ptr(ws), L.stream_ptr()) == 0
    ref = a.double() @ b.double().t()
    assert float((c.double() - ref).abs().max() / (a.double().abs() @ b.double().abs().t()).max()) < 1e-6
    assert lib.acr_gemm_h2(0, 0, L.ptr(ai), L.ptr(bc), None, None, 0, L.ptr(c), N, None, M, N, K, L.ptr(ws), L.stream_ptr()) == -1
    assert lib.acr_conv1x1_f32(2, L.ptr(a), 0, L.ptr(a), None, L.ptr(c), 1, 4, 4, 4, None, L.stream_ptr()) == -3


@pytest.mark.parametrize("M,K,N", [(394, 192, 576), (785, 768, 768), (131, 128, 260)])
def test_linear_f32_fp16x2_against_fp64(M, K, N):
    from acr_wsss_amd import ops
    g = torch.Generator(device="cpu").manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV).requires_grad_(True)
    b = torch.randn(N, generator=g).to(DEV).requires_grad_(True)
    r = torch.randn(M, N, generator=g).to(DEV).requires_grad_(True)
    y = ops.LinearF32Fn.apply(x, w, b, r, None, 2)
    dy = torch.randn(M, N, generator=g).to(DEV)
    (y * dy).sum().backward()
    cmp = KC.Cmp()
    KC.verify_linear(cmp, x, w, b, r, y, dy, KC.grads_of(x, w, b, r))
    assert not cmp.failures, "\n".join(cmp.failures)
    first = (y.detach().clone(), x.grad.clone(), w.grad.clone(), b.grad.clone())
    x.grad = w.grad = b.grad = None
    y2 = ops.LinearF32Fn.apply(x, w, b, r, None, 2)
    (y2 * dy).sum().backward()
    assert all(torch.equal(u, v) for u, v in zip(first, (y2, x.grad, w.grad, b.grad)))


@pytest.mark.parametrize("M,D,Hd", [(197 * 2, 192, 768), (785, 768, 3072), (131, 128, 260)])
def test_mlp_f32_fp16x2_against_fp64(M, D, Hd):
    from acr_wsss_amd import ops
    g = torch.Generator(device="cpu").manual_seed(M + D)
    fc1, fc2 = torch.nn.Linear(D, Hd).to(DEV), torch.nn.Linear(Hd, D).to(DEV)
    with torch.no_grad():
        fc1.bias.copy_(torch.randn(Hd, generator=g) * 0.3)
        fc2.bias.copy_(torch.randn(D, generator=g) * 0.3)
        fc1.weight.mul_(3.0)
    x = torch.randn(1, M, D, generator=g).to(DEV).requires_grad_(True)
    r = torch.randn(1, M, D, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(1, M, D, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        for t in (x, r, fc1.weight, fc1.bias, fc2.weight, fc2.bias):
            t.grad = None
        y = ops.mlp_f32(x, fc1, fc2, r, 2)
        (y * dy).sum().backward()
        runs.append([t.detach().clone() for t in (y, x.grad, r.grad, fc1.weight.grad, fc1.bias.grad, fc2.weight.grad, fc2.bias.grad)])
    assert all(torch.equal(u, v) for u, v in zip(*runs))
    cmp = KC.Cmp()
    KC.verify_mlp(cmp, x, r, [fc1.weight, fc1.bias, fc2.weight, fc2.bias], runs[0][0], dy, runs[0][1:], math=2)
    assert not cmp.failures, "\n".join(cmp.failures)


def _model(kind="hybrid"):
    from acr_wsss_amd.DPT.ACR import ACR
    m = ACR(num_classes=80 if kind == "coco" else 20, backbone_name="vit_tiny" if kind == "tiny" else "vitb_hybrid", use_pretrain=False)
    missing = m.load_state_dict(recipe_sd(kind), strict=(kind != "tiny"))
    if kind == "tiny":
        assert all(k.startswith("scratch.") for k in missing.missing_keys) and not missing.unexpected_keys
    return m.to(DEV)


@pytest.fixture(scope="module")
def hybrid():
    return _model("hybrid")


def test_only_the_block_linears_change(hybrid):
    """Under f32_fp16x2 the stem and the patch-embedding projection (the tokens entering block 0) are bit-identical to
    f32_split, and the attention core is called with the split-product arithmetic (math 1)."""
    from acr_wsss_amd import ops
    vit = hybrid.pretrained.model
    img, _ = make_inputs(1, 96, 20, 2)
    img = img.to(DEV)
    seen, orig = [], ops.attention_core
    captured = {}

    def spy(qkv, heads, stack=None, layer=0, owner=None, math=0):
        seen.append(math)
        return orig(qkv, heads, stack, layer, owner, math)

    h = vit.blocks[0].register_forward_pre_hook(lambda mod, inp: captured.setdefault(hybrid.math, inp[0].detach().clone()))
    ops.attention_core = spy
    try:
        hybrid.train()
        for math in ("f32_split", "f32_fp16x2"):
            hybrid.set_math(math)
            hybrid.zero_grad(set_to_none=True)
            cl, _ = hybrid.forward_mirror(img, img.flip(-1))
            if math == "f32_fp16x2":
                assert seen and all(m == 1 for m in seen), seen
            seen.clear()
    finally:
        ops.attention_core = orig
        h.remove()
        hybrid.set_math("f32")
    assert torch.equal(captured["f32_split"], captured["f32_fp16x2"])
    assert vit.acr_math == 0


ILL_CONDITIONED = {"grad:pretrained.model.patch_embed.backbone.stem.norm.bias": 8e-2}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _train_case(model, fx, rtol_loss=1.5e-5, rtol_attn=2e-4, rtol_grad=2e-3):
    from acr_wsss_amd.train import acr_loss
    size, batch, ncls, alpha, seed = [int(v) for v in fx["meta"]]
    img, label = make_inputs(batch, size, ncls, seed)
    img, label = img.to(DEV), label.to(DEV)
    model.train()
    model.zero_grad()
    cls_list, attn_list = model.forward_mirror(img, img.flip(-1))
    loss, terms = acr_loss(cls_list, attn_list, label, size // 16, alpha)
    loss.backward()
    for k in ("loss", "cls_align", "aff_align", "cls_loss_1", "cls_loss_2"):
        assert abs(float(terms[k]) - float(fx[k])) <= rtol_loss * abs(float(fx[k])) + 1e-7, (k, float(terms[k]), float(fx[k]))
    for i, k in enumerate(("x_cls_1", "x_cls_2", "x_p_cls_1", "x_p_cls_2")):
        assert _rel(cls_list[i].detach().cpu().numpy(), fx[k]) <= 1e-4, k
    for i, k in enumerate(("attn1", "attn2")):
        a = attn_list[i].detach().cpu().numpy()
        if k in fx:
            assert _rel(a, fx[k]) <= rtol_attn, (k, _rel(a, fx[k]))
        else:
            s0, s1 = [int(v) for v in fx["sub"]]
            assert _rel(a[:, :, ::s0, ::s1], fx[k + "_sub"]) <= rtol_attn
            assert _rel(a[:, :, 0, :], fx[k + "_row0"]) <= rtol_attn
            np.testing.assert_allclose(a.astype(np.float64).sum(axis=(2, 3)), fx[k + "_sum"], rtol=1e-5)
    params = dict(model.named_parameters())
    n = 0
    for k, v in fx.items():
        if k.startswith("grad:"):
            g = params[k[5:]].grad
            assert g is not None, k
            assert _rel(g.cpu().numpy(), v) <= ILL_CONDITIONED.get(k, rtol_grad), (k, _rel(g.cpu().numpy(), v))
            n += 1
    assert n >= 5
    return terms


@pytest.mark.parametrize("kind,name,rtol_loss", [("hybrid", "train_hybrid_64_b2", 1.5e-5), ("hybrid", "train_hybrid_96_b1", 1.5e-5),
                                                 ("hybrid", "train_hybrid_448_b1", 5e-6), ("tiny", "train_tiny_224_b2", 1.5e-5),
                                                 ("coco", "train_coco_512_b1", 5e-6)])
def test_train_parity_fp16x2(hybrid, kind, name, rtol_loss):
    model = hybrid if kind == "hybrid" else _model(kind)
    model.set_math("f32_fp16x2")
    try:
        _train_case(model, load_golden(name), rtol_loss=rtol_loss)
    finally:
        model.set_math("f32")


def test_infer_cam_fp16x2_seeds(hybrid):
    """CAM generation (graphs included: the default path and the launch-by-launch one) on an f32_fp16x2 model against the
    reference's infer_hybrid_384 fixture: seeds exact-or-tie at the suite's fixed margin."""
    import test_model_gpu as TM
    hybrid.set_math("f32_fp16x2")
    try:
        TM._infer_cam_real_geometry_and_multi_scale(hybrid, "infer_hybrid_384")
    finally:
        hybrid.set_math("f32")
        TM._drop_graphs(hybrid.pretrained.model)


def test_mode_is_per_model_and_reproducible(hybrid):
    from acr_wsss_amd.train import acr_loss
    img, label = make_inputs(1, 96, 20, 4)
    img, label = img.to(DEV), label.to(DEV)
    outs = []
    try:
        for math in ("f32_split", "f32_fp16x2", "f32_split", "f32_fp16x2"):
            hybrid.set_math(math)
            hybrid.train()
            hybrid.zero_grad(set_to_none=True)
            cl, al = hybrid.forward_mirror(img, img.flip(-1))
            loss, _ = acr_loss(cl, al, label, 6, 125)
            loss.backward()
            outs.append((loss.detach().clone(), al.stacked.detach().clone(),
                         dict(hybrid.named_parameters())["pretrained.model.blocks.3.attn.qkv.weight"].grad.clone()))
    finally:
        hybrid.set_math("f32")
    for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    assert abs(float(outs[0][0]) - float(outs[1][0])) <= 1e-5 * abs(float(outs[0][0]))
    gs, gh = outs[0][2].double(), outs[1][2].double()
    assert float((gs - gh).abs().max() / gs.abs().max()) <= 2e-3
