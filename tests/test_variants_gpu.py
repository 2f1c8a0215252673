"""Every kernel variant an ``extern "C"`` entry point chooses on its own, on each side of the choice.

tests/test_dispatch_gpu.py holds what *Python* decides (the ``*_fusable`` / ``*_usable`` predicates) to a float64 reference on both
sides of its edge.  The C entry points decide too -- by a shape remainder, a leading dimension, a workspace that was not passed or
the low bits of a pointer -- among different kernels or among a vector and a scalar body of one kernel, and fresh ``torch.empty``
tensors (256-byte aligned, dense, N a multiple of 8, a workspace always there) only ever reach one side.  This file calls each entry
with the smallest arguments that reach EACH side and compares with float64 through tests/kernel_checks.py; variants documented as
the same operations in the same order are also held to each other bit for bit.

Which side a case is on is decided by the restatements of tests/variant_rules.py (tied to the source by tests/test_variants_cpu.py,
which also checks every claim below without a GPU): each test asserts that the pointers it really passes give the side its case
claims.  Misaligned operands are contiguous views that start 4 bytes (fp32), 2 bytes (bf16) or 1 byte (uint8) off a 16-byte
boundary inside a larger buffer; every output lies between guard elements of that buffer, which must come back unchanged, and is
filled with NaN (0xEE for bytes) before the call, so that an element the kernel leaves out cannot pass.

Sides another test already runs are cited where the case table leaves them out."""
import functools
import math as pymath
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_checks as KC
import pseudo_sal_ref as PSR
import traincam_ref as TCR
import variant_rules as VR
from kernel_checks import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
GUARD = {F32: -7.25, BF16: -7.25, U8: 0xA5}                  # exact in every format
UNWRITTEN = {F32: float("nan"), BF16: float("nan"), U8: 0xEE}
FRONT = 16                                                   # guard elements in front: a multiple of 16 bytes for every dtype


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _rand(g, shape, dtype=F32, scale=1.0):
    """Seeded on the CPU, rounded to ``dtype`` once."""
    return (torch.randn(tuple(shape), generator=g) * scale).to(dtype).to(DEV)


def _lib():
    from acr_wsss_amd import _lib as L
    return L, L.load()


class Placed:
    """An operand inside a larger buffer: FRONT guard elements, ``mis`` BYTES past a 16-byte boundary, rows ``ld`` elements apart
    (the elements between the rows are guards too), 16 guard elements behind.  ``t``: the operand as a view of the buffer, holding
    ``src`` (an input) or the unwritten mark (an output)."""

    def __init__(self, shape, dtype, mis=0, ld=None, src=None):
        size = torch.empty(0, dtype=dtype).element_size()
        assert mis % size == 0
        shape = tuple(shape)
        cols = shape[-1] if ld is not None else int(np.prod(shape))
        rows = int(np.prod(shape[:-1])) if ld is not None else 1
        ld = cols if ld is None else ld
        assert ld >= cols and (ld == cols or len(shape) == 2)
        front = FRONT + mis // size
        self.buf = torch.full((front + rows * ld + 16,), GUARD[dtype], dtype=dtype, device=DEV)
        body = self.buf[front:front + rows * ld].view(rows, ld)[:, :cols]
        self.guard = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        self.guard[front:front + rows * ld].view(rows, ld)[:, :cols] = False
        if src is not None:
            body.copy_(src.detach().reshape(rows, cols))
        else:
            body.fill_(UNWRITTEN[dtype])
        self.t = body if ld != cols else body.reshape(shape)
        assert self.t.data_ptr() % 16 == mis and self.t.stride(-1) == 1
        if mis:
            assert self.t.data_ptr() % 16 != 0

    def intact(self):
        g = self.buf[self.guard]
        assert bool((g == GUARD[self.buf.dtype]).all()), "guard elements around the operand were written"


def _mod(t):
    return None if t is None else t.data_ptr() % 16


def _passes(cmp):
    assert cmp.compared > 0
    assert not cmp.failures, "\n".join(cmp.failures)


def _same_bits(a, b, what):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, what
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    ia, ib = a.view(bits), b.view(bits)
    assert torch.equal(ia, ib), "%s: %d of %d elements differ in their bits" % (what, int((ia != ib).sum()), ia.numel())


def claims():
    """(id, rule, keyword arguments, claimed side) of every case of this file -- what tests/test_variants_cpu.py checks."""
    out = []
    for fn in (_linear_claims, _gemm_claims, _sgd_claims, _pool_claims, _ksplit_claims, _traincam_claims, _sal_claims):
        out += list(fn())
    return out


# ------------------------------------------------------------------------------------------------
# 1. acr_linear_bf16: scalar epilogue / 128x128 DMA kernel / 320x256 wide kernel, each <bias, resid> instance
# ------------------------------------------------------------------------------------------------
# name -> M, N, K, extra elements of y's / resid's pitch, misalignment in bytes of y / bias / resid, the operand the trigger needs
LINEAR_SCALAR = {
    "N20-one-partial-tile": dict(M=3, N=20, K=64),
    "N20-two-tiles-ragged-M": dict(M=130, N=20, K=128),
    "bias-one-element-in": dict(M=130, N=200, K=64, bias_mis=2, needs="bias"),
    "resid-ldr-N+4": dict(M=130, N=200, K=64, ldr_pad=4, needs="resid"),
    "y-ldy-N+4": dict(M=130, N=200, K=64, ldy_pad=4),
    "y-2-bytes-off": dict(M=130, N=200, K=64, y_mis=2),
}
# the aligned neighbour of the scalar cases (the DMA kernel with ragged tiles in both directions), and the tilesw >= 200 edge:
# N = 256 is one wide tile column, so tilesw = ceil(M / 320)
LINEAR_VEC = {
    "N200-aligned": dict(M=130, N=200, K=64, side="dma"),
    "199-wide-tiles": dict(M=199 * VR.GW_BM, N=256, K=64, side="dma"),
    "200-wide-tiles-one-row-last": dict(M=199 * VR.GW_BM + 1, N=256, K=64, side="wide"),
}
COMBOS = [(False, False), (True, False), (False, True), (True, True)]


def _linear_cases():
    for name, c in LINEAR_SCALAR.items():
        for bias, resid in COMBOS:
            if (c.get("needs") == "bias" and not bias) or (c.get("needs") == "resid" and not resid):
                continue                                     # without that operand the trigger is not there
            yield "%s-bias%d-resid%d" % (name, bias, resid), dict(c, side="scalar"), bias, resid
    for name, c in LINEAR_VEC.items():
        for bias, resid in (COMBOS if name == "N200-aligned" else [(False, False), (True, True)]):
            yield "%s-bias%d-resid%d" % (name, bias, resid), c, bias, resid


def _linear_rule_args(c, bias, resid):
    N = c["N"]
    return dict(M=c["M"], N=N, ldy=N + c.get("ldy_pad", 0), ldr=(N + c.get("ldr_pad", 0)) if resid else 0, y=c.get("y_mis", 0),
                bias=c.get("bias_mis", 0) if bias else None, resid=c.get("resid_mis", 0) if resid else None)


def _linear_claims():
    for cid, c, bias, resid in _linear_cases():
        yield "linear-" + cid, VR.linear_bf16_variant, _linear_rule_args(c, bias, resid), c["side"]


@pytest.mark.parametrize("cid,c,has_bias,has_resid", [pytest.param(*t, id=t[0]) for t in _linear_cases()])
def test_linear_bf16_kernels(cid, c, has_bias, has_resid):
    """acr_linear_bf16 through the C ABI vs float64 at KC.TOL["linear"][BF16]: the scalar-epilogue kernel by each of its triggers
    in the <bias, resid> instances the trigger exists in, its aligned neighbour, and both sides of the 200-wide-tile edge.
    (The DMA and the wide kernel on ordinary tensors: test_kernels_gpu.py::test_linear_bf16.)"""
    L, lib = _lib()
    M, N, K = c["M"], c["N"], c["K"]
    g = _gen("linear", M, N, K)
    x, w = _rand(g, (M, K), BF16), _rand(g, (N, K), BF16, K ** -0.5)
    bias = Placed((N,), BF16, c.get("bias_mis", 0), src=_rand(g, (N,), BF16)) if has_bias else None
    resid = Placed((M, N), BF16, c.get("resid_mis", 0), ld=N + c.get("ldr_pad", 0), src=_rand(g, (M, N), BF16)) if has_resid else None
    y = Placed((M, N), BF16, c.get("y_mis", 0), ld=N + c.get("ldy_pad", 0))
    bt, rt = (bias.t if bias else None), (resid.t if resid else None)
    args = dict(M=M, N=N, ldy=y.t.stride(0), ldr=rt.stride(0) if rt is not None else 0, y=_mod(y.t), bias=_mod(bt), resid=_mod(rt))
    assert args == _linear_rule_args(c, has_bias, has_resid) and VR.linear_bf16_variant(**args) == c["side"]
    L.check(lib.acr_linear_bf16(L.ptr(x), x.stride(0), L.ptr(w), w.stride(0), L.ptr(bt), L.ptr(rt), args["ldr"], L.ptr(y.t), args["ldy"],
                                M, N, K, L.stream_ptr()), "acr_linear_bf16")
    cmp = KC.Cmp()
    KC.verify_linear(cmp, x, w, bt, rt, y.t, None, [])
    _passes(cmp)
    for p in (y, bias, resid):
        if p is not None:
            p.intact()


@pytest.mark.parametrize("din,with_resid", [(64, False), (128, True)])
def test_linear_bf16_scalar_epilogue_through_autograd(din, with_resid):
    """ops.linear_or_hip on a bf16 nn.Linear with 20 outputs: the forward is the scalar-epilogue kernel (N % 8 != 0), the backward
    takes torch.mm for dx (20 is no multiple of the K tile) and for dW (no multiple of 128) and a plain sum for db: output and
    every gradient vs float64."""
    from acr_wsss_amd import ops
    g = _gen("linear-autograd", din)
    lin = torch.nn.Linear(din, 20).to(DEV).to(BF16)
    with torch.no_grad():
        lin.weight.copy_(_rand(g, (20, din), BF16, din ** -0.5))
        lin.bias.copy_(_rand(g, (20,), BF16))
    x = _rand(g, (3, 11, din), BF16).requires_grad_(True)
    resid = _rand(g, (3, 11, 20), BF16).requires_grad_(True) if with_resid else None
    assert VR.linear_bf16_variant(M=33, N=20, ldy=20, ldr=20 if with_resid else 0, y=0, bias=_mod(lin.bias), resid=_mod(resid)) == "scalar"
    y = ops.linear_or_hip(x, lin, resid)
    assert isinstance(y.grad_fn, ops.LinearBf16Fn._backward_cls)
    dy = _rand(g, (3, 11, 20), BF16)
    y.backward(dy)
    cmp = KC.Cmp()
    KC.verify_linear(cmp, x, lin.weight, lin.bias, resid, y, dy, KC.grads_of(x, lin.weight, lin.bias, resid))
    _passes(cmp)


# ------------------------------------------------------------------------------------------------
# 2. acr_gemm_f32: images / in-kernel split / DMA / staged loop, K-split tail tiles, the TN branch
# ------------------------------------------------------------------------------------------------
# what makes vec_ok false or takes the workspace away, one at a time ("aligned": the other side of all of them)
GEMM_TRIGGERS = {
    "aligned": dict(act=0, bias=True, aux=True),
    "aligned-act1": dict(act=1, bias=True, c2=True),        # at K = 192 the GELU / GELU' epilogues of the tail's own kernel
    "aligned-act2": dict(act=2, aux=True),
    "ws-null": dict(act=0, bias=True, aux=True, ws=None),
    "ws-off4": dict(act=0, bias=True, aux=True, ws=4),
    "bias-off4": dict(act=0, bias=True, bias_mis=4),
    "ldc-N+1": dict(act=0, bias=True, ldc_pad=1),
    "aux-off4-act2": dict(act=2, aux=True, aux_mis=4),
    "c2-off4-act1": dict(act=1, bias=True, c2=True, c2_mis=4),
}
GEMM_UNALIGNED = sorted(t for t in GEMM_TRIGGERS if not t.startswith("aligned"))
GEMM_MN = 132                                                # two tiles each way, every one ragged
GEMM_KS = (72, 96, 192)                                      # K % 32 != 0: the staged loop; the DMA loops; the smallest K with a tail plan
MODES = {"nt": VR.NT, "nn": VR.NN}


def _gemm_claim(trigger, math, K):
    """By hand: 72 is no multiple of the 32-deep chunk (the staged exact-fp32 loop, whatever the math); with a 16-byte aligned
    workspace and operands math 1 runs on images and math 0 K-splits its four tiles at K = 192 (192 / 64 = 3 parts)."""
    exact = {72: "staged", 96: "dma", 192: "dma"}[K]
    if trigger.startswith("aligned"):
        return ("planes", 0) if math == 1 else (exact, 4 if K == 192 else 0)
    return ("split" if (math == 1 and K != 72) else exact), 0


def _gemm_rule_args(trigger, mode, math, M, N, K):
    t = GEMM_TRIGGERS[trigger]
    return dict(mode=MODES[mode], math=math, M=M, N=N, K=K, ldc=N + t.get("ldc_pad", 0), ldaux=N if t.get("aux") else 0, ws=t.get("ws", 0), c=0,
                bias=t.get("bias_mis", 0) if t.get("bias") else None, aux=t.get("aux_mis", 0) if t.get("aux") else None,
                c2=t.get("c2_mis", 0) if t.get("c2") else None)


# tail plan on / off at its smallest shape (K = 192: three parts of 64; K = 160 allows two, below the minimum of three), with
# several ragged tail tiles, and behind two whole rounds of 256 tiles (23 x 23 = 529 tiles: 17 tail tiles)
TAIL_SHAPES = {(5, 8, 192): 1, (5, 8, 160): 0, (2893, 2900, 192): 17}


def _gemm_claims():
    for trigger in GEMM_TRIGGERS:
        for mode in MODES:
            for math in (0, 1):
                for K in GEMM_KS:
                    yield ("gemm-%s-%s-math%d-K%d" % (trigger, mode, math, K), VR.gemm_f32_variant,
                           _gemm_rule_args(trigger, mode, math, GEMM_MN, GEMM_MN, K), _gemm_claim(trigger, math, K))
    for trigger in GEMM_UNALIGNED:
        yield "gemm-fp16x2-%s" % trigger, VR.gemm_f32_variant, _gemm_rule_args(trigger, "nt", 2, GEMM_MN, GEMM_MN, 96), ("refused", 0)
    for (M, N, K), ntail in TAIL_SHAPES.items():
        for mode in MODES:
            yield ("gemm-tail-%dx%dx%d-%s" % (M, N, K, mode), VR.gemm_f32_variant, _gemm_rule_args("aligned", mode, 0, M, N, K),
                   ("dma", ntail))
    for math in (0, 1):
        for K, loop in ((72, "staged"), (96, "dma"), (520, "staged"), (544, "dma")):
            yield ("gemm-tn-math%d-K%d" % (math, K), VR.gemm_f32_variant, dict(mode=VR.TN, math=math, M=GEMM_MN, N=GEMM_MN, K=K),
                   ("planes" if math == 1 else loop, 0))
        yield "gemm-tn-math%d-ws-null" % math, VR.gemm_f32_variant, dict(mode=VR.TN, math=math, M=GEMM_MN, N=GEMM_MN, K=96, ws=None), ("refused", 0)


@functools.lru_cache(maxsize=None)
def _gemm_inputs(mode, M, N, K):
    """(a, b, bias, aux, float64 a.b) of one product, shared by every case on it; h = a.b + bias is about N(0, 1)."""
    g = _gen("gemm", mode, M, N, K)
    a = _rand(g, (M, K))
    b = _rand(g, (N, K) if mode == "nt" else (K, N), scale=K ** -0.5)
    bias, aux = _rand(g, (N,), scale=0.5), _rand(g, (M, N))
    acc = a.double() @ (b.double().t() if mode == "nt" else b.double())
    return a, b, bias, aux, acc


def _gemm_ws(lib, md, math, M, N, K, ws_mode):
    """The call's workspace: the floats acr_gemm_f32_ws_floats asks for (ws_mode 0), the same 4 bytes off, or none."""
    if ws_mode is None:
        return None
    n = max(int(lib.acr_gemm_f32_ws_floats(md, math, M, N, K)), 4) + 4
    buf = torch.zeros(n, dtype=F32, device=DEV)
    return buf[ws_mode // 4:]


def _gemm_call(trigger, mode, math, M, N, K):
    """One acr_gemm_f32 call of a trigger's layout -> (return code, c, c2, float64 references of c and c2, the placed operands)."""
    L, lib = _lib()
    t = GEMM_TRIGGERS[trigger]
    a, b, bias0, aux0, acc = _gemm_inputs(mode, M, N, K)
    ldc = N + t.get("ldc_pad", 0)
    bias = Placed((N,), F32, t.get("bias_mis", 0), src=bias0) if t.get("bias") else None
    aux = Placed((M, N), F32, t.get("aux_mis", 0), ld=N, src=aux0) if t.get("aux") else None
    c = Placed((M, N), F32, 0, ld=ldc)
    c2 = Placed((M, N), F32, t.get("c2_mis", 0), ld=ldc) if t.get("c2") else None          # c2 shares c's pitch
    ws = _gemm_ws(lib, MODES[mode], math, M, N, K, t.get("ws", 0))
    bt, at, c2t = (bias.t if bias else None), (aux.t if aux else None), (c2.t if c2 else None)
    args = dict(mode=MODES[mode], math=math, M=M, N=N, K=K, ldc=c.t.stride(0), ldaux=at.stride(0) if at is not None else 0, ws=_mod(ws),
                c=_mod(c.t), bias=_mod(bt), aux=_mod(at), c2=_mod(c2t))
    assert args == _gemm_rule_args(trigger, mode, math, M, N, K)
    rc = lib.acr_gemm_f32(MODES[mode], math, t["act"], L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), L.ptr(bt), L.ptr(at), args["ldaux"],
                          L.ptr(c.t), args["ldc"], L.ptr(c2t), None, M, N, K, L.ptr(ws), L.stream_ptr())
    if t["act"] == 0:
        want, want2 = acc + (bias0.double() if bias else 0) + (aux0.double() if aux else 0), None
    elif t["act"] == 1:                                      # c = GELU'(h), c2 = GELU(h), h = acc + bias (include/acr_hip.h)
        h = acc + bias0.double()
        cdf = 0.5 * (1 + torch.erf(h / pymath.sqrt(2.0)))
        want, want2 = cdf + h * torch.exp(-0.5 * h * h) / pymath.sqrt(2 * pymath.pi), h * cdf
    else:                                                    # c = acc * aux, aux = the saved GELU'
        want, want2 = acc * aux0.double(), None
    return rc, args, c, c2, want, want2, [p for p in (c, c2, bias, aux) if p is not None]


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("trigger", sorted(GEMM_TRIGGERS))
def test_gemm_f32_loops_by_workspace_and_alignment(trigger, mode, math):
    """acr_gemm_f32 NT / NN with every operand aligned and a workspace, and with exactly one thing taken away -- the workspace, its
    alignment, the alignment of bias / aux / c2 or the pitch of c -- which turns off the operand images (math 1) and the K-split
    tail (math 0, K = 192) and leaves the whole product to the per-tile kernels and their scalar epilogue.  The aligned layouts
    run all three epilogues, which at K = 192 under math 0 are those of gemm_f32_tail_epilogue_kernel<0 / 1 / 2>.  vs float64 at
    KC.TOL["linear"][F32]["y"] (act 0) resp. KC.TOL["mlp"][math] (acts 1 and 2: the fc1 / fc2 epilogues of the fused MLP, whose
    entry that is).  (The aligned side at the model's shapes: test_kernels_gpu.py::test_gemm_f32_linear, ::test_fused_mlp_f32.)"""
    for K in GEMM_KS:
        rc, args, c, c2, want, want2, placed = _gemm_call(trigger, mode, math, GEMM_MN, GEMM_MN, K)
        L, _ = _lib()
        L.check(rc, "acr_gemm_f32")
        assert VR.gemm_f32_variant(**args) == _gemm_claim(trigger, math, K)
        act = GEMM_TRIGGERS[trigger]["act"]
        tol = KC.TOL["linear"][F32]["y"] if act == 0 else KC.TOL["mlp"][math]
        cmp = KC.Cmp()
        cmp.where = "K=%d" % K
        cmp.check("c", c.t, want, **tol)
        if c2 is not None:
            cmp.check("c2", c2.t, want2, **tol)
        _passes(cmp)
        for p in placed:
            p.intact()


@pytest.mark.parametrize("trigger", GEMM_UNALIGNED)
def test_gemm_f32_fp16x2_refuses_what_it_cannot_read_as_vectors(trigger):
    """math 2 has no scalar epilogue and no way without its images: the same arguments are refused with the documented message,
    and nothing is written.  (The accepted side: tests/test_fp16x2_gpu.py.)"""
    L, lib = _lib()
    rc, args, c, c2, _, _, placed = _gemm_call(trigger, "nt", 2, GEMM_MN, GEMM_MN, 96)
    torch.cuda.synchronize()
    assert VR.gemm_f32_variant(**args) == ("refused", 0)
    assert rc != 0 and lib.acr_last_error().decode() == VR.FP16X2_REFUSAL
    assert bool(torch.isnan(c.t).all()) and (c2 is None or bool(torch.isnan(c2.t).all()))
    for p in placed:
        p.intact()


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", sorted(TAIL_SHAPES), ids=lambda s: "%dx%dx%d" % s)
def test_gemm_f32_tail_plan_on_and_off(shape, mode, math):
    """gemm_tail_plan at its smallest (M, N, K) with a tail (one tile in three parts), its neighbour without (K = 160 allows two
    parts only) and a product of 529 tiles whose last 17 are K-split behind two whole rounds; bias and residual in the tail's own
    epilogue kernel.  math 1 takes the images at these arguments (its own tail plan is acr_gemm_x3's)."""
    M, N, K = shape
    rc, args, c, _, want, _, placed = _gemm_call("aligned", mode, math, M, N, K)
    L, _ = _lib()
    L.check(rc, "acr_gemm_f32")
    assert VR.gemm_tail_plan(M, N, K)[0] == TAIL_SHAPES[shape]
    assert VR.gemm_f32_variant(**args) == (("planes", 0) if math == 1 else ("dma", TAIL_SHAPES[shape]))
    cmp = KC.Cmp()
    cmp.check("c", c.t, want, **KC.TOL["linear"][F32]["y"])
    _passes(cmp)
    for p in placed:
        p.intact()


@pytest.mark.parametrize("with_colsum", [False, True])
@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("K", [72, 96, 520, 544])
def test_gemm_f32_tn_loops(K, math, with_colsum):
    """The TN branch (weight gradient, + the bias gradient from the same sweep): the staged loop (K % 32 != 0), the DMA loop, and
    under math 1 the product on images -- K = 72 / 96 in one part, K = 520 / 544 split over workgroups.  vs float64 at
    KC.TOL["linear"][F32]'s dW / db.  (Under math 1 the entry always makes images: the in-kernel split loop behind them is not
    reachable)"""
    L, lib = _lib()
    M = N = GEMM_MN
    g = _gen("gemm-tn", K)
    a, b = _rand(g, (K, M)), _rand(g, (K, N))
    c = Placed((M, N), F32)
    cs = Placed((M,), F32) if with_colsum else None
    ws = _gemm_ws(lib, VR.TN, math, M, N, K, 0)
    claim = ("planes" if math == 1 else ("dma" if K % 32 == 0 else "staged"), 0)
    assert VR.gemm_f32_variant(mode=VR.TN, math=math, M=M, N=N, K=K) == claim
    L.check(lib.acr_gemm_f32(VR.TN, math, 0, L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), None, None, 0, L.ptr(c.t), N, None,
                             L.ptr(cs.t) if cs else None, M, N, K, L.ptr(ws), L.stream_ptr()), "acr_gemm_f32")
    t = KC.TOL["linear"][F32]
    cmp = KC.Cmp()
    cmp.check("c", c.t, a.double().t() @ b.double(), **t["dW"])
    if cs is not None:
        cmp.check("colsum", cs.t, a.double().sum(0), **t["db"])
        cs.intact()
    _passes(cmp)
    c.intact()


@pytest.mark.parametrize("math", [0, 1])
def test_gemm_f32_tn_refuses_a_null_workspace(math):
    """TN has no way without its slabs: refused with the documented message, nothing written."""
    L, lib = _lib()
    M = N = GEMM_MN
    g = _gen("gemm-tn", 96)
    a, b = _rand(g, (96, M)), _rand(g, (96, N))
    c = Placed((M, N), F32)
    assert VR.gemm_f32_variant(mode=VR.TN, math=math, M=M, N=N, K=96, ws=None) == ("refused", 0)
    rc = lib.acr_gemm_f32(VR.TN, math, 0, L.ptr(a), a.stride(0), L.ptr(b), b.stride(0), None, None, 0, L.ptr(c.t), N, None, None, M, N, 96,
                          None, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and lib.acr_last_error().decode() == VR.TN_NULL_WS_REFUSAL
    assert bool(torch.isnan(c.t).all())
    c.intact()


# ------------------------------------------------------------------------------------------------
# 3. acr_sgd_step_bf16 / acr_sgd_step_f32: vector or scalar body per tensor, by the pointers in the table
# ------------------------------------------------------------------------------------------------
SGD_OFFSETS = (0, 1, 3)                                      # element offsets of a tensor's start from a 16-byte boundary, in every role
SGD_LRS = (0.05, 0.031, 0.0127)
SGD_MU = 0.9


def _sgd_lengths(chunk):
    return (1, 7, 8, chunk - 1, chunk, chunk + 1, 2 * chunk + 7)


def _sgd_tensors(chunk):
    """(length, element offset of grad / master / momentum / param): every length at every offset, and one tensor whose momentum
    buffer alone is off."""
    ts = [(n, (o, o, o, o)) for n in _sgd_lengths(chunk) for o in SGD_OFFSETS]
    return ts + [(chunk + 9, (0, 0, 1, 0))]


def _sgd_claims():
    for dtype, gsize in (("bf16", 2), ("f32", 4)):
        for n, (og, om, ob, op) in _sgd_tensors(VR.SGD_CHUNK):
            side = "vec" if (og, om, ob, op) == (0, 0, 0, 0) else "scalar"
            yield ("sgd-%s-n%d-off%d%d%d%d" % (dtype, n, og, om, ob, op), VR.sgd_variant,
                   dict(grad=og * gsize, master=om * 4, mom=ob * 4, param=op * 2 if dtype == "bf16" else None), side)


def _flat_views(tensors, role, dtype, fill):
    """Views of ONE flat buffer, tensor i starting ``tensors[i][1][role]`` elements past a 16-byte boundary, guard elements
    between neighbours -> (views, buffer, guard mask)."""
    pos, spans = 0, []
    for n, offs in tensors:
        start = (pos + 1 + 7) // 8 * 8 + offs[role]          # at least one guard element; 8 elements are 16 (bf16) or 32 bytes
        spans.append((start, n))
        pos = start + n
    buf = torch.full((pos + 8,), GUARD[dtype], dtype=dtype, device=DEV)
    guard = torch.ones(pos + 8, dtype=torch.bool, device=DEV)
    views = []
    for (start, n), (_, offs) in zip(spans, tensors):
        v = buf[start:start + n]
        guard[start:start + n] = False
        v.copy_(fill(n))
        assert v.data_ptr() % 16 == offs[role] * buf.element_size() % 16
        views.append(v)
    return views, buf, guard


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_sgd_step_vector_and_scalar_bodies(dtype):
    """The fused SGD steps over views of one flat buffer per role (gradient buckets, flattened parameters): lengths around the chunk
    at element offsets 0, 1 and 3, and a tensor with only its momentum buffer off.  Three steps with a changing learning rate:
    masters, momentum buffers and bf16 copies bit-equal to torch's SGD on separately allocated tensors (the standard of
    test_model_gpu.py::test_fused_sgd_step_matches_torch_sgd / ::test_fused_sgd_f32_matches_torch_sgd), the bodies bit-equal to
    each other (tensors of one length hold the same values at every offset), guards intact."""
    L, lib = _lib()
    chunk = int(lib.acr_sgd_chunk_elems())
    assert chunk == VR.SGD_CHUNK
    tensors = _sgd_tensors(chunk)
    gdt = BF16 if dtype == "bf16" else F32
    values = lambda what, step: (lambda n: _rand(_gen("sgd", what, step, n), (n,)))
    masters, mbuf, mguard = _flat_views(tensors, 1, F32, values("w", 0))
    moms, bbuf, bguard = _flat_views(tensors, 2, F32, lambda n: torch.zeros(n, device=DEV))
    grads, gbuf, gguard = _flat_views(tensors, 0, gdt, lambda n: torch.zeros(n, device=DEV, dtype=gdt))
    if dtype == "bf16":
        params, pbuf, pguard = _flat_views(tensors, 3, BF16, lambda n: torch.zeros(n, device=DEV, dtype=BF16))
    for i, (n, offs) in enumerate(tensors):
        args = dict(grad=_mod(grads[i]), master=_mod(masters[i]), mom=_mod(moms[i]), param=_mod(params[i]) if dtype == "bf16" else None)
        assert VR.sgd_variant(**args) == ("vec" if offs == (0, 0, 0, 0) else "scalar")
    tab = torch.tensor([[grads[i].data_ptr(), masters[i].data_ptr(), moms[i].data_ptr(), params[i].data_ptr() if dtype == "bf16" else 0, n]
                        for i, (n, _) in enumerate(tensors)], dtype=torch.int64).to(DEV)
    nch = [(n + chunk - 1) // chunk for n, _ in tensors]
    bt = torch.tensor([i for i, k in enumerate(nch) for _ in range(k)], dtype=torch.int32).to(DEV)
    bc = torch.tensor([j for k in nch for j in range(k)], dtype=torch.int32).to(DEV)
    # the reference: torch SGD on separately allocated fp32 masters, gradients cast up, the bf16 copy cast down afterwards
    ref = [torch.nn.Parameter(m.detach().clone()) for m in masters]
    opt = torch.optim.SGD(ref, lr=SGD_LRS[0], momentum=SGD_MU)
    step = lib.acr_sgd_step_bf16 if dtype == "bf16" else lib.acr_sgd_step_f32
    for it, lr in enumerate(SGD_LRS):
        for i, (n, _) in enumerate(tensors):
            gv = values("g", it + 1)(n).to(gdt)
            grads[i].copy_(gv)
            ref[i].grad = gv.float()
        opt.param_groups[0]["lr"] = lr
        opt.step()
        L.check(step(L.ptr(tab), L.ptr(bt), L.ptr(bc), bt.numel(), lr, SGD_MU, L.stream_ptr()), "acr_sgd_step")
    first = {}
    for i, (n, offs) in enumerate(tensors):
        what = "n=%d offsets %s" % (n, offs)
        assert torch.equal(masters[i], ref[i].detach()), "master, " + what
        assert torch.equal(moms[i], opt.state[ref[i]]["momentum_buffer"]), "momentum, " + what
        got = [masters[i], moms[i]]
        if dtype == "bf16":
            assert torch.equal(params[i], ref[i].detach().to(BF16)), "bf16 copy, " + what
            got.append(params[i])
        for a, b in zip(got, first.setdefault(n, got)):
            _same_bits(a, b, "vector and scalar body, " + what)
    checks = [(mbuf, mguard), (bbuf, bguard), (gbuf, gguard)] + ([(pbuf, pguard)] if dtype == "bf16" else [])
    for buf, guard in checks:
        assert bool((buf[guard] == GUARD[buf.dtype]).all()), "guard elements between the tensors were written"


# ------------------------------------------------------------------------------------------------
# 4. pool.hip: maxpool_fwd (vec4 / scalar), maxpool_bwd (2x8 / 8-wide / scalar), subsample2 (vector / scalar)
# ------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 3, 8, 16), (1, 2, 6, 8)]                  # even maps, W % 8 == 0: SAME pads (0, 1, 0, 1), the vector kernels' geometry
POOL_ODD_H = (1, 2, 7, 8)                                    # rows 7, padding 2 below: ho * 2 != h sends the 2x8 backward to 8-wide
# which single operand is off (bytes) -> the side claimed for fp32 maps
POOL_FWD = {"aligned": (None, 0, "vec4"), "x-off4": ("x", 4, "scalar"), "y-off4": ("y", 4, "scalar"), "amax-off1": ("amax", 1, "scalar")}
POOL_BWD = {"aligned": (None, 0, "2x8"), "dy-off4": ("dy", 4, "8wide"), "amax-off1": ("amax", 1, "8wide"), "dx-off4": ("dx", 4, "scalar")}
POOL_BWD_BF16 = {"aligned": (None, 0, "8wide"), "dx-off2": ("dx", 2, "scalar")}
SUB_FWD = {"aligned": (None, 0, "vec"), "x-off4": ("x", 4, "scalar"), "y-off4": ("y", 4, "scalar")}
SUB_BWD = {"aligned": (None, 0, "vec"), "dy-off4": ("dy", 4, "scalar"), "dx-off4": ("dx", 4, "scalar")}


def _pool_geom(shape):
    N, C, H, W = shape
    ph, pw = (2 if H % 2 else 1), 1                          # pad_top = pad_left = 0
    return N * C, H, W, (H + ph - 3) // 2 + 1, (W + pw - 3) // 2 + 1, ph, pw


def _off(table, key, name):
    which, mis, _ = table[key]
    return mis if which == name else 0


def _pool_claims():
    for shape in POOL_SHAPES + [POOL_ODD_H]:
        nc, H, W, Ho, Wo, _, _ = _pool_geom(shape)
        tag = "x".join(map(str, shape))
        for k, (_, _, side) in POOL_FWD.items():
            yield ("maxpool-fwd-f32-%s-%s" % (tag, k), VR.maxpool_fwd_variant,
                   dict(elsize=4, pt=0, pl=0, w=W, wo=Wo, x=_off(POOL_FWD, k, "x"), y=_off(POOL_FWD, k, "y"), amax=_off(POOL_FWD, k, "amax")), side)
        for k, (_, _, side) in POOL_BWD.items():
            if shape == POOL_ODD_H:
                side = "8wide" if side == "2x8" else side
            yield ("maxpool-bwd-f32-%s-%s" % (tag, k), VR.maxpool_bwd_variant,
                   dict(elsize=4, pt=0, pl=0, h=H, w=W, ho=Ho, wo=Wo, dy=_off(POOL_BWD, k, "dy"), amax=_off(POOL_BWD, k, "amax"),
                        dx=_off(POOL_BWD, k, "dx")), side)
        for k, (_, _, side) in POOL_BWD_BF16.items():
            yield ("maxpool-bwd-bf16-%s-%s" % (tag, k), VR.maxpool_bwd_variant,
                   dict(elsize=2, pt=0, pl=0, h=H, w=W, ho=Ho, wo=Wo, dy=0, amax=0, dx=_off(POOL_BWD_BF16, k, "dx")), side)
    for shape in POOL_SHAPES:
        tag = "x".join(map(str, shape))
        for k, (_, _, side) in SUB_FWD.items():
            yield "subsample2-fwd-%s-%s" % (tag, k), VR.subsample2_variant, dict(w=shape[3], src=_off(SUB_FWD, k, "x"), dst=_off(SUB_FWD, k, "y")), side
        for k, (_, _, side) in SUB_BWD.items():
            yield "subsample2-bwd-%s-%s" % (tag, k), VR.subsample2_variant, dict(w=shape[3], src=_off(SUB_BWD, k, "dy"), dst=_off(SUB_BWD, k, "dx")), side


@functools.lru_cache(maxsize=None)
def _pool_case(shape, dtype):
    """Distinct inputs (unique maxima, as test_kernels_gpu.py::test_maxpool_same_bf16), small integer gradients (every sum of up
    to four of them is exact in either format) and the float64 y, argmax byte and dx."""
    N, C, H, W = shape
    nc, _, _, Ho, Wo, ph, pw = _pool_geom(shape)
    g = _gen("pool", shape)
    n = N * C * H * W
    p = torch.randperm(n, generator=g)
    bits = 0x3C00 + p % (n // 2) + (p >= n // 2) * 0x8000    # n distinct bf16 patterns: 2^-7 upwards, half of them negative
    x = bits.to(torch.int32).to(torch.int16).view(BF16).reshape(shape).to(dtype).to(DEV)
    assert x.unique().numel() == n and bool(torch.isfinite(x).all())
    dy = torch.randint(-8, 9, (N, C, Ho, Wo), generator=g).to(dtype).to(DEV)
    xr = x.double().requires_grad_(True)
    padded = F.pad(xr, [0, pw, 0, ph], value=-float("inf"))
    y, idx = F.max_pool2d(padded, 3, 2, return_indices=True)
    (dx,) = torch.autograd.grad(y, xr, dy.double())
    hh, ww = idx // (W + pw), idx % (W + pw)
    oh = torch.arange(Ho, device=DEV).view(1, 1, Ho, 1)
    ow = torch.arange(Wo, device=DEV).view(1, 1, 1, Wo)
    amax = ((hh - 2 * oh) * 3 + (ww - 2 * ow)).to(U8)
    return x, dy, y.detach(), amax, dx


def _pool_fns(lib, dtype):
    return ((lib.acr_maxpool3x3s2_fwd_f32, lib.acr_maxpool3x3s2_bwd_f32) if dtype == F32 else
            (lib.acr_maxpool3x3s2_fwd_bf16, lib.acr_maxpool3x3s2_bwd_bf16))


@pytest.mark.parametrize("shape", POOL_SHAPES + [POOL_ODD_H], ids=lambda s: "x".join(map(str, s)))
def test_maxpool_f32_variants(shape):
    """fp32 max-pool forward (four outputs per thread / one) and backward (2 rows x 8 / 8-wide / scalar) with every operand
    aligned and with exactly one of x, y, amax, dy, dx off: y, the argmax bytes and dx equal the float64 reference exactly and
    each other bit for bit.  The odd-height map has no 2x8 geometry: its aligned backward is the 8-wide kernel."""
    L, lib = _lib()
    fwd, bwd = _pool_fns(lib, F32)
    x0, dy0, y_ref, amax_ref, dx_ref = _pool_case(shape, F32)
    nc, H, W, Ho, Wo, _, _ = _pool_geom(shape)
    oshape = (shape[0], shape[1], Ho, Wo)
    outs = {}
    for k, (_, _, side) in POOL_FWD.items():
        x = Placed(shape, F32, _off(POOL_FWD, k, "x"), src=x0)
        y, amax = Placed(oshape, F32, _off(POOL_FWD, k, "y")), Placed(oshape, U8, _off(POOL_FWD, k, "amax"))
        assert VR.maxpool_fwd_variant(4, 0, 0, W, Wo, _mod(x.t), _mod(y.t), _mod(amax.t)) == side
        L.check(fwd(L.ptr(x.t), L.ptr(y.t), L.ptr(amax.t), nc, H, W, Ho, Wo, 0, 0, L.stream_ptr()), "acr_maxpool3x3s2_fwd_f32")
        cmp = KC.Cmp()
        cmp.where = k
        cmp.check("y", y.t, y_ref, **KC.EXACT)
        cmp.check("amax", amax.t, amax_ref, **KC.EXACT)
        _passes(cmp)
        for p in (x, y, amax):
            p.intact()
        outs[k] = (y.t, amax.t)
    for k in outs:
        _same_bits(outs[k][0], outs["aligned"][0], "y, %s vs aligned" % k)
        _same_bits(outs[k][1], outs["aligned"][1], "amax, %s vs aligned" % k)
    dxs = {}
    for k, (_, _, side) in POOL_BWD.items():
        side = "8wide" if (side == "2x8" and shape == POOL_ODD_H) else side
        dy = Placed(oshape, F32, _off(POOL_BWD, k, "dy"), src=dy0)
        amax = Placed(oshape, U8, _off(POOL_BWD, k, "amax"), src=amax_ref)
        dx = Placed(shape, F32, _off(POOL_BWD, k, "dx"))
        assert VR.maxpool_bwd_variant(4, 0, 0, H, W, Ho, Wo, _mod(dy.t), _mod(amax.t), _mod(dx.t)) == side
        L.check(bwd(L.ptr(dy.t), L.ptr(amax.t), L.ptr(dx.t), nc, H, W, Ho, Wo, 0, 0, L.stream_ptr()), "acr_maxpool3x3s2_bwd_f32")
        cmp = KC.Cmp()
        cmp.where = k
        cmp.check("dx", dx.t, dx_ref, **KC.EXACT)
        _passes(cmp)
        for p in (dy, amax, dx):
            p.intact()
        dxs[k] = dx.t
    for k in dxs:
        _same_bits(dxs[k], dxs["aligned"], "dx, %s vs aligned" % k)


@pytest.mark.parametrize("shape", POOL_SHAPES + [POOL_ODD_H], ids=lambda s: "x".join(map(str, s)))
def test_maxpool_bf16_backward_variants(shape):
    """bf16 maps have one forward kernel (test_kernels_gpu.py::test_maxpool_same_bf16) and two backward ones: 8-wide with dx
    aligned, scalar with dx two bytes off."""
    L, lib = _lib()
    fwd, bwd = _pool_fns(lib, BF16)
    x0, dy0, y_ref, amax_ref, dx_ref = _pool_case(shape, BF16)
    nc, H, W, Ho, Wo, _, _ = _pool_geom(shape)
    oshape = (shape[0], shape[1], Ho, Wo)
    y, amax = Placed(oshape, BF16), Placed(oshape, U8)
    L.check(fwd(L.ptr(x0), L.ptr(y.t), L.ptr(amax.t), nc, H, W, Ho, Wo, 0, 0, L.stream_ptr()), "acr_maxpool3x3s2_fwd_bf16")
    cmp = KC.Cmp()
    cmp.check("y", y.t, y_ref, **KC.EXACT)
    cmp.check("amax", amax.t, amax_ref, **KC.EXACT)
    dxs = {}
    for k, (_, _, side) in POOL_BWD_BF16.items():
        dx = Placed(shape, BF16, _off(POOL_BWD_BF16, k, "dx"))
        assert VR.maxpool_bwd_variant(2, 0, 0, H, W, Ho, Wo, _mod(dy0), _mod(amax.t), _mod(dx.t)) == side
        L.check(bwd(L.ptr(dy0), L.ptr(amax.t), L.ptr(dx.t), nc, H, W, Ho, Wo, 0, 0, L.stream_ptr()), "acr_maxpool3x3s2_bwd_bf16")
        cmp.where = k
        cmp.check("dx", dx.t, dx_ref, **KC.EXACT)
        dx.intact()
        dxs[k] = dx.t
    _passes(cmp)
    _same_bits(dxs["dx-off2"], dxs["aligned"], "dx, scalar vs 8-wide")
    y.intact()
    amax.intact()


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_subsample2_variants(shape):
    """subsample2 forward and backward, vector body and (one operand 4 bytes off) scalar body: x[:, :, ::2, ::2] and its autograd
    backward exactly, each other bit for bit.  (The scalar body by W % 8 != 0: test_kernels_gpu.py::test_subsample2.)"""
    L, lib = _lib()
    N, C, H, W = shape
    g = _gen("subsample2", shape)
    x0, dy0 = _rand(g, shape), _rand(g, (N, C, H // 2, W // 2))
    y_ref = x0[:, :, ::2, ::2]
    dx_ref = torch.zeros_like(x0)
    dx_ref[:, :, ::2, ::2] = dy0
    ys, dxs = {}, {}
    for k, (_, _, side) in SUB_FWD.items():
        x, y = Placed(shape, F32, _off(SUB_FWD, k, "x"), src=x0), Placed(dy0.shape, F32, _off(SUB_FWD, k, "y"))
        assert VR.subsample2_variant(W, _mod(x.t), _mod(y.t)) == side
        L.check(lib.acr_subsample2_fwd_f32(L.ptr(x.t), L.ptr(y.t), N * C, H, W, L.stream_ptr()), "acr_subsample2_fwd_f32")
        cmp = KC.Cmp()
        cmp.where = k
        cmp.check("y", y.t, y_ref, **KC.EXACT)
        _passes(cmp)
        x.intact()
        y.intact()
        ys[k] = y.t
    for k, (_, _, side) in SUB_BWD.items():
        dy, dx = Placed(dy0.shape, F32, _off(SUB_BWD, k, "dy"), src=dy0), Placed(shape, F32, _off(SUB_BWD, k, "dx"))
        assert VR.subsample2_variant(W, _mod(dy.t), _mod(dx.t)) == side
        L.check(lib.acr_subsample2_bwd_f32(L.ptr(dy.t), L.ptr(dx.t), N * C, H, W, L.stream_ptr()), "acr_subsample2_bwd_f32")
        cmp = KC.Cmp()
        cmp.where = k
        cmp.check("dx", dx.t, dx_ref, **KC.EXACT)
        _passes(cmp)
        dy.intact()
        dx.intact()
        dxs[k] = dx.t
    for k in ys:
        _same_bits(ys[k], ys["aligned"], "y, %s vs aligned" % k)
    for k in dxs:
        _same_bits(dxs[k], dxs["aligned"], "dx, %s vs aligned" % k)


# ------------------------------------------------------------------------------------------------
# 5. K-split of the small convolution launches: taken only with a 16-byte aligned workspace
# ------------------------------------------------------------------------------------------------
WS_MODES = {"ws": 0, "ws-null": None, "ws-off4": 4}
# 3x3: 32 channels are 18 stages of 16, the fewest that allow two parts of at least 8; 48 outputs take the 64 x 256 tiling of
# the image kernels, 160 the 128 x 128 one with a ragged second tile row.  1x1: 128 channels are two parts of 64.
C3 = dict(N=2, cin=32, H=12, W=20)
C3_COUTS = (48, 160)
S2 = dict(N=2, cin=32, H=24, W=40)                           # its space-to-depth grid is C3's 12 x 20
C1 = dict(N=2, cin=128, H=6, W=8)
C1_COUTS = (20, 132)
KSPLIT_ENTRIES = [("acr_conv3x3_f32", C3, C3_COUTS, 9), ("acr_conv3x3_x3", C3, C3_COUTS, 9), ("acr_conv_taps_x3", S2, C3_COUTS, 9),
                  ("acr_conv1x1_f32", C1, C1_COUTS, 1), ("acr_conv1x1_x3", C1, C1_COUTS, 1)]


def _ksplit_hw(entry, s):
    return (s["H"] // 2) * (s["W"] // 2) if entry == "acr_conv_taps_x3" else s["H"] * s["W"]


def _ksplit_claims():
    for entry, s, couts, ntap in KSPLIT_ENTRIES:
        for cout in couts:
            for k, ws in WS_MODES.items():
                yield ("ksplit-%s-cout%d-%s" % (entry, cout, k), VR.conv_ksplit,
                       dict(entry=entry, ws=ws, nsamp=s["N"], cout=cout, cin=s["cin"], HW=_ksplit_hw(entry, s), ntap=ntap), 2 if k == "ws" else 1)


def _conv_ws(nfloats, mode):
    if mode is None:
        return None
    buf = torch.zeros(int(nfloats) + 4, dtype=F32, device=DEV)
    return buf[mode // 4:]


@pytest.mark.parametrize("cout", C3_COUTS)
@pytest.mark.parametrize("entry", ["acr_conv3x3_f32", "acr_conv3x3_x3", "acr_conv_taps_x3"])
def test_conv3x3_ksplit_by_workspace(entry, cout):
    """The 3x3 convolutions (stride 1 on the packed weight and on its image, stride 2 on the tap table) at the smallest contraction
    that is K-split: with the workspace (two parts, summed by the reduce kernel), without it and with it 4 bytes off (one part,
    written straight to y).  All three vs float64 at KC.TOL["conv"]."""
    from acr_wsss_amd import ops
    L, lib = _lib()
    s = S2 if entry == "acr_conv_taps_x3" else C3
    N, cin, H, W = s["N"], s["cin"], s["H"], s["W"]
    g = _gen("c3", entry, cout)
    x, w = _rand(g, (N, cin, H, W)), _rand(g, (cout, cin, 3, 3), scale=(9 * cin) ** -0.5)
    if entry == "acr_conv_taps_x3":
        plan = ops.conv_s2_plan(3, cin, H, W, x.device)
        H2, W2 = plan.H2, plan.W2
        xs = torch.empty((N, plan.xrows, H2, W2), dtype=F32, device=DEV)
        L.check(lib.acr_space_to_depth2_f32(L.ptr(x), L.ptr(xs), N, cin, H, W, plan.xrows, L.stream_ptr()), "acr_space_to_depth2_f32")
        wi = ops.x3_image(plan.pack(w))
        nws = lib.acr_conv_taps_ws_floats(N, cout, plan.cin, H2, W2, plan.ntap)
    else:
        H2, W2 = H, W
        wp = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()
        wi = ops.x3_image(wp)
        nws = lib.acr_conv3x3_ws_floats(N, cout, cin, H, W)
    assert nws > 0
    for k, mode in WS_MODES.items():
        ws = _conv_ws(nws, mode)
        assert VR.conv_ksplit(entry, _mod(ws), N, cout, cin, H2 * W2) == (2 if k == "ws" else 1)
        y = Placed((N, cout, H2, W2), F32)
        if entry == "acr_conv3x3_f32":
            rc = lib.acr_conv3x3_f32(1, L.ptr(wp), L.ptr(x), L.ptr(y.t), N, cout, cin, H, W, L.ptr(ws), L.stream_ptr())
        elif entry == "acr_conv3x3_x3":
            rc = lib.acr_conv3x3_x3(L.ptr(wi), L.ptr(x), L.ptr(y.t), N, cout, cin, H, W, L.ptr(ws), L.stream_ptr())
        else:
            rc = lib.acr_conv_taps_x3(L.ptr(wi), L.ptr(xs), L.ptr(y.t), N, cout, plan.cin, H2, W2, plan.ntap, plan.fwd[0], plan.fwd[1], plan.fwd[2],
                                      plan.xrows, cout, L.ptr(ws), L.stream_ptr())
        L.check(rc, entry)
        cmp = KC.Cmp()
        cmp.where = k
        KC.verify_conv_same(cmp, x, w, 2 if entry == "acr_conv_taps_x3" else 1, y.t, None, [])
        _passes(cmp)
        y.intact()


@pytest.mark.parametrize("addend", [False, True])
@pytest.mark.parametrize("cout", C1_COUTS)
@pytest.mark.parametrize("entry", ["acr_conv1x1_f32", "acr_conv1x1_f32-transposed", "acr_conv1x1_x3"])
def test_conv1x1_ksplit_by_workspace(entry, cout, addend):
    """The fp32 1x1 convolution under split products (weight as stored, as the forward's (cin, cout) weight, and as an image) at
    the smallest contraction that is K-split: with the workspace (two parts + the part-sum kernel, which also adds the addend),
    without it and with it 4 bytes off (one part, addend in the GEMM epilogue).  vs float64 at KC.TOL["conv1x1"][F32]["y"]."""
    from acr_wsss_amd import ops
    L, lib = _lib()
    N, cin, H, W = C1["N"], C1["cin"], C1["H"], C1["W"]
    hw = H * W
    g = _gen("c1", entry, cout)
    x, w = _rand(g, (N, cin, H, W)), _rand(g, (cout, cin), scale=cin ** -0.5)
    add = _rand(g, (N, cout, H, W)) if addend else None
    transposed = entry.endswith("transposed")
    w2 = w.t().contiguous() if transposed else w
    wi = ops.x3_image(w) if entry == "acr_conv1x1_x3" else None
    name = entry.split("-")[0]
    nws = lib.acr_conv1x1_ws_floats(1, N, cout, cin, hw)
    assert nws > 0
    ref = F.conv2d(x.double(), w.double().view(cout, cin, 1, 1)) + (add.double() if addend else 0)
    for k, mode in WS_MODES.items():
        ws = _conv_ws(nws, mode)
        assert VR.conv_ksplit(name, _mod(ws), N, cout, cin, hw) == (2 if k == "ws" else 1)
        y = Placed((N, cout, H, W), F32)
        if name == "acr_conv1x1_x3":
            rc = lib.acr_conv1x1_x3(L.ptr(wi), L.ptr(x), L.ptr(add), L.ptr(y.t), N, cout, cin, hw, L.ptr(ws), L.stream_ptr())
        else:
            rc = lib.acr_conv1x1_f32(1, L.ptr(w2), int(transposed), L.ptr(x), L.ptr(add), L.ptr(y.t), N, cout, cin, hw, L.ptr(ws), L.stream_ptr())
        L.check(rc, name)
        cmp = KC.Cmp()
        cmp.where = k
        cmp.check("y", y.t, ref, **KC.TOL["conv1x1"][F32]["y"])
        _passes(cmp)
        y.intact()


# ------------------------------------------------------------------------------------------------
# 6. acr_train_cam_f32: 16-byte and 4-byte stores
# ------------------------------------------------------------------------------------------------
TRAINCAM_SHAPES = [(2, 3, 2, 3, 32, 48), (3, 20, 5, 7, 80, 112)]         # ow % 4 == 0 (ow % 4 != 0: test_traincam_gpu.py's 61 x 37)
TRAINCAM_EPS = 1e-5


def _traincam_claims():
    for shape in TRAINCAM_SHAPES:
        for mis, side in ((0, "vec"), (4, "scalar")):
            yield "traincam-%s-out%d" % ("x".join(map(str, shape)), mis), VR.train_cam_variant, dict(ow=shape[5], out=mis), side


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("shape", TRAINCAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_train_cam_store_variants(shape, two, normalize):
    """out on a 16-byte boundary (four values per store) and 4 bytes past one (single stores): the same bits, and those of
    tests/traincam_ref.py's float32 restatement."""
    L, lib = _lib()
    B, C, gh, gw, oh, ow = shape
    cam1, cam2, lab = TCR.make_case(shape, 21 + C)
    want = torch.from_numpy(TCR.cams_f32(cam1, cam2 if two else None, lab, (gh, gw), (oh, ow), TRAINCAM_EPS, normalize)).to(DEV)
    d1, d2, dl = (torch.from_numpy(v).to(DEV) for v in (cam1, cam2, lab))
    nbytes = lib.acr_train_cam_ws_bytes(B, C, oh, ow)
    outs = {}
    for mis, side in ((0, "vec"), (4, "scalar")):
        out = Placed((B, C, oh, ow), F32, mis)
        ws = torch.empty(nbytes, dtype=U8, device=DEV)
        assert VR.train_cam_variant(ow, _mod(out.t)) == side
        L.check(lib.acr_train_cam_f32(L.ptr(d1), L.ptr(d2 if two else None), d1.stride(1), d1.stride(0), L.ptr(dl), B, C, gh, gw, oh, ow,
                                      TRAINCAM_EPS, int(normalize), L.ptr(ws), nbytes, L.ptr(out.t), L.stream_ptr()), "acr_train_cam_f32")
        _same_bits(out.t, want, "%s stores vs the float32 restatement" % side)
        out.intact()
        outs[side] = out.t
    _same_bits(outs["scalar"], outs["vec"], "4-byte vs 16-byte stores")


# ------------------------------------------------------------------------------------------------
# 7. acr_sal_pseudo_compose: four pixels per thread / one
# ------------------------------------------------------------------------------------------------
SAL_CASE = dict(seed=41, b=2, c=5, h=22, w=26, present=[[1, 0, 1, 1, 0], [0, 1, 0, 0, 1]])          # h * w = 572 = 4 * 143
# the misaligned operand -> bytes off (hw % 4 != 0, the other way to the scalar passes: test_pseudo_sal_gpu.py's 33 x 35 case)
SAL_OFF = {"aligned": None, "cams": 4, "saliency": 1, "saliency_out": 1, "label": 1}


def _sal_claims():
    hw = SAL_CASE["h"] * SAL_CASE["w"]
    for k, mis in SAL_OFF.items():
        offs = {n: (mis if n == k else 0) for n in ("cams", "saliency", "saliency_out", "label")}
        yield "sal-pseudo-%s" % k, VR.sal_pseudo_variant, dict(hw=hw, **offs), "vec" if k == "aligned" else "scalar"


@pytest.mark.parametrize("open_size", [0, 10])
def test_sal_pseudo_vector_and_scalar_passes(open_size):
    """Every operand aligned (four values per thread in the histogram and pixel passes) and exactly one of cams, saliency,
    saliency_out, label off (one per thread): labels and saliency output equal the aligned call and tests/pseudo_sal_ref.py."""
    L, lib = _lib()
    cams, present, sal, mg = PSR.decisive_case(**SAL_CASE)
    assert mg > 1e-5
    B, C, h, w = cams.shape
    want, want_sal = PSR.seg_label(cams, present, sal, open_size=open_size)
    d_pres = torch.from_numpy(present).to(DEV)
    nbytes = lib.acr_sal_pseudo_ws_bytes(B, C, h, w)
    got = {}
    for k, mis in SAL_OFF.items():
        off = lambda n: mis if n == k else 0
        dc = Placed(cams.shape, F32, off("cams"), src=torch.from_numpy(cams))
        ds = Placed(sal.shape, U8, off("saliency"), src=torch.from_numpy(sal))
        label, sal_out = Placed(sal.shape, U8, off("label")), Placed(sal.shape, U8, off("saliency_out"))
        ws = torch.full((nbytes,), 0xFF, dtype=U8, device=DEV)
        assert VR.sal_pseudo_variant(h * w, _mod(dc.t), _mod(ds.t), _mod(sal_out.t), _mod(label.t)) == ("vec" if k == "aligned" else "scalar")
        L.check(lib.acr_sal_pseudo_compose(L.ptr(dc.t), L.ptr(d_pres), B, C, h, w, L.ptr(ds.t), 12.0, 0.9, open_size, L.ptr(ws), nbytes,
                                           L.ptr(label.t), L.ptr(sal_out.t), L.stream_ptr()), "acr_sal_pseudo_compose")
        np.testing.assert_array_equal(label.t.cpu().numpy(), want, err_msg="label, " + k)
        np.testing.assert_array_equal(sal_out.t.cpu().numpy(), want_sal, err_msg="saliency, " + k)
        for p in (dc, ds, label, sal_out):
            p.intact()
        got[k] = (label.t, sal_out.t)
    for k in got:
        assert torch.equal(got[k][0], got["aligned"][0]) and torch.equal(got[k][1], got["aligned"][1]), k
