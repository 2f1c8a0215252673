"""BatchNorm2d with cross-rank statistics on the device: the four ``acr_bn2d_*`` entry points with the ranks emulated in one process,
an ``nn.SyncBatchNorm`` outside a process group against an ``nn.BatchNorm2d``, and two ranks (sharing cuda:0, collectives over
gloo) on one fusion block and on the whole ``seg=True`` model under ``GradSync``.

Kernel level: the rule of tests/test_decoder_gpu.py, nothing fixed in advance -- the device's error against the float64 restatement
of the FULL batch may be at most 2x the error torch's CPU fp32 ``BatchNorm2d`` shows on that full batch, with a floor of 4 fp32
ulps of the largest value; a fused ReLU only on decisive inputs, asserted.
Block level: 2e-4 of the maximum for activations and 2e-3 for gradients, the bounds test_decoder_gpu.py uses there.
Model level: max <= 5e-3 and mean <= 1e-5 of the reference's maximum, the bound tests/test_dp_gpu.py holds the hybrid two-rank
step to (its measured allowance for shard-versus-batch summation order through the same stem)."""
import datetime
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

import decoder_ref as R
from conftest import load_golden
from kernel_checks import Cmp
from test_decoder_gpu import BN_SHAPES, EPS, MARGIN, MOMENTUM, bn_case, compare

pytestmark = pytest.mark.gpu

DEV = "cuda"
# tag -> how the batch is cut along N into ranks: equal and unequal counts, C = 300, several slabs, W = 3 on the aligned path
SPLITS = {"odd": (1, 1), "gen": (2, 1), "chan": (1, 1), "slabs": (1, 1), "wide": (1, 2, 1), "mean1000": (1, 1)}
# one value per channel per rank (a local n - 1 is 0), and shards whose means lie 100 standard deviations apart
EXTRA = {"one_value": ((2, 3, 1, 1), (1, 1)), "far_means": ((2, 16, 5, 7), (1, 1))}
# seeds for which the ReLU inputs of the two extra cases are decisive (found on the CPU; asserted)
EXTRA_SEEDS = {("one_value", True): 0, ("far_means", True): 0}
assert set(SPLITS) <= set(BN_SHAPES)


@functools.lru_cache(maxsize=None)
def extra_case(name, relu, nres):
    """``bn_case`` for the shapes of EXTRA: inputs, the float64 restatement and torch's CPU fp32 result on the full batch"""
    shape, _ = EXTRA[name]
    rng = np.random.default_rng(1000 * EXTRA_SEEDS.get((name, relu), 0) + len(name) + 7 * nres)
    c = shape[1]
    x = rng.standard_normal(shape)
    if name == "far_means":
        x[1] += 100.0
    x = x.astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    res = [rng.standard_normal(shape).astype(np.float32) for _ in range(nres)]
    gamma, beta = (1 + 0.1 * rng.standard_normal(c)).astype(np.float32), (0.1 * rng.standard_normal(c)).astype(np.float32)
    rm, rv = (0.2 * rng.standard_normal(c)).astype(np.float32), (0.5 + rng.random(c)).astype(np.float32)
    f = R.bn_fwd(x, gamma, beta, rm, rv, True, MOMENTUM, EPS, relu, *(res + [None, None])[:2])
    dx, dgamma, dbeta, dres = R.bn_bwd(x, gamma, f["mean"], f["invstd"], dy, True, mask=(f["pre"] > 0) if relu else None)
    ref = dict(y=f["y"], running_mean=f["running_mean"], running_var=f["running_var"], dx=dx, dgamma=dgamma, dbeta=dbeta, dres=dres)
    bn = nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM).train()
    with torch.no_grad():
        for t, v in ((bn.weight, gamma), (bn.bias, beta), (bn.running_mean, rm), (bn.running_var, rv)):
            t.copy_(torch.from_numpy(v))
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    rt = [torch.from_numpy(r).clone().requires_grad_(True) for r in res]
    pre = bn(xt)
    for r in rt:
        pre = pre + r
    yt = F.relu(pre) if relu else pre
    yt.backward(torch.from_numpy(dy))
    tor = dict(y=yt.detach(), running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(), dx=xt.grad, dgamma=bn.weight.grad,
               dbeta=bn.bias.grad, dres=rt[0].grad if rt else None)
    decisive = True
    if relu:
        dev = float(np.abs(pre.detach().numpy().astype(np.float64) - f["pre"]).max())
        decisive = float(np.abs(f["pre"]).min()) > MARGIN * dev
    return dict(x=x, dy=dy, res=res, gamma=gamma, beta=beta, rm=rm, rv=rv, ref=ref, tor=tor, decisive=decisive)


def _case(tag, relu, nres):
    if tag in EXTRA:
        return extra_case(tag, relu, nres), EXTRA[tag][1]
    return bn_case(tag, relu, nres), SPLITS[tag]


def run_sharded(case, split, relu):
    """The four entry points on the shards of ``case`` cut along N by ``split``, the gathered rows stacked by hand.  Per rank:
    y, dx, dres, dgamma, dbeta, stats, running_mean, running_var (CPU tensors)."""
    from acr_wsss_amd import _lib as L
    lib = L.load()
    cuts = np.cumsum(split)[:-1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xs = [dev(a) for a in np.split(case["x"], cuts)]
    dys = [dev(a) for a in np.split(case["dy"], cuts)]
    res = [[dev(a) for a in np.split(r, cuts)] for r in case["res"]]
    gamma, beta = dev(case["gamma"]), dev(case["beta"])
    c, hw, W = xs[0].shape[1], xs[0].shape[2] * xs[0].shape[3], len(split)
    st = L.stream_ptr()
    wss = [torch.empty(lib.acr_bn2d_ws_bytes(x.shape[0], c, hw), dtype=torch.uint8, device=DEV) for x in xs]
    moments = []
    for x, ws in zip(xs, wss):
        m = torch.empty(c, 3, dtype=torch.float64, device=DEV)
        assert lib.acr_bn2d_moments(L.ptr(x), x.shape[0], c, hw, L.ptr(ws), ws.numel(), L.ptr(m), st) == 0, lib.acr_last_error()
        moments.append(m)
    gathered = torch.stack(moments)
    ranks = []
    for r, (x, ws) in enumerate(zip(xs, wss)):
        rm, rv = dev(case["rm"]), dev(case["rv"])
        stats, y = torch.empty(3 * c, dtype=torch.float64, device=DEV), torch.empty_like(x)
        r1 = res[0][r] if len(res) >= 1 else None
        r2 = res[1][r] if len(res) >= 2 else None
        rc = lib.acr_bn2d_fwd_merged(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(r1), L.ptr(r2), x.shape[0], c, hw,
                                     L.ptr(gathered), W, EPS, MOMENTUM, int(relu), L.ptr(ws), ws.numel(), L.ptr(stats), L.ptr(y), st)
        assert rc == 0, lib.acr_last_error()
        ranks.append(dict(y=y, stats=stats, running_mean=rm, running_var=rv))
    sums = []
    for x, dy, ws, k in zip(xs, dys, wss, ranks):
        s = torch.empty(c, 2, dtype=torch.float64, device=DEV)
        k["dgamma"], k["dbeta"] = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        rc = lib.acr_bn2d_bwd_sums(L.ptr(x), L.ptr(k["y"]) if relu else None, L.ptr(dy), L.ptr(k["stats"]), x.shape[0], c, hw, int(relu),
                                   L.ptr(ws), ws.numel(), L.ptr(s), L.ptr(k["dgamma"]), L.ptr(k["dbeta"]), st)
        assert rc == 0, lib.acr_last_error()
        sums.append(s)
    gsums = torch.stack(sums)
    for x, dy, ws, k in zip(xs, dys, wss, ranks):
        k["dx"] = torch.empty_like(x)
        k["dres"] = torch.empty_like(x) if relu else None
        rc = lib.acr_bn2d_bwd_merged(L.ptr(x), L.ptr(k["y"]) if relu else None, L.ptr(dy), L.ptr(gamma), L.ptr(k["stats"]), L.ptr(gsums), W,
                                     x.shape[0], c, hw, int(relu), L.ptr(ws), ws.numel(), L.ptr(k["dx"]), L.ptr(k["dres"]), st)
        assert rc == 0, lib.acr_last_error()
    torch.cuda.synchronize()
    return [{n: (None if v is None else v.cpu()) for n, v in k.items()} for k in ranks]


@pytest.mark.parametrize("relu,nres", [(False, 0), (True, 2)])
@pytest.mark.parametrize("tag", sorted(SPLITS) + sorted(EXTRA))
def test_emulated_ranks_equal_the_full_batch(tag, relu, nres):
    case, split = _case(tag, relu, nres)
    assert case["decisive"], "the ReLU inputs of %s are not decisive: pick another seed" % ((tag, relu, nres),)
    ranks = run_sharded(case, split, relu)
    ref, tor = case["ref"], case["tor"]
    cmp = Cmp()
    cmp.where = "syncbn %s %s relu%d res%d" % (tag, "+".join(map(str, split)), relu, nres)
    compare(cmp, "y", torch.cat([k["y"] for k in ranks]), tor["y"], ref["y"])
    compare(cmp, "dx", torch.cat([k["dx"] for k in ranks]), tor["dx"], ref["dx"])
    if relu:
        compare(cmp, "dres", torch.cat([k["dres"] for k in ranks]), tor["dres"], ref["dres"])
    compare(cmp, "sum dgamma", sum(k["dgamma"].double() for k in ranks), tor["dgamma"], ref["dgamma"])
    compare(cmp, "sum dbeta", sum(k["dbeta"].double() for k in ranks), tor["dbeta"], ref["dbeta"])
    compare(cmp, "running_mean", ranks[0]["running_mean"], tor["running_mean"], ref["running_mean"])
    compare(cmp, "running_var", ranks[0]["running_var"], tor["running_var"], ref["running_var"])
    assert not cmp.failures, "\n".join(cmp.failures)
    # every rank was fed the same gathered buffer: the same bits, and the merged count is exact
    shape = case["x"].shape
    for k in ranks[1:]:
        for name in ("stats", "running_mean", "running_var"):
            assert k[name].numpy().tobytes() == ranks[0][name].numpy().tobytes(), name
    assert torch.equal(ranks[0]["stats"][2 * shape[1]:], torch.full((shape[1],), float(shape[0] * shape[2] * shape[3]), dtype=torch.float64))
    if tag == "far_means":
        assert float(case["ref"]["running_var"].max()) > 100                    # the delta^2 term carried the variance
    if tag == "mean1000":
        assert abs(float(case["x"].mean()) - 1000) < 1


def test_repeat_is_bit_identical_and_a_merged_count_of_one_is_refused():
    from acr_wsss_amd import _lib as L
    case, split = _case("slabs", True, 2)
    one, two = run_sharded(case, split, True), run_sharded(case, split, True)
    for a, b in zip(one, two):
        for name in a:
            assert a[name].numpy().tobytes() == b[name].numpy().tobytes(), name
    lib = L.load()
    x = torch.zeros(1, 3, 1, 1, device=DEV)
    bn = nn.BatchNorm2d(3).to(DEV)
    ws = torch.empty(lib.acr_bn2d_ws_bytes(1, 3, 1), dtype=torch.uint8, device=DEV)
    m, stats, y = torch.empty(1, 3, 3, dtype=torch.float64, device=DEV), torch.empty(9, dtype=torch.float64, device=DEV), torch.empty_like(x)
    assert lib.acr_bn2d_moments(L.ptr(x), 1, 3, 1, L.ptr(ws), ws.numel(), L.ptr(m), L.stream_ptr()) == 0          # n = 1 is legal here
    assert torch.equal(m.cpu(), torch.tensor([[[1.0, 0.0, 0.0]] * 3], dtype=torch.float64))
    rc = lib.acr_bn2d_fwd_merged(L.ptr(x), L.ptr(bn.weight), L.ptr(bn.bias), L.ptr(bn.running_mean), L.ptr(bn.running_var), None, None, 1, 3,
                                 1, L.ptr(m), 1, 1e-5, 0.1, 0, L.ptr(ws), ws.numel(), L.ptr(stats), L.ptr(y), L.stream_ptr())
    assert rc == -1                                                              # ACR_ERR_INVALID
    assert torch.equal(bn.running_mean.cpu(), torch.zeros(3)) and torch.equal(bn.running_var.cpu(), torch.ones(3))


# ------------------------------------------------------------------------------------------------
# an nn.SyncBatchNorm that does not exchange: the bits of an nn.BatchNorm2d
# ------------------------------------------------------------------------------------------------
def _module_run(cls, case, relu, training):
    from acr_wsss_amd import decoder as D
    bn = cls(case["x"].shape[1], eps=EPS, momentum=MOMENTUM).to(DEV).train(training)
    with torch.no_grad():
        for t, v in ((bn.weight, case["gamma"]), (bn.bias, case["beta"]), (bn.running_mean, case["rm"]), (bn.running_var, case["rv"])):
            t.copy_(torch.from_numpy(v))
    x = torch.from_numpy(case["x"]).to(DEV).requires_grad_(True)
    res = [torch.from_numpy(r).to(DEV).requires_grad_(True) for r in case["res"]]
    y = D.batch_norm_act(x, bn, "relu" if relu else "none", *res)
    y.backward(torch.from_numpy(case["dy"]).to(DEV))
    out = dict(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var,
               tracked=bn.num_batches_tracked)
    out.update({"dres%d" % i: r.grad for i, r in enumerate(res)})
    return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("tag,relu,nres", [("gen", False, 0), ("slabs", True, 2)])
def test_without_a_process_group_syncbatchnorm_is_batchnorm_bit_for_bit(tag, relu, nres, training):
    import torch.distributed as dist
    assert not dist.is_initialized()
    case = bn_case(tag, relu, nres)
    plain, conv = _module_run(nn.BatchNorm2d, case, relu, training), _module_run(nn.SyncBatchNorm, case, relu, training)
    assert plain.keys() == conv.keys() and len(plain) == 7 + nres
    for k in plain:
        assert plain[k] == conv[k], k
    assert np.frombuffer(conv["tracked"], np.int64)[0] == (1 if training else 0)


# ------------------------------------------------------------------------------------------------
# two ranks sharing cuda:0 over gloo
# ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _init(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    # 60 s: a collective one rank never issues raises instead of hanging
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    torch.backends.cudnn.deterministic = True              # as tests/conftest.py and test_dp_gpu.py::_hybrid_worker


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _block_run(fx, rows, convert):
    """The "a" fixture's block on the rows ``rows`` of its batch -> out, input gradients, parameter gradients, running statistics"""
    from test_decoder_gpu import _block
    blk = _block(fx, "f32").train()
    if convert:
        blk = nn.SyncBatchNorm.convert_sync_batchnorm(blk)
        assert sum(isinstance(m, nn.SyncBatchNorm) for m in blk.modules()) == 4
    xs = [torch.from_numpy(fx["x%d" % i][rows]).to(DEV).requires_grad_(True) for i in range(2)]
    out = blk(*xs)
    out.backward(torch.from_numpy(fx["dy"][rows]).to(DEV))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), dx=[x.grad.cpu() for x in xs], grads={k: p.grad.cpu() for k, p in blk.named_parameters()},
                running={k: v.cpu() for k, v in blk.state_dict().items() if "running_" in k})


def _block_worker(rank, world, port, out):
    import torch.distributed as dist
    _init(rank, world, port)
    fx = load_golden("decoder_block_a")
    rows = slice(rank, rank + 1)
    out[("plain", rank)] = _block_run(fx, rows, False)      # the control: per-rank statistics
    out[("sync", rank)] = _block_run(fx, rows, True)
    dist.destroy_process_group()


def test_two_ranks_one_fusion_block_equals_the_single_process_batch():
    fx = load_golden("decoder_block_a")
    assert fx["x0"].shape[0] == 2 and (fx["relu_min64"] > MARGIN * fx["relu_dev32"]).all()
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_block_worker, args=(world, port, out), nprocs=world, join=True)
    one = _block_run(fx, slice(0, 2), False)                 # one process, the unconverted block, the whole batch
    sync, plain = [out[("sync", r)] for r in range(world)], [out[("plain", r)] for r in range(world)]
    worst = {"out": _rel(torch.cat([s["out"] for s in sync]), one["out"]),
             "control out": _rel(torch.cat([s["out"] for s in plain]), one["out"])}
    for i in range(2):
        worst["dx%d" % i] = _rel(torch.cat([s["dx"][i] for s in sync]), one["dx"][i])
    # parameter gradients averaged over the ranks against the single process fed dy / 2 (its gradients are linear in dy)
    for k, g in one["grads"].items():
        worst["grad " + k] = _rel((sync[0]["grads"][k] + sync[1]["grads"][k]) / 2, g / 2)
    print("two-rank fusion block: %s" % {k: "%.2e" % v for k, v in worst.items() if not k.startswith("grad")},
          "worst grad %.2e" % max(v for k, v in worst.items() if k.startswith("grad")))
    assert worst["out"] <= 2e-4, worst
    assert all(v <= 2e-3 for k, v in worst.items() if k.startswith(("dx", "grad"))), worst
    assert len(one["grads"]) == 14
    # the control: per-rank statistics miss the activation bound by far, so these inputs do show the feature
    assert worst["control out"] >= 10 * 2e-4, worst
    # running statistics: the same bits on both ranks, and against the float64 fixture no further off than the kernel rule
    # allows with the single process in the place of torch's fp32 result
    cmp = Cmp()
    cmp.where = "two-rank fusion block"
    for k, v in sync[0]["running"].items():
        assert v.numpy().tobytes() == sync[1]["running"][k].numpy().tobytes(), k
        compare(cmp, k, v, one["running"][k], fx["after64:" + k])
    assert len(sync[0]["running"]) == 8 and not cmp.failures, "\n".join(cmp.failures)


def _seg_build():
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd.backbone import set_math
    from acr_wsss_amd.DPT.ACR import ACR
    torch.manual_seed(5)
    model = ACR(20, "vitb_hybrid", seg=True, features=16, use_pretrain=False, math="f32_split").to("cuda:0").train()
    head = set_math(D.SegmentationHead(16, 20).to("cuda:0").train(), "f32_split")
    head[3].p = 0.0                                          # Dropout draws per process: a shard and the batch would see other masks
    return model, head


def _seg_batch():
    """4 images at 64 x 64.  The cross-entropy is a mean over the background pixels plus a mean over the foreground pixels of the
    batch: the ranks' averaged gradients are the batch's only if every rank holds as many of each.  Images 2, 3 carry the label
    maps of images 0, 1 transposed, with the foreground classes renamed; no pixel is ignored."""
    g = torch.Generator().manual_seed(11)
    images = torch.randn(4, 3, 64, 64, generator=g)
    half = torch.randint(0, 21, (2, 64, 64), generator=g)
    other = half.transpose(1, 2)
    label = torch.cat([half, torch.where(other > 0, 21 - other, other)]).to(torch.uint8)
    ori = torch.randint(0, 256, (4, 3, 64, 64), generator=g).to(torch.uint8)
    return images, ori, torch.ones(64, 64, 4), label


def _seg_step(model, head, opt, rows, sync=None):
    from acr_wsss_amd.segtrain import seg_train_step
    images, ori, crop, label = _seg_batch()
    seg_train_step(model, head, opt, images[rows].cuda(), ori[rows].cuda(), crop[:, :, rows].cuda(), label[rows].cuda(), None, grad_sync=sync)
    torch.cuda.synchronize()
    named = [(k, p) for k, p in model.named_parameters()] + [("head." + k, p) for k, p in head.named_parameters()]
    flat = lambda pick: torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).cpu()
                                   for k, p in named if pick(k)])
    decoder = lambda k: k.startswith(("scratch.", "head."))
    return dict(decoder=flat(decoder), rest=flat(lambda k: not decoder(k)), names=[(k, p.numel()) for k, p in named if decoder(k)])


def _seg_worker(rank, world, port, out):
    import torch.distributed as dist
    from acr_wsss_amd.dp import GradSync, broadcast_parameters
    from acr_wsss_amd.train import PolyOptimizer
    _init(rank, world, port)
    model, head = _seg_build()
    if rank == 1:
        with torch.no_grad():
            head[4].weight.add_(1.0)                         # must be overwritten by the broadcast
    broadcast_parameters(model, 0)
    broadcast_parameters(head, 0)
    params = list(model.parameters()) + list(head.parameters())
    sync = GradSync(params)
    opt = PolyOptimizer(params, lr=0.0, weight_decay=5e-4, max_step=10)          # learning rate 0: the parameters stay put
    rows = slice(2 * rank, 2 * rank + 2)
    out[("plain", rank)] = _seg_step(model, head, opt, rows, sync)               # the control: per-rank statistics
    model, head = nn.SyncBatchNorm.convert_sync_batchnorm(model), nn.SyncBatchNorm.convert_sync_batchnorm(head)
    assert sum(isinstance(m, nn.SyncBatchNorm) for m in list(model.modules()) + list(head.modules())) == 17
    out[("sync", rank)] = _seg_step(model, head, opt, rows, sync)
    dist.destroy_process_group()


def test_two_ranks_seg_train_step_equals_the_single_process_batch():
    """One ``seg_train_step`` (cross-entropy alone, learning rate 0) of the hybrid ``seg=True`` model and its head on two ranks with
    2 images each, after ``convert_sync_batchnorm`` and under ``GradSync``: the averaged gradients are the same bits on both
    ranks and those of one process on the 4-image batch with plain BatchNorm, within max <= 5e-3 and mean <= 1e-5 of the
    reference's maximum -- for the decoder and head parameters and for the rest apart.  The control, the same step before the
    conversion, must miss the decoder group's bound by 10x at least; the bound has two parts and the control misses it by the
    larger of the two factors.  Measured on an MI355X in two runs: cross-rank, decoder group max 6.5e-8 and 2.2e-5 / mean 2.7e-9
    and 1.1e-6, the rest max 1.8e-6 and 6.2e-4 / mean 1.8e-10 and 7.1e-8; per-rank (the control), decoder group max 1.27e-2
    (2.5x its part) / mean 1.37e-3 (137x its part), the rest 7.0e-1 / 8.4e-5.  The maximum part is insensitive because it is taken relative to the group's largest gradient, and that gradient
    is ``head.4.bias``'s, which the statistics barely move, while the many small gradients of the decoder's convolutions, which the
    statistics move by their own size, carry the mean (the test prints where the largest gradient and the largest deviation sit)"""
    from acr_wsss_amd.train import PolyOptimizer
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_seg_worker, args=(world, port, out), nprocs=world, join=True)
    model, head = _seg_build()
    params = list(model.parameters()) + list(head.parameters())
    ref = _seg_step(model, head, PolyOptimizer(params, lr=0.0, weight_decay=5e-4, max_step=10), slice(0, 4))
    ratios = {}
    for kind in ("sync", "plain"):
        for group in ("decoder", "rest"):
            assert torch.equal(out[(kind, 0)][group], out[(kind, 1)][group]), (kind, group)      # the same bits on both ranks
            diff, top = (out[(kind, 0)][group] - ref[group]).abs(), float(ref[group].abs().max())
            assert top > 0
            ratios[(kind, group)] = (float(diff.max()) / top, float(diff.mean()) / top)
            print("two-rank seg step, %s BatchNorm, %s parameters (%d values): max %.3e mean %.3e of the reference's maximum %.3e"
                  % ("cross-rank" if kind == "sync" else "per-rank", group, diff.numel(), *ratios[(kind, group)], top))
    for group in ("decoder", "rest"):
        assert ratios[("sync", group)][0] <= 5e-3 and ratios[("sync", group)][1] <= 1e-5, (group, ratios[("sync", group)])
    # where the decoder group's largest gradient and the control's largest deviation sit
    off, spans = 0, {}
    for k, n in ref["names"]:
        spans[k], off = (off, off + n), off + n
    at = lambda i: next(k for k, (a, b) in spans.items() if a <= i < b)
    cdiff = (out[("plain", 0)]["decoder"] - ref["decoder"]).abs()
    print("decoder group: largest reference gradient in %s, the control's largest deviation in %s"
          % (at(int(ref["decoder"].abs().argmax())), at(int(cdiff.argmax()))))
    miss = max(ratios[("plain", "decoder")][0] / 5e-3, ratios[("plain", "decoder")][1] / 1e-5)
    assert miss >= 10, ratios[("plain", "decoder")]
