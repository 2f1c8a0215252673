"""Data-parallel training step on the GPU: two ranks (sharing cuda:0, collectives over gloo -- RCCL needs one
GPU per rank) each run acr_wsss_amd.train.train_step on half of a batch with GradSync; replicas must stay
identical and match a single process stepping on the whole batch."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _build():
    from acr_wsss_amd.DPT.ACR import ACR
    torch.manual_seed(3)
    m = ACR(num_classes=20, backbone_name="vit_tiny", use_pretrain=False).to("cuda:0")
    with torch.no_grad():                                  # sharper attention than the 0.02-std init
        for blk in m.pretrained.model.blocks:
            blk.attn.qkv.weight.mul_(8.0)
    return m


def _batch():
    g = torch.Generator().manual_seed(11)
    img = torch.randn(4, 3, 64, 64, generator=g)
    label = (torch.rand(4, 20, generator=g) > 0.7).float()
    return img, label


def _worker(rank, world, port, out):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from acr_wsss_amd.dp import GradSync, broadcast_parameters
    from acr_wsss_amd.train import PolyOptimizer, train_step
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _build()
    if rank == 1:
        with torch.no_grad():
            model.cls_head.weight.add_(1.0)                # must be overwritten by the broadcast
    broadcast_parameters(model, 0)
    sync = GradSync(model.parameters(), bucket_mb=4)
    opt = PolyOptimizer(model.parameters(), lr=0.05, weight_decay=5e-4, max_step=10)
    img, label = _batch()
    sl = slice(rank * 2, rank * 2 + 2)
    for _ in range(2):
        loss, _ = train_step(model, opt, img[sl].cuda(), label[sl].cuda(), 125, grad_sync=sync)
    out[rank] = torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])
    out["nb"] = len(sync.buckets)
    dist.destroy_process_group()


def test_two_rank_train_step_matches_single_process():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    assert out["nb"] >= 2
    torch.testing.assert_close(out[0], out[1], rtol=0, atol=0)
    from acr_wsss_amd.train import PolyOptimizer, train_step
    model = _build()
    opt = PolyOptimizer(model.parameters(), lr=0.05, weight_decay=5e-4, max_step=10)
    img, label = _batch()
    for _ in range(2):
        train_step(model, opt, img.cuda(), label.cuda(), 125)
    ref = torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])
    # sign() gradients of the L1 terms make the comparison tolerant, not exact: a 2-sample shard and the 4-sample
    # batch reduce in different orders
    diff = (out[0] - ref).abs()
    assert diff.max() <= 2e-3 * ref.abs().max() and diff.mean() <= 1e-5 * ref.abs().max(), (diff.max(), diff.mean())


def _build_hybrid():
    from acr_wsss_amd.DPT.ACR import ACR
    torch.manual_seed(5)
    m = ACR(num_classes=20, backbone_name="vitb_hybrid", use_pretrain=False, math="f32_split").to("cuda:0")
    with torch.no_grad():
        for blk in m.pretrained.model.blocks:
            blk.attn.qkv.weight.mul_(4.0)
    return m


def _flat_grads(model):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).cpu() for p in model.parameters()])


def _hybrid_worker(rank, world, port, out):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from acr_wsss_amd.dp import GradSync, broadcast_parameters
    from acr_wsss_amd.train import PolyOptimizer, train_step
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # at this small geometry a few stem convolutions still fall to MIOpen (maps narrower than the HIP kernels' tiles), whose
    # default solvers sum with atomics, forward included: held to the deterministic ones as in tests/conftest.py -- measured
    # without it (scripts/lab/step_repeat.py): the SAME step repeated moves the stem's gradients by up to 2 % of their maximum
    torch.backends.cudnn.deterministic = True
    model = _build_hybrid()
    broadcast_parameters(model, 0)
    # exactly what bench.py --gpus N builds: the declared-late stem parameters in the last bucket, static graph
    sync = GradSync(model.parameters(), bucket_mb=64, late_params=model.late_gradient_parameters(), static_graph=True)
    # learning rate 0: the parameters stay put, so EVERY step's averaged gradients -- the learning steps and the static-regime ones
    # alike -- can be held against the single-process full-batch gradient (with a real learning rate this 28-layer random network
    # with sign() gradients amplifies the summation-order difference of the first step chaotically: 3 % after four steps, seen)
    opt = PolyOptimizer(model.parameters(), lr=0.0, weight_decay=5e-4, max_step=10)
    img, label = _batch()
    sl = slice(rank * 2, rank * 2 + 2)
    grads = []
    for _ in range(4):
        train_step(model, opt, img[sl].cuda(), label[sl].cuda(), 125, grad_sync=sync)
        grads.append(_flat_grads(model))
    torch.cuda.synchronize()
    out[rank] = torch.stack(grads)
    if rank == 0:
        late = set(id(p) for p in model.late_gradient_parameters())
        out["info"] = dict(sync.describe(), log=list(sync.launch_log),
                           late_last=[all(id(p) in late for p in b.params) for b in sync.buckets], static=sync._static_ok)
    dist.destroy_process_group()


def test_two_rank_hybrid_late_buckets_static_graph_matches_single_process():
    """the configuration bench.py --gpus N runs -- the HYBRID model (ResNetV2 stem: weight-standardisation launches
    whose backward decides when the stem's gradients exist), `late_params=model.late_gradient_parameters()` and
    `static_graph=True` -- on two ranks (sharing cuda:0 over gloo), four steps: the first learns the gradient-less tensors, the
    second confirms the pattern, the last two run in the static regime (no host rendezvous, the last bucket leaves from
    finish() with the deviation flag).  Every step's gradients: bit-identical on the two ranks and equal to a single process's
    gradient on the whole batch (tolerance: a 2-sample shard and the 4-sample batch reduce in different orders)."""
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_hybrid_worker, args=(world, port, out), nprocs=world, join=True)
    torch.testing.assert_close(out[0], out[1], rtol=0, atol=0)
    info = out["info"]
    nb = info["buckets"]
    assert nb >= 3 and info["late_last"][-1] and not any(info["late_last"][:-1]) and info["static"], info
    assert info["steps"] == 4 and info["agreement_exchanges"] == 2 and info["static_deviations"] == 0 and info["rank_disagreements"] == 0, info
    assert info["late_reexchanges"] == 0 and [i for i, _ in info["log"]] == list(range(nb)), info
    assert info["log"][-1] == (nb - 1, "finish") and all(w == "backward" for _, w in info["log"][:-1]), info["log"]
    assert info["unused_parameters"] == 9                  # the reference's never-used tensors (bkg_token, norm.*, head.*, scratch.*)
    from acr_wsss_amd.train import PolyOptimizer, train_step
    model = _build_hybrid()
    opt = PolyOptimizer(model.parameters(), lr=0.0, weight_decay=5e-4, max_step=10)
    img, label = _batch()
    train_step(model, opt, img.cuda(), label.cuda(), 125)
    ref = _flat_grads(model)
    for it in range(4):
        diff = (out[0][it] - ref).abs()
        print("hybrid DP step %d vs single process: max %.3e mean %.3e of max %.3e" % (it, diff.max(), diff.mean(), ref.abs().max()))
        # (mean: measured 1.6e-7 of max.  The maximum sits in the stem's ill-conditioned gradients -- a 2-sample shard groups a few
        # fp32 sums differently from the 4-sample batch, sign() gradients and 16 bottlenecks of GroupNorm over 4 x 4 maps amplify
        # the last bits: 1.8e-3 of max measured, the same at every step)
        assert diff.max() <= 5e-3 * ref.abs().max() and diff.mean() <= 1e-5 * ref.abs().max(), (it, diff.max(), diff.mean())
        assert torch.equal(out[0][it], out[0][0])          # lr 0 + deterministic kernels: every step repeats the first bit for bit


def _rccl_worker(rank, world, port, out):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from acr_wsss_amd.dp import GradSync, broadcast_parameters
    from acr_wsss_amd.train import PolyOptimizer, train_step
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    t = torch.arange(8, dtype=torch.float32, device="cuda:0")
    dist.all_reduce(t, op=dist.ReduceOp.AVG)                # RCCL's native AVG, the op GradSync uses
    dist.broadcast(t, src=0)
    dist.barrier()
    model = _build()
    broadcast_parameters(model, 0)
    sync = GradSync(model.parameters(), bucket_mb=4, always_reduce=True)
    opt = PolyOptimizer(model.parameters(), lr=0.05, weight_decay=5e-4, max_step=10)
    img, label = _batch()
    for _ in range(2):
        train_step(model, opt, img.cuda(), label.cuda(), 125, grad_sync=sync)
    torch.cuda.synchronize()
    out["t"] = t.cpu()
    out["params"] = torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])
    out["stats"] = dict(sync.stats)
    out["backend"] = dist.get_backend()
    out["nccl"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    dist.destroy_process_group()


def test_rccl_one_rank_group_runs_the_exchange():
    """The box has ONE GPU, so a real multi-rank RCCL run is the driver's; what CAN run here is RCCL itself: a one-rank
    `nccl` process group (= RCCL on ROCm) initialised by this code, its AVG all-reduce / broadcast / barrier, and GradSync's
    bucketed exchange overlapping backward through that backend (the all-reduce of one rank is the identity, so the result
    must equal a plain single-process run)."""
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_rccl_worker, args=(1, port, out), nprocs=1, join=True)
    assert out["backend"] == "nccl" and torch.equal(out["t"], torch.arange(8, dtype=torch.float32))
    assert out["stats"]["steps"] == 2 and out["stats"]["bucket_launches_in_backward"] >= 1 and out["stats"]["rank_disagreements"] == 0
    print("RCCL %s: one-rank group, %s" % (out["nccl"], out["stats"]))
    from acr_wsss_amd.train import PolyOptimizer, train_step
    model = _build()
    opt = PolyOptimizer(model.parameters(), lr=0.05, weight_decay=5e-4, max_step=10)
    img, label = _batch()
    for _ in range(2):
        train_step(model, opt, img.cuda(), label.cuda(), 125)
    ref = torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])
    # same tolerance as the two-rank test: sign() gradients of the L1 terms amplify last-bit differences between two runs
    # (MIOpen's patch-embedding weight gradient is not run-to-run deterministic outside cudnn.deterministic mode)
    diff = (out["params"] - ref).abs()
    assert diff.max() <= 2e-3 * ref.abs().max() and diff.mean() <= 1e-5 * ref.abs().max(), (diff.max(), diff.mean())


def test_bench_plain_run_times_the_headline_only_and_dumps_outputs(tmp_path):
    """A plain `bench.py` run (no --full): the headline's warm-up and timed steps and the result line, nothing else -- no other
    precision, roofline, CAM-generation or CPU-baseline record.  --dump-outputs writes what the last timed step computed, and two
    runs with the same arguments write the same arrays: seeded inputs, and at the bench geometry (448^2, batch 16) a step is
    bit-reproducible from process to process."""
    import json
    import subprocess
    import numpy as np
    recs = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / run)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        recs.append(json.loads(lines[0]))
    rec = recs[0]
    assert rec["dtype"] == "f32_split" and rec["unit"] == "img/s" and rec["higher_is_better"] is True and rec["steps"] == 3
    assert abs(rec["value"] - 16 * 1e3 / rec["ms_per_step"]) <= 0.02 * rec["value"]
    for k in ("f32", "bf16", "roofline", "infer", "cpu_baseline", "dist"):
        assert k not in rec, k
    assert sorted(rec["loss_step0"]) == ["f32_split"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "cls_align.npy", "aff_align.npy", "params_sample.npy", "grads_sample.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == pytest.approx(rec["loss"], rel=1e-4, abs=1e-5)
    assert np.abs(np.load(tmp_path / "a" / "grads_sample.npy")).max() > 0


def test_bench_two_ranks_gloo_rehearsal(tmp_path):
    """bench.py's N > 1 path executed end to end THROUGH ITS SELF-LAUNCH: `python bench.py --gpus 2` with no WORLD_SIZE in the
    environment (the driver's command shape, here with --full) must start the two ranks itself (child torch.distributed.run, one
    process per rank), relay ONE JSON line and return the child's code.  The ranks share cuda:0 with gloo collectives (`--backend gloo`:
    RCCL needs one GPU per rank and the test box has one).  Checks the contract fields: whole-job img/s over both ranks,
    weak scaling, the split-product fp32 headline with the exact-fp32 and bf16 sub-records, `roofline` on the line (rank 0's
    probe; the CPU baseline is switched off here for time, its N > 1 placement is the same code path as N = 1) and the `dist`
    record: what the process group looked like and GradSync's buckets going out inside backward, PER MODE."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "2",
           "--batch", "2", "--size", "224", "--backend", "gloo", "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    assert "self-launch" in out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and rec["dtype"] == "f32_split" and rec["config"]["global_batch"] == 4
    assert rec["config"]["parallelism"] == "dp2" and rec["unit"] == "img/s" and rec["higher_is_better"] is True
    assert abs(rec["value"] - 4 * 1e3 / rec["ms_per_step"]) <= 0.02 * rec["value"]          # whole job: both ranks' images
    assert rec["bf16"]["dtype"] == "bf16" and rec["bf16"]["value"] > 0 and rec["f32"]["dtype"] == "f32" and "infer" not in rec
    for r in (rec["roofline"], rec["f32"]["roofline"], rec["bf16"]["roofline"]):
        assert r["bound"] == "mfma" and 0 < r["frac"] < 1 and r["unit"] == "TFLOP/s" and "kernels" in r
    assert abs(rec["roofline"]["peak"] - 2500.0 / 6) < 0.1 and rec["f32"]["roofline"]["peak"] == 157.3
    d = rec["dist"]
    assert d["backend"] == "gloo" and d["world_size"] == 2 and [r["rank"] for r in d["ranks_devices"]] == [0, 1]
    assert sorted(d["sync"]) == ["bf16", "f32", "f32_split"]
    for m, sy in d["sync"].items():
        assert sy["buckets"] >= 1 and len(sy["bucket_mb"]) == sy["buckets"] and sy["rank_disagreements"] == 0, m
        # step 0 learns the unused tensors (everything from finish()); step 1 confirms the pattern with every bucket going out
        # inside backward; steps 2 and 3 run in the static regime: no host rendezvous, and the LAST bucket (the declared-late
        # gradients + this rank's deviation flag) leaves from finish()
        assert sy["steps_counted"] == 4 and sy["bucket_launches_in_backward"] == 3 * sy["buckets"] - 2, m
        assert sy["bucket_launches_in_finish"] == sy["buckets"] + 2 and sy["late_reexchanges"] == 0, m
        assert sy["static_graph"] is True and sy["host_agreement_exchanges"] == 2 and sy["static_deviations"] == 0, m
        # the diagnostics of an N > 1 run: the step with the exchange disarmed and the exchange on its own
        assert sy["ms_step"] > 0 and sy["ms_compute_only"] > 0 and sy["ms_allreduce_only"] > 0 and sy["allreduce_mb"] > 300 * (0.5 if m == "bf16" else 1), (m, sy)
        assert abs(sy["exposed_ms"] - (sy["ms_step"] - sy["ms_compute_only"])) < 1e-2 and sy["allreduce_busbw_gbs"] > 0, (m, sy)
    assert rec["loss_step0_agree"] is True and 0 <= rec["loss_step0_max_rel"] <= 5e-5
    # a wrong WORLD_SIZE is still an error, not a silent single-rank run
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                         cwd=str(tmp_path))
    assert bad.returncode != 0
