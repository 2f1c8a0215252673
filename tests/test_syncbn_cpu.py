"""BatchNorm2d with cross-rank statistics, the parts that need no GPU: the float64 restatement tests/syncbn_ref.py (moments per rank,
the pairwise merge in rank order, the backward with merged sums) against ``decoder_ref.bn_fwd`` / ``bn_bwd`` on the concatenated
batch; the four ``acr_bn2d_*`` entry points in the header, in ``_lib.SIGNATURES`` and in the library, and what they refuse on the
host; the gather helper on two gloo ranks; and torch's ``convert_sync_batchnorm`` as the switch."""
import ctypes
import datetime
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

import abi_checks
import decoder_ref as R
import syncbn_ref as S
from conftest import ROOT

NEW = {"acr_bn2d_moments": 8, "acr_bn2d_fwd_merged": 20, "acr_bn2d_bwd_sums": 14, "acr_bn2d_bwd_merged": 16}


def _case(name):
    """(shape, split along N, x as float64)"""
    rng = np.random.default_rng(len(name))
    shape, split = {"1+1": ((2, 5, 3, 4), (1, 1)), "2+1": ((3, 5, 3, 4), (2, 1)), "1+2+1": ((4, 5, 3, 4), (1, 2, 1)),
                    "one_value": ((2, 3, 1, 1), (1, 1)), "far_means": ((2, 16, 5, 7), (1, 1)),
                    "mean1000": ((2, 16, 5, 7), (1, 1))}[name]
    x = rng.standard_normal(shape)
    if name == "far_means":
        x[1] += 100.0                                        # the shards' means lie 100 standard deviations apart
    if name == "mean1000":
        x += 1000.0
    return shape, split, x


def _cut(a, split):
    return np.split(a, np.cumsum(split)[:-1], axis=0)


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    err = np.abs(got - want).max()
    assert err <= 1e-12 * np.abs(want).max(), (what, err, np.abs(want).max())


@pytest.mark.parametrize("relu,nres", [(False, 0), (True, 2)])
@pytest.mark.parametrize("name", ["1+1", "2+1", "1+2+1", "one_value", "far_means", "mean1000"])
def test_restatement_equals_batchnorm_of_the_concatenated_batch(name, relu, nres):
    shape, split, x = _case(name)
    rng = np.random.default_rng(7)
    c = shape[1]
    gamma, beta = 1 + 0.1 * rng.standard_normal(c), 0.1 * rng.standard_normal(c)
    rm, rv = rng.standard_normal(c), 0.5 + rng.random(c)
    dy = rng.standard_normal(shape)
    res = [rng.standard_normal(shape) for _ in range(nres)]
    full = R.bn_fwd(x, gamma, beta, rm, rv, True, 0.1, 1e-5, relu, *(res + [None, None])[:2])
    mask = (full["pre"] > 0) if relu else None
    dx, dgamma, dbeta, dres = R.bn_bwd(x, gamma, full["mean"], full["invstd"], dy, True, mask=mask)

    xs = _cut(x, split)
    f = S.fwd(xs, gamma, beta, rm, rv, 0.1, 1e-5, relu, _cut(res[0], split) if nres >= 1 else None,
              _cut(res[1], split) if nres >= 2 else None)
    assert np.array_equal(f["n"], np.full(c, shape[0] * shape[2] * shape[3]))
    for k in ("mean", "invstd", "running_mean", "running_var"):
        _close(f[k], full[k], k)
    _close(np.concatenate(f["y"]), full["y"], "y")
    masks = [p > 0 for p in f["pre"]] if relu else None
    assert not relu or np.array_equal(np.concatenate(masks), mask)
    b = S.bwd(xs, gamma, f["n"], f["mean"], f["invstd"], _cut(dy, split), masks)
    _close(np.concatenate([r[0] for r in b]), dx, "dx")
    _close(sum(r[1] for r in b), dgamma, "dgamma")
    _close(sum(r[2] for r in b), dbeta, "dbeta")
    _close(np.concatenate([r[3] for r in b]), dres, "dres")
    if name == "one_value":                                  # a rank's own n - 1 is 0: only the merged count may be asked for 2
        assert all(m[0, 0] == 1 and (m[:, 2] == 0).all() for m in map(S.moments, xs))
        with pytest.raises(ValueError):
            S.fwd(xs[:1], gamma, beta)
    if name == "far_means":                                  # the delta^2 term carries the variance
        m2_within = sum(S.moments(s)[:, 2] for s in xs)
        assert (S.merge(np.stack([S.moments(s) for s in xs]))[2] > 20 * m2_within).all()


def test_merge_is_the_pairwise_update_in_rank_order():
    rows = np.array([[[3.0, 1.0, 2.0]], [[1.0, 5.0, 0.0]], [[2.0, -1.0, 4.0]]])
    n, mean, m2 = S.merge(rows)
    # by hand: (3, 1, 2) + (1, 5, 0): n 4, delta 4, mean 2, M2 2 + 0 + 16 * 3 / 4 = 14; + (2, -1, 4): n 6, delta -3, mean 1,
    # M2 14 + 4 + 9 * 4 * 2 / 6 = 30
    assert n[0] == 6 and mean[0] == 1.0 and m2[0] == 30.0


def test_new_symbols_are_declared_bound_and_exported():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    for name, nargs in NEW.items():
        params = abi_checks.declared(name)[1]
        res, args = L.SIGNATURES[name]
        assert len(params) == len(args) == nargs and res is ctypes.c_int32, name
        for p, a in zip(params, args):                       # one ctypes type per declared parameter, of the declared kind
            want = (ctypes.c_void_p if "*" in p else {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[p.split()[0]])
            assert a is want, (name, p, a)
        assert getattr(lib, name) is not None
    assert "PER RANK" not in open(os.path.join(ROOT, "acr_wsss_amd", "decoder.py")).read()


def test_c_abi_refuses_bad_arguments_on_the_host():
    from acr_wsss_amd import _lib as L
    lib = L.load()
    p = ctypes.c_void_p(64)                                  # never dereferenced: the arguments are refused first
    big = 1 << 20

    def last():
        return lib.acr_last_error().decode()
    # a merged count of 1: one rank, one value per channel
    assert lib.acr_bn2d_fwd_merged(p, p, p, p, p, None, None, 1, 3, 1, p, 1, 1e-5, 0.1, 0, p, big, p, p, None) == -1 and "1 value" in last()
    assert lib.acr_bn2d_fwd_merged(p, p, p, p, p, None, None, 1, 3, 1, p, 0, 1e-5, 0.1, 0, p, big, p, p, None) == -1 and "W=0" in last()
    assert lib.acr_bn2d_fwd_merged(p, p, p, p, p, None, p, 2, 3, 4, p, 2, 1e-5, 0.1, 0, p, big, p, p, None) == -1 and "resid2" in last()
    assert lib.acr_bn2d_fwd_merged(p, p, p, p, p, None, None, 2, 3, 4, p, 2, 1e-5, 0.1, 0, p, 8, p, p, None) == -1 and "workspace" in last()
    assert lib.acr_bn2d_fwd_merged(p, p, p, p, p, None, None, 2, 3, 4, ctypes.c_void_p(68), 2, 1e-5, 0.1, 0, p, big, p, p, None) == -1
    assert lib.acr_bn2d_moments(p, 0, 3, 1, p, big, p, None) == -1 and "N=0" in last()
    assert lib.acr_bn2d_moments(ctypes.c_void_p(68), 1, 3, 1, p, big, p, None) == -1 and "aligned" in last()
    assert lib.acr_bn2d_moments(p, 1, 3, 1, p, big, None, None) == -1 and "null" in last()
    assert lib.acr_bn2d_bwd_sums(p, None, p, p, 2, 3, 4, 1, p, big, p, None, None, None) == -1 and "saved output" in last()
    assert lib.acr_bn2d_bwd_merged(p, None, p, p, p, p, 2, 2, 3, 4, 0, p, big, p, p, None) == -1 and "dres" in last()
    assert lib.acr_bn2d_bwd_merged(p, None, p, p, p, p, 65537, 2, 3, 4, 0, p, big, p, None, None) == -1 and "W=65537" in last()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist
    from acr_wsss_amd import decoder as D
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    t = torch.arange(15, dtype=torch.float64).reshape(5, 3) + 100.0 * rank + 2.0 ** -40
    a, b = D.gather_rows(t), D.gather_rows(t[:, :2])         # the (C, 3) and the (C, 2) exchange
    out[rank] = (a, b)
    dist.destroy_process_group()


def test_gather_returns_the_rows_in_rank_order_on_both_ranks():
    world, port = 2, _free_port()
    out = mp.Manager().dict()
    mp.spawn(_gather_worker, args=(world, port, out), nprocs=world, join=True)
    base = torch.arange(15, dtype=torch.float64).reshape(5, 3) + 2.0 ** -40
    want = torch.stack([base, base + 100.0])
    for rank in range(world):
        a, b = out[rank]
        assert a.dtype == torch.float64 and tuple(a.shape) == (2, 5, 3) and torch.equal(a, want)
        assert tuple(b.shape) == (2, 5, 2) and torch.equal(b, want[:, :, :2])


def test_convert_sync_batchnorm_is_the_switch_and_keeps_every_key():
    from acr_wsss_amd import decoder as D
    from acr_wsss_amd._lib import AcrHipError
    for make in (lambda: D.make_fusion_block(8, True), lambda: D.SegmentationHead(8, 20)):
        plain = make()
        conv = nn.SyncBatchNorm.convert_sync_batchnorm(make())
        norms = [m for m in conv.modules() if isinstance(m, nn.SyncBatchNorm)]
        assert len(norms) == sum(isinstance(m, nn.BatchNorm2d) for m in plain.modules()) > 0
        assert all(m.process_group is None for m in norms) and type(conv) is type(plain)
        assert list(conv.state_dict()) == list(plain.state_dict())
    # no process group here: the converted norm is taken (today's path; on a CPU tensor that ends at "there is no CPU path")
    x = torch.zeros(2, 4, 3, 3)
    assert D._sync_group(nn.SyncBatchNorm(4)) == (False, None) and D._sync_group(nn.BatchNorm2d(4)) == (False, None)
    with pytest.raises(AcrHipError):
        D.batch_norm_act(x, nn.SyncBatchNorm(4))
    with pytest.raises(NotImplementedError):
        D.batch_norm_act(x, nn.SyncBatchNorm(4, affine=False))
    with pytest.raises(NotImplementedError):
        D.batch_norm_act(x, nn.SyncBatchNorm(4, momentum=None))
    with pytest.raises(NotImplementedError):
        D.batch_norm_act(x, nn.GroupNorm(2, 4))
