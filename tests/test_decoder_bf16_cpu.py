"""What the bf16 decoder needs that a machine without a GPU can check: the ten ``*_bf16`` entry points in the header and in the
derived binding, ``train.MasterWeights`` leaving a BatchNorm's buffers fp32, and the yardstick of tests/test_decoder_bf16_gpu.py
(tests/decoder_bf16_checks.py) on synthetic values with a known verdict."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

import abi_checks
import decoder_bf16_checks as K

NEW = ("acr_bn2d_fwd_bf16", "acr_bn2d_bwd_bf16", "acr_bn2d_moments_bf16", "acr_bn2d_fwd_merged_bf16", "acr_bn2d_bwd_sums_bf16",
       "acr_bn2d_bwd_merged_bf16", "acr_relu_fwd_bf16", "acr_relu_bwd_bf16", "acr_upsample2x_fwd_bf16", "acr_upsample2x_bwd_bf16")
BF16_ARGS = {"x", "y", "resid", "resid2", "dy", "dx", "dres", "gamma", "beta"}
FLOAT_ARGS = {"running_mean", "running_var", "dgamma", "dbeta"}
DOUBLE_ARGS = {"stats", "moments", "gathered", "sums", "gathered_sums"}


def twin(name):
    return name[:-5] if not name.startswith("acr_relu") else name[:-5] + "_f32"


def test_the_ten_entry_points_are_declared_and_bound_with_the_stated_types():
    from acr_wsss_amd import _abi
    abi_checks.check_bound(NEW, _abi.prototypes)
    for name in NEW:
        ret, params = abi_checks.declared(name)
        fret, fparams = abi_checks.declared(twin(name))
        assert ret == fret == "int" and params[-1] == "void* stream"
        assert [p.split()[-1].lstrip("*") for p in params] == [p.split()[-1].lstrip("*") for p in fparams], name      # the fp32 argument list
        res, args = _abi.prototypes[name]
        assert res is ctypes.c_int32 and len(args) == len(params)
        for p, fp, a in zip(params, fparams, args):
            arg = p.split()[-1].lstrip("*")
            ctype = p[:p.rindex(arg)].replace(" ", "")
            if arg in BF16_ARGS:
                assert ctype in ("constvoid*", "void*") and a is ctypes.c_void_p, (name, p)
                assert ("const" in ctype) == ("const" in fp), (name, p)
            elif arg in FLOAT_ARGS:
                assert ctype == "float*" and a is ctypes.c_void_p, (name, p)
            elif arg in DOUBLE_ARGS:
                assert ctype in ("double*", "constdouble*") and a is ctypes.c_void_p, (name, p)
            else:
                assert " ".join(p.split()) == " ".join(fp.split()), (name, p, fp)           # scalars, ws and stream as in fp32
                assert a is abi_checks.ctype_of(p.rsplit(None, 1)[0] if "*" not in p else p[:p.rindex("*") + 1]), (name, p)
    assert "double -> fp32 -> bf16" in abi_checks.HEADER                                     # the definition is written down


def test_master_weights_leaves_batchnorm_buffers_fp32():
    from acr_wsss_amd.train import MasterWeights, PolyOptimizer

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.bn = nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4)
            self.register_buffer("scale", torch.ones(4))

    m = Tiny()
    m.bn.num_batches_tracked.fill_(3)
    rv = torch.rand(4) + 0.5
    m.bn.running_var.copy_(rv)
    mw = MasterWeights(m, lambda ps: PolyOptimizer(ps, lr=0.01, weight_decay=0, max_step=10))
    assert all(p.dtype == torch.bfloat16 for p in m.parameters()) and all(x.dtype == torch.float32 for x in mw.masters)
    assert m.bn.running_mean.dtype == torch.float32 and m.bn.running_var.dtype == torch.float32
    assert torch.equal(m.bn.running_var, rv)                                                # not rounded on the way either
    assert m.bn.num_batches_tracked.dtype == torch.int64 and int(m.bn.num_batches_tracked) == 3
    assert m.scale.dtype == torch.bfloat16                                                  # any other floating buffer as before
    assert len(mw.masters) == 4                                                             # conv weight / bias, norm weight / bias


def test_rne_matches_torch():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.integers(-20, 20, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625], np.float32)])   # ties to even on both sides
    want = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(K.bf16_rne(a), want)
    assert np.array_equal(K.bf16_to_f32(want), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)


def test_the_acceptance_rule_on_values_with_a_known_verdict():
    up, down = 0x3F81, 0x3F80                                # the bf16 neighbours 1.0078125 and 1.0
    inside = _f32((down << 16) | 0x8000 | 3)                 # 3 fp32 ulps above the midpoint: rounds up, the lower neighbour is tolerated
    edge = _f32((down << 16) | 0x8000 - K.WINDOW)            # exactly WINDOW ulps below it: still inside
    outside = _f32((down << 16) | 0x8000 + K.WINDOW + 1)     # one ulp past the window: only RNE will do
    assert K.in_window(inside)[0] and K.in_window(edge)[0] and not K.in_window(outside)[0]
    assert K.bf16_rne(inside)[0] == up and K.bf16_rne(edge)[0] == down and K.bf16_rne(outside)[0] == up
    # a tensor of 2000 exact elements plus the probe: the cap of 1e-3 admits 2 exemptions
    fill = np.full(2000, 1.0, np.float32)
    ref = np.concatenate([fill, inside])
    good = np.concatenate([K.bf16_rne(fill), [up]]).astype(np.uint16)
    r = K.accept_bf16(good, ref)
    assert r["ok"] and r["exact"] == 2001 and r["exempt"] == 0
    other = good.copy()
    other[-1] = down
    r = K.accept_bf16(other, ref)
    assert r["ok"] and r["exempt"] == 1 and r["wrong"] == 0
    # the same wrong neighbour outside the window is an error ...
    r = K.accept_bf16(other, np.concatenate([fill, outside]))
    assert not r["ok"] and r["wrong"] == 1
    # ... as is a value two bf16 steps away inside it, and an exemption beyond the cap (1 of 10 elements)
    far = good.copy()
    far[-1] = down - 1
    assert not K.accept_bf16(far, ref)["ok"]
    r = K.accept_bf16(other[-10:], ref[-10:])
    assert r["wrong"] == 0 and r["exempt"] == 1 and not r["ok"]
    # negative values mirror; a zero may carry either sign
    r = K.accept_bf16(np.array([down | 0x8000, 0x8000], np.uint16), np.concatenate([-inside, [0.0]]).astype(np.float32))
    assert r["wrong"] == 0 and r["exempt"] == 1 and r["exact"] == 1
    assert abs(K.window_share(np.random.default_rng(1).standard_normal(1 << 20)) - 9 / 65536) < 5e-5


def test_double_and_float_rules():
    a = np.array([1.0, 2.0, 3.0])
    r = K.close_f64(a, a + np.array([0.0, 1e-15, 0.0]), 2e-15)
    assert r["ok"] and r["equal"] == 2 and r["size"] == 3
    assert not K.close_f64(a, a + 1e-12, np.array([1e-15, 1e-15, 1e-15]))["ok"]
    one = np.float32(1.0)
    nxt = np.nextafter(one, np.float32(2.0))
    assert K.close_f32([one], [nxt])["ok"] and K.close_f32([one], [nxt])["equal"] == 0
    assert not K.close_f32([one], [np.nextafter(nxt, np.float32(2.0))])["ok"]
