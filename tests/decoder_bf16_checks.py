"""The yardstick of the bf16-storage decoder entry points (tests/test_decoder_bf16_gpu.py), free of torch and of the GPU so that
tests/test_decoder_bf16_cpu.py can exercise it on synthetic values.

include/acr_hip.h defines a bf16 output as the fp32 entry point's result rounded to bf16 by round-to-nearest-even.  ``accept_bf16``
holds a tensor of bf16 bit patterns to that, element by element.  One exception serves an implementation that sums in another
(fixed) order: where the fp32 result lies within ``WINDOW`` fp32 ulps of the midpoint between two adjacent bf16 values, the other
neighbour is accepted too -- for at most ``CAP`` of a tensor's elements.  The window holds 2 * WINDOW + 1 = 9 of the 65536 fp32
values between two bf16 neighbours, so about 1.4e-4 of random elements fall into it.

Doubles and floats: ``close_f64`` (a bound the caller computes from the summands: 2^-53 * n * sum |summand|, the reordering error of
a double sum of n terms) and ``close_f32`` (1 ulp); both report how many values were bit-equal."""
import numpy as np

WINDOW = 4
CAP = 1e-3


def f32_bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32).astype(np.uint64)


def bf16_rne(a):
    """the bf16 bit patterns (uint16) of fp32 values rounded to nearest, ties to even (finite values)"""
    u = f32_bits(a)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def in_window(a):
    """True where an fp32 value lies within WINDOW fp32 ulps of the midpoint between its two bf16 neighbours"""
    low = (f32_bits(a) & 0xFFFF).astype(np.int64)
    return np.abs(low - 0x8000) <= WINDOW


def window_share(a):
    a = np.asarray(a)
    return float(in_window(a.astype(np.float32)).mean()) if a.size else 0.0


def accept_bf16(got_bits, ref_f32, what=""):
    """got_bits: uint16 bf16 patterns; ref_f32: the fp32 yardstick.  Returns dict(exact, exempt, wrong, share, ok): ``exact``
    elements equal RNE(ref), ``exempt`` ones are the other neighbour inside the window, ``wrong`` everything else; ok = no wrong
    element and exempt <= CAP * size."""
    got = np.asarray(got_bits, np.uint16).reshape(-1)
    ref = np.asarray(ref_f32, np.float32).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    want = bf16_rne(ref)
    down = (f32_bits(ref) >> 16).astype(np.uint16)                 # the neighbour towards zero; the other one is down + 1
    other = np.where(want == down, down + np.uint16(1), down).astype(np.uint16)
    exact = got == want
    exempt = ~exact & (got == other) & in_window(ref)
    wrong = ~exact & ~exempt
    # -0 and +0 are the same value: a zero result may carry either sign
    zero = (bf16_to_f32(got) == 0) & (bf16_to_f32(want) == 0)
    wrong &= ~zero
    exact |= zero
    n = max(got.size, 1)
    out = dict(exact=int(exact.sum()), exempt=int(exempt.sum()), wrong=int(wrong.sum()), share=float(exempt.sum()) / n, size=got.size)
    out["ok"] = out["wrong"] == 0 and out["exempt"] <= CAP * got.size
    return out


def close_f64(got, ref, bound):
    """|got - ref| <= bound elementwise (bound: array or scalar, >= 0).  dict(equal, size, worst, ok)"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, np.float64).reshape(-1) if np.ndim(bound) else np.float64(bound), got.shape)
    err = np.abs(got - ref)
    return dict(equal=int((got.view(np.uint64) == ref.view(np.uint64)).sum()), size=got.size, worst=float(err.max()) if got.size else 0.0,
                ok=bool((err <= bound).all()))


def close_f32(got, ref):
    """within 1 fp32 ulp of each other.  dict(equal, size, ok)"""
    got, ref = np.asarray(got, np.float32).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(ref)).astype(np.float32))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return dict(equal=int((got.view(np.uint32) == ref.view(np.uint32)).sum()), size=got.size, ok=bool((err <= ulp).all()))
