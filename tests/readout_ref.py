"""The read-out heads of the plain ViT backbones (DPT/vit.py:263-341, run by forward_vit :117-146) restated in numpy: the three
formulas acr_wsss_amd/decoder.py ``readout`` is built from, and their backward.

    z   = tok2d (B T, D) . W1^T (D, f) + b1                        the 1x1 convolution as a Linear on ALL tokens
    y2  = z (B T, f) . Wt.view(f, f s^2)                           the ConvTranspose2d weight (ci, co, s, s) as stored
    out[b, co, i s + di, j s + dj] = y2[b T + start + i gw + j, (co s + di) s + dj] + bt[co]

``reassemble`` / ``reassemble_bwd`` keep the dtype of what they are given (float32 in: copies and one fp32 add, the bits the kernels
must produce); ``readout_fwd`` / ``readout_bwd`` compute in float64.  tests/test_readout_cpu.py pins all of it to torch's float64
``Conv2d -> ConvTranspose2d`` autograd."""
import numpy as np


def reassemble(y2, bias, B, T, start, gh, gw, C, s):
    """y2 (B T, >= C s^2): columns past C s^2 are row padding -> (B, C, gh s, gw s)"""
    y = np.asarray(y2)[:, :C * s * s].reshape(B, T, C, s, s)[:, start:].reshape(B, gh, gw, C, s, s)
    out = np.ascontiguousarray(y.transpose(0, 3, 1, 4, 2, 5)).reshape(B, C, gh * s, gw * s)
    return out if bias is None else out + np.asarray(bias).reshape(1, C, 1, 1)


def reassemble_bwd(dout, B, T, start, gh, gw, C, s):
    """-> (dy2 (B T, C s^2) with zeros in the skipped rows, dbias (C) in float64)"""
    dout = np.asarray(dout)
    d = dout.reshape(B, C, gh, s, gw, s).transpose(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * s * s)
    dy = np.zeros((B, T, C * s * s), dout.dtype)
    dy[:, start:] = d
    return dy.reshape(B * T, C * s * s), dout.astype(np.float64).sum(axis=(0, 2, 3))


def readout_fwd(tok, w1, b1, wt, bt, start, gh, gw):
    """tok (B, T, D), w1 (f, D, 1, 1), b1 (f); wt (f, f, s, s) and bt (f), or both None (tap 3: s = 1, no second step)
    -> (out (B, f, gh s, gw s), cache)"""
    tok = np.asarray(tok, np.float64)
    B, T, D = tok.shape
    f = w1.shape[0]
    w1m = np.asarray(w1, np.float64).reshape(f, D)
    tok2 = tok.reshape(B * T, D)
    z = tok2 @ w1m.T + np.asarray(b1, np.float64)
    if wt is None:
        s, w2, y2 = 1, None, z
    else:
        s = wt.shape[2]
        w2 = np.asarray(wt, np.float64).reshape(f, f * s * s)
        y2 = z @ w2
    out = reassemble(y2, None if bt is None else np.asarray(bt, np.float64), B, T, start, gh, gw, f, s)
    return out, dict(tok2=tok2, w1m=w1m, z=z, w2=w2, geom=(B, T, start, gh, gw, f, s), D=D)


def readout_bwd(cache, dout):
    """-> dict(tok, w1, b1[, wt, bt]) of float64 gradients shaped like the forward's arguments"""
    B, T, start, gh, gw, f, s = cache["geom"]
    dy2, dbt = reassemble_bwd(np.asarray(dout, np.float64), B, T, start, gh, gw, f, s)
    g = {}
    if cache["w2"] is None:
        dz = dy2
    else:
        dz = dy2 @ cache["w2"].T
        g["wt"] = (cache["z"].T @ dy2).reshape(f, f, s, s)
        g["bt"] = dbt
    g["tok"] = (dz @ cache["w1m"]).reshape(B, T, cache["D"])
    g["w1"] = (dz.T @ cache["tok2"]).reshape(f, cache["D"], 1, 1)
    g["b1"] = dz.sum(axis=0)
    return g
