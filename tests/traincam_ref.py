"""numpy restatement of ``acr_train_cam_f32`` (include/acr_hip.h; the reference's compute_cam_up, myTool.py:860-864, and the
two-view sum + min-max normalisation of infer_cam.py:156-162, 201-202).

``cams_f32``: csrc/acr_resample.h's operations in their order, every intermediate rounded to float32 -- the kernel is compiled with
-ffp-contract=off, so this is its arithmetic and the comparison is bit for bit.  ``cams_f64``: the same rule in float64."""
import numpy as np

F = np.float32


def _axis(n_in, n_out, dt):
    """first tap, second tap, lambda, 1 - lambda of every destination index (acr_src_half_pixel + acr_taps_of)"""
    scale = dt(dt(n_in) / dt(n_out))
    d = np.arange(n_out).astype(dt)
    src = ((scale * (d + dt(0.5))).astype(dt) - dt(0.5)).astype(dt)        # every step rounded to dt
    src = np.where(src < 0, dt(0), src).astype(dt)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    lam = (src - i0.astype(dt)).astype(dt)
    return i0, i1, lam, (dt(1) - lam).astype(dt)


def upsample(src, oh, ow, dt=F):
    """src (..., gh, gw) -> (..., oh, ow): hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11), align_corners=False"""
    src = np.asarray(src, dt)
    gh, gw = src.shape[-2:]
    y0, y1, ly, hy = _axis(gh, oh, dt)
    x0, x1, lx, hx = _axis(gw, ow, dt)
    ly, hy = ly[:, None], hy[:, None]
    v00, v01 = src[..., y0[:, None], x0[None, :]], src[..., y0[:, None], x1[None, :]]
    v10, v11 = src[..., y1[:, None], x0[None, :]], src[..., y1[:, None], x1[None, :]]
    top = ((hx * v00).astype(dt) + (lx * v01).astype(dt)).astype(dt)
    bot = ((hx * v10).astype(dt) + (lx * v11).astype(dt)).astype(dt)
    return ((hy * top).astype(dt) + (ly * bot).astype(dt)).astype(dt)


def plane_sum(cam1, cam2, label, grid, out_hw, dt=F):
    """s (B, C, oh, ow) before the normalisation; cam (B, gh * gw, C) token-major, label (B, C).  Planes with label 0 are +0."""
    gh, gw = grid
    oh, ow = out_hw
    B, N, C = cam1.shape
    lab = np.asarray(label, dt)[:, :, None, None]
    on = lab != 0

    def up(cam):
        planes = np.where(on, np.asarray(cam).transpose(0, 2, 1).reshape(B, C, gh, gw), 0)    # an absent plane's source is not read
        return upsample(planes.astype(dt), oh, ow, dt)
    s = (up(cam1) * lab).astype(dt)
    if cam2 is not None:
        s = (s + (up(cam2)[..., ::-1] * lab).astype(dt)).astype(dt)      # the mirrored OUTPUT column
    return np.where(on, s, dt(0)).astype(dt)


def normalise(s, eps, label, dt=F):
    mn = s.min(axis=(2, 3), keepdims=True)
    mx = s.max(axis=(2, 3), keepdims=True)
    den = ((mx - mn).astype(dt) + dt(eps)).astype(dt)
    out = ((s - mn).astype(dt) / den).astype(dt)
    return np.where(np.asarray(label)[:, :, None, None] != 0, out, dt(0)).astype(dt)


def cams_f32(cam1, cam2, label, grid, out_hw, eps=1e-5, normalize=True):
    s = plane_sum(np.asarray(cam1, F), None if cam2 is None else np.asarray(cam2, F), label, grid, out_hw, F)
    return normalise(s, eps, label, F) if normalize else s


def cams_f64(cam1, cam2, label, grid, out_hw, eps=1e-5, normalize=True):
    """float64 arithmetic throughout; eps is the float32 value the kernel adds"""
    dt = np.float64
    s = plane_sum(np.asarray(cam1, dt), None if cam2 is None else np.asarray(cam2, dt), label, grid, out_hw, dt)
    return normalise(s, float(F(eps)), label, dt) if normalize else s


def make_case(shape, seed):
    """cam1, cam2 (B, N, C) float32 in the normal range, labels 0/1 with 1-3 present classes per image and (B > 1) one image with none"""
    B, C, gh, gw, _, _ = shape
    rng = np.random.default_rng(seed)
    cam1 = (rng.random((B, gh * gw, C), dtype=np.float32) * 4).astype(np.float32)      # relu outputs: >= 0
    cam2 = (rng.random((B, gh * gw, C), dtype=np.float32) * 4).astype(np.float32)
    lab = np.zeros((B, C), np.float32)
    for b in range(B):
        if B > 1 and b == B - 1:
            continue                                     # an image without a class
        lab[b, rng.choice(C, size=min(C, int(rng.integers(1, 4))), replace=False)] = 1
    return cam1, cam2, lab
