"""The variance-guided filter of a progressive accumulation (fr_ctx_denoise) restated in numpy
f32: fo-rma_amd/csrc/denoise.h operation for operation, every one rounded once in f32
(tests/test_denoise_host.py holds this against the header's own bits). Validity is carried as a
boolean image from prep through every level, as the header carries it in var's sign bit.
Shared by the host and the GPU tests; not a test module."""
import numpy as np

F = np.float32
EPS, MEAN_MAX, VAR_MAX = F(2.0 ** -20), F(2.0 ** 40), F(2.0 ** 80)
LEVELS, K = 4, 4.0
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
B3 = (F(1), F(2), F(1))


def prep(a, q, n, frames):
    """(C [H, W, 3], var [H, W], valid [H, W]) from A and Q [H, W, 3]; n and frames are scalars
    or [H, W] arrays (each pixel's tile's n_t and K_t)."""
    a, q = np.asarray(a, F), np.asarray(q, F)
    fn = np.broadcast_to(np.asarray(n).astype(F), a.shape[:2])
    fk = np.broadcast_to((np.asarray(frames) - 1).astype(F), a.shape[:2])
    with np.errstate(all="ignore"):
        m = (a / fn[..., None]).astype(F)
        v = np.fmax(((q - (a * m).astype(F)).astype(F) / fk[..., None]).astype(F), F(0))  # fmax: a NaN reads 0
        var = (((v[..., 0] + v[..., 1]).astype(F) + v[..., 2]).astype(F) / fn).astype(F)
        valid = (np.abs(m) <= MEAN_MAX).all(-1) & (var <= VAR_MAX)
    return m, var, valid


def _shifted(img, dx, dy, fill):
    """img sampled at p + (dx, dy); `fill` where that is outside the image."""
    h, w = img.shape[:2]
    out = np.full_like(img, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = img[ys, xs]
    return out


def level(c, var, valid, step, k):
    """One level: (C', var') from the previous level's; `valid` is prep's and does not change."""
    k = F(k)
    zero = np.zeros(var.shape, F)
    with np.errstate(all="ignore"):
        gs, gw = zero.copy(), zero.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = _shifted(valid, dx, dy, False)
                vq = _shifted(var, dx, dy, F(0))
                wt = F(B3[dy + 1] * B3[dx + 1])
                gs = np.where(ok, (gs + (wt * vq).astype(F)).astype(F), gs)
                gw = np.where(ok, (gw + wt).astype(F), gw)
        g = (gs / gw).astype(F)
        sden = ((k * g).astype(F) + EPS).astype(F)
        sumc = np.zeros(c.shape, F)
        sumv, sumw = zero.copy(), zero.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ok = _shifted(valid, step * dx, step * dy, False)
                cq = _shifted(c, step * dx, step * dy, F(0))
                vq = _shifted(var, step * dx, step * dy, F(0))
                d = (cq - c).astype(F)
                dd = (d * d).astype(F)
                d2 = ((dd[..., 0] + dd[..., 1]).astype(F) + dd[..., 2]).astype(F)
                wc = (sden / (sden + d2).astype(F)).astype(F)
                w = (F(H5[dy + 2] * H5[dx + 2]) * wc).astype(F)
                sumc = np.where(ok[..., None], (sumc + (w[..., None] * cq).astype(F)).astype(F), sumc)
                sumv = np.where(ok, (sumv + ((w * w).astype(F) * vq).astype(F)).astype(F), sumv)
                sumw = np.where(ok, (sumw + w).astype(F), sumw)
        c2 = (sumc / sumw[..., None]).astype(F)
        v2 = (sumv / (sumw * sumw).astype(F)).astype(F)
    return np.where(valid[..., None], c2, c), np.where(valid, v2, var)


def denoise(a, q, n, frames, levels=LEVELS, k=K):
    """(mean [H, W, 3] f32, u8 [H, W, 3], var [H, W] f32) of fr_ctx_denoise."""
    from tests.test_accumulate import _to_u8
    c, var, valid = prep(a, q, n, frames)
    for i in range(levels):
        c, var = level(c, var, valid, 1 << i, k)
    return c, _to_u8(c), var


def valid_mask(a, q, n, frames):
    return prep(a, q, n, frames)[2]
