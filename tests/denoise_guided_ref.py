"""The feature-guided filter of a progressive accumulation (fr_ctx_denoise_guided) restated in
numpy f32: the guided functions of fo-rma_amd/csrc/denoise.h operation for operation, every one
rounded once in f32 (tests/test_denoise_guided_host.py holds this against the header's own
bits). The features are a G-buffer as tests/gbuffer_ref.py returns it: "prim" [H, W] u32,
"depth" [H, W], "normal", "position" and "albedo" [H, W, 3] f32. Shared by the host and the GPU
tests; not a test module."""
import numpy as np

from tests import denoise_ref as D
from tests.denoise_ref import B3, EPS, H5, _shifted

F = np.float32
FEAT_MAX, NORMAL_MAX, ALB_MIN, ALB_MAX = F(2.0 ** 40), F(2.0 ** 10), F(2.0 ** -6), F(2.0 ** 6)
SIGMA_Z, NORMAL_POW2 = 2.0 ** -5, 4
MISS = np.uint32(0xFFFFFFFF)


def alb_of(g, demodulate):
    """a [H, W, 3]: the albedo where it is in [2^-6, 2^6], else (and without demodulate) 1."""
    alb = np.asarray(g["albedo"], F)
    if not demodulate:
        return np.ones(alb.shape, F)
    with np.errstate(invalid="ignore"):
        return np.where((alb >= ALB_MIN) & (alb <= ALB_MAX), alb, F(1))


def feat_ok(g):
    """[H, W]: a miss, or a hit whose t, |P_c| and |N_c| are under their caps (NaN is not)."""
    with np.errstate(invalid="ignore"):
        ok = ((np.asarray(g["depth"], F) <= FEAT_MAX) & (np.abs(np.asarray(g["position"], F)) <= FEAT_MAX).all(-1) &
              (np.abs(np.asarray(g["normal"], F)) <= NORMAL_MAX).all(-1))
    return ok | (np.asarray(g["prim"]) == MISS)


def prep(a, q, n, frames, g, demodulate=True):
    """(C [H, W, 3], var [H, W], valid [H, W]) of dn_prep_guided."""
    m, var, valid = D.prep(a, q, n, frames)
    if demodulate:
        a, q = np.asarray(a, F), np.asarray(q, F)
        fn = np.broadcast_to(np.asarray(n).astype(F), a.shape[:2])
        fk = np.broadcast_to((np.asarray(frames) - 1).astype(F), a.shape[:2])
        al = alb_of(g, True)
        with np.errstate(all="ignore"):
            v = np.fmax(((q - (a * m).astype(F)).astype(F) / fk[..., None]).astype(F), F(0))
            c = (m / al).astype(F)
            vd = (v / (al * al).astype(F)).astype(F)
            var = (((vd[..., 0] + vd[..., 1]).astype(F) + vd[..., 2]).astype(F) / fn).astype(F)
        m = c
    return m, var, valid & feat_ok(g)


def level(c, var, valid, g, step, k, sigma_z, normal_pow2):
    """One guided level: (C', var') from the previous level's; `valid` is prep's."""
    k, sigma_z = F(k), F(sigma_z)
    nrm, pos, t = np.asarray(g["normal"], F), np.asarray(g["position"], F), np.asarray(g["depth"], F)
    miss = np.asarray(g["prim"]) == MISS
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
        gg = (gs / gw).astype(F)
        sden = ((k * gg).astype(F) + EPS).astype(F)
        z = (sigma_z * t).astype(F)
        zden = ((z * z).astype(F) + EPS).astype(F)
        sumc = np.zeros(c.shape, F)
        sumv, sumw = zero.copy(), zero.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sx, sy = step * dx, step * dy
                ok = _shifted(valid, sx, sy, False) & (_shifted(miss, sx, sy, False) == miss)
                cq = _shifted(c, sx, sy, F(0))
                vq = _shifted(var, sx, sy, F(0))
                d = (cq - c).astype(F)
                dd = (d * d).astype(F)
                d2 = ((dd[..., 0] + dd[..., 1]).astype(F) + dd[..., 2]).astype(F)
                wc = (sden / (sden + d2).astype(F)).astype(F)
                w = (F(H5[dy + 2] * H5[dx + 2]) * wc).astype(F)
                if dx or dy:
                    nq = _shifted(nrm, sx, sy, F(0))
                    pq = _shifted(pos, sx, sy, F(0))
                    pr = (nrm * nq).astype(F)
                    cs = ((pr[..., 0] + pr[..., 1]).astype(F) + pr[..., 2]).astype(F)
                    cs = np.where(cs > 0, cs, F(0))
                    for _ in range(normal_pow2):
                        cs = (cs * cs).astype(F)
                    dp = (pq - pos).astype(F)
                    pe = (nrm * dp).astype(F)
                    e = ((pe[..., 0] + pe[..., 1]).astype(F) + pe[..., 2]).astype(F)
                    wz = (zden / (zden + (e * e).astype(F)).astype(F)).astype(F)
                    wn = np.where(miss, F(1), cs)
                    wz = np.where(miss, F(1), wz)
                    w = ((w * wn).astype(F) * wz).astype(F)
                sumc = np.where(ok[..., None], (sumc + (w[..., None] * cq).astype(F)).astype(F), sumc)
                sumv = np.where(ok, (sumv + ((w * w).astype(F) * vq).astype(F)).astype(F), sumv)
                sumw = np.where(ok, (sumw + w).astype(F), sumw)
        c2 = (sumc / sumw[..., None]).astype(F)
        v2 = (sumv / (sumw * sumw).astype(F)).astype(F)
    return np.where(valid[..., None], c2, c), np.where(valid, v2, var)


def denoise(a, q, n, frames, g, levels=D.LEVELS, k=D.K, sigma_z=SIGMA_Z, normal_pow2=NORMAL_POW2, demodulate=True):
    """(mean [H, W, 3] f32, u8 [H, W, 3], var [H, W] f32) of fr_ctx_denoise_guided; var is the
    demodulated-space variance."""
    from tests.test_accumulate import _to_u8
    c, var, valid = prep(a, q, n, frames, g, demodulate)
    for i in range(levels):
        c, var = level(c, var, valid, g, 1 << i, k, sigma_z, normal_pow2)
    if demodulate:
        with np.errstate(all="ignore"):
            c = (c * alb_of(g, True)).astype(F)
    return c, _to_u8(c), var


def valid_mask(a, q, n, frames, g):
    return prep(a, q, n, frames, g, False)[2]
