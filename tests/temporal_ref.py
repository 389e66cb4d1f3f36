"""Temporal reuse of a progressive accumulation (fr_ctx_temporal) restated in numpy f32 from
DESIGN.md §4.5f: the reprojection of the previous view's totals through the G-buffers of both
views, the totals, the filter's pixel and the call's place in a sequence of views, every
operation rounded once in f32 (tests/test_temporal_host.py holds this against the bits of the
header the kernels compile, fo-rma_amd/csrc/temporal.h). The features are G-buffers as
tests/gbuffer_ref.py returns them; the levels are tests/denoise_ref.py's and
tests/denoise_guided_ref.py's. Shared by the host and the GPU tests; not a test module."""
import numpy as np

from oracle import scene_ref as S
from tests import denoise_guided_ref as DG
from tests import denoise_ref as D
from tests.accum_error_ref import FLOOR
from tests.gbuffer_ref import cam_fields

F = np.float32
NONE = 0xFFFFFFFF
REUSED, NO_HISTORY, MISS, OFFSCREEN, ID, NORMAL, PLANE, HISTORY = range(8)
REASONS = ("reused", "no history yet", "miss", "behind the camera or out of frame", "id", "normal", "plane distance",
           "non-finite or empty history")
N_MAX, N_MAX_SPECULAR, SIGMA_Z, NORMAL_MIN = 32.0, 4.0, 2.0 ** -5, float(F(0.9))
OPT = dict(n_max=N_MAX, n_max_specular=N_MAX_SPECULAR, sigma_z=SIGMA_Z, normal_min=NORMAL_MIN)
SC_LAMBERT, SC_METAL, SC_DIELECTRIC, SC_LIGHT, SC_NONE = range(5)
FIELDS = ("prior_a", "prior_q", "prior_n", "prior_k", "total_a", "total_q", "total_n", "total_k", "source", "reason")


def scatter_classes(prims):
    """pack.cpp's effective scatter class per primitive: a stub has none, a plane is metal or
    lambertian whatever its material says, the others follow their material."""
    out = []
    for p in prims:
        kind = p["kind"] if p["kind"] <= S.TRIANGLE else S.STUB
        if kind == S.STUB:
            out.append(SC_NONE)
        elif kind == S.PLANE:
            out.append(SC_METAL if p["material"] == S.METAL else SC_LAMBERT)
        else:
            out.append({S.METAL: SC_METAL, S.DIELECTRIC: SC_DIELECTRIC, S.LIGHT: SC_LIGHT}.get(p["material"], SC_LAMBERT))
    return np.array(out, np.uint32)


def _dot(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z over the last axis."""
    p = (np.asarray(a, F) * np.asarray(b, F)).astype(F)
    return ((p[..., 0] + p[..., 1]).astype(F) + p[..., 2]).astype(F)


def _cross(a, b):
    return np.array([(a[1] * b[2]).astype(F) - (a[2] * b[1]).astype(F),
                     -((a[0] * b[2]).astype(F) - (a[2] * b[0]).astype(F)),
                     (a[0] * b[1]).astype(F) - (a[1] * b[0]).astype(F)], F)


def camera(cam):
    """What the projection reads of the previous camera (an FrCamera, an OrCamera or the four
    fields): pos, e = ll - pos, hor, ver, nrm = cross(hor, ver), hh, vv."""
    pos, ll, hor, ver = cam_fields(cam) if not isinstance(cam, tuple) else cam
    return dict(pos=pos, e=(ll - pos).astype(F), hor=hor, ver=ver, nrm=_cross(hor, ver), hh=_dot(hor, hor),
                vv=_dot(ver, ver))


def project(c, p, w, h):
    """(ok, x0, y0) [H, W] of the points p [H, W, 3] in camera c's w x h frame."""
    with np.errstate(all="ignore"):
        q = (p - c["pos"]).astype(F)
        s = (_dot(c["e"], c["nrm"]) / _dot(q, c["nrm"])).astype(F)
        r = ((s[..., None] * q).astype(F) - c["e"]).astype(F)
        u = (_dot(r, c["hor"]) / c["hh"]).astype(F)
        v = (_dot(r, c["ver"]) / c["vv"]).astype(F)
        fx, fy = np.floor((u * F(w)).astype(F)), np.floor((v * F(h)).astype(F))
        ok = (s > 0) & (fx >= 0) & (fx < F(w)) & (fy >= 1) & (fy <= F(h))
    x0 = np.where(ok, fx, 0).astype(np.int64)
    y0 = np.where(ok, h - np.where(ok, fy, 0).astype(np.int64), 0)
    return ok, x0, y0


def empty_prior(h, w, reason=NO_HISTORY):
    return dict(prior_a=np.zeros((h, w, 3), F), prior_q=np.zeros((h, w, 3), F), prior_n=np.zeros((h, w), F),
                prior_k=np.zeros((h, w), F), source=np.full((h, w), NONE, np.uint32),
                reason=np.full((h, w), reason, np.uint32))


def reproject(g, cls, hist, n_max=N_MAX, n_max_specular=N_MAX_SPECULAR, sigma_z=SIGMA_Z, normal_min=NORMAL_MIN):
    """The prior of the view with features g from the history {"g", "cam", "total_a", "total_q",
    "total_n", "total_k"} of the previous view; cls: the scene's classes by primitive."""
    h, w = g["prim"].shape
    prim, nrm, pos, t = np.asarray(g["prim"]), np.asarray(g["normal"], F), np.asarray(g["position"], F), np.asarray(g["depth"], F)
    out = empty_prior(h, w, MISS)
    hit = prim != NONE
    ok, x0, y0 = project(camera(hist["cam"]), pos, w, h)
    hg = hist["g"]
    with np.errstate(all="ignore"):
        id0, n0, p0 = np.asarray(hg["prim"])[y0, x0], np.asarray(hg["normal"], F)[y0, x0], np.asarray(hg["position"], F)[y0, x0]
        ta, tq, tn, tk = hist["total_a"][y0, x0], hist["total_q"][y0, x0], hist["total_n"][y0, x0], hist["total_k"][y0, x0]
        d = _dot(nrm, (p0 - pos).astype(F))
        z = (F(sigma_z) * t).astype(F)
        tests = [(OFFSCREEN, ok), (ID, id0 == prim), (NORMAL, _dot(nrm, n0) >= F(normal_min)),
                 (PLANE, (d * d).astype(F) <= ((z * z).astype(F) + D.EPS).astype(F)),
                 (HISTORY, (tn > 0) & np.isfinite(ta).all(-1) & np.isfinite(tq).all(-1))]
        reason = np.full((h, w), REUSED, np.uint32)
        for code, passed in reversed(tests):  # the first failure in the list's order wins
            reason = np.where(passed, reason, np.uint32(code))
        reason = np.where(hit, reason, np.uint32(MISS))
        spec = np.isin(cls[np.where(hit, prim, 0)], (SC_METAL, SC_DIELECTRIC)) if len(cls) else np.zeros((h, w), bool)
        cap = np.where(spec, F(n_max_specular), F(n_max)).astype(F)
        f = np.where(tn > cap, (cap / tn).astype(F), F(1)).astype(F)
        use = (reason == REUSED) & (f > 0)
        out["prior_a"] = np.where(use[..., None], (ta * f[..., None]).astype(F), F(0))
        out["prior_q"] = np.where(use[..., None], (tq * f[..., None]).astype(F), F(0))
        out["prior_n"] = np.where(use, (tn * f).astype(F), F(0))
        out["prior_k"] = np.where(use, (F(1) + ((tk - F(1)).astype(F) * f).astype(F)).astype(F), F(0))
    out["source"] = np.where(hit & ok, y0 * w + x0, NONE).astype(np.uint32)
    out["reason"] = reason
    return out


def totals(a, q, n, frames, prior):
    """A_T = A + A', Q_T = Q + Q', n_T = (float)n + n', K_T = (float)K + K'; n and frames are
    scalars or [H, W] arrays (each pixel's tile's n_t and K_t)."""
    a, q = np.asarray(a, F), np.asarray(q, F)
    fn = np.broadcast_to(np.asarray(n, np.uint32).astype(F), a.shape[:2])
    fk = np.broadcast_to(np.asarray(frames, np.uint32).astype(F), a.shape[:2])
    with np.errstate(all="ignore"):
        return dict(total_a=(a + prior["prior_a"]).astype(F), total_q=(q + prior["prior_q"]).astype(F),
                    total_n=(fn + prior["prior_n"]).astype(F), total_k=(fk + prior["prior_k"]).astype(F))


def prep(tot, miss, g=None, demodulate=True):
    """(C [H, W, 3], var [H, W], valid [H, W]): dn_prep (with g: dn_prep_guided) of (A_T, Q_T, n_T,
    K_T - 1) where K_T >= 2; where K_T < 2, var = (g g) / n_T with g = max((C_r + C_g) + C_b, 2^-7),
    or 0 where `miss` [H, W] says the pixel's primary ray hits nothing."""
    ta, tq, tn, tk = tot["total_a"], tot["total_q"], tot["total_n"], tot["total_k"]
    with np.errstate(all="ignore"):
        # (the refs take K and subtract 1 in f32: K_T - 1 here, rounded once)
        c, var, valid = DG.prep(ta, tq, tn, tk, g, demodulate) if g is not None else D.prep(ta, tq, tn, tk)
        m = (ta / tn[..., None]).astype(F)
        c1 = (m / DG.alb_of(g, True)).astype(F) if g is not None and demodulate else m
        gg = np.fmax(((c1[..., 0] + c1[..., 1]).astype(F) + c1[..., 2]).astype(F), FLOOR)
        var1 = np.where(miss, F(0), ((gg * gg).astype(F) / tn).astype(F))
        valid1 = (np.abs(m) <= D.MEAN_MAX).all(-1) & (var1 <= D.VAR_MAX)
        if g is not None:
            valid1 = valid1 & DG.feat_ok(g)
        first = tk < F(2)
    return np.where(first[..., None], c1, c), np.where(first, var1, var), np.where(first, valid1, valid)


def show(tot, miss, levels=D.LEVELS, k=D.K, g=None, sigma_z=DG.SIGMA_Z, normal_pow2=DG.NORMAL_POW2, demodulate=True):
    """(mean [H, W, 3] f32, u8 [H, W, 3], var [H, W] f32) of the totals: prep, `levels` levels (0:
    none) of the unguided filter, or with g of the guided one."""
    from tests.test_accumulate import _to_u8
    c, var, valid = prep(tot, miss, g, demodulate)
    for i in range(levels):
        if g is None:
            c, var = D.level(c, var, valid, 1 << i, k)
        else:
            c, var = DG.level(c, var, valid, g, 1 << i, k, sigma_z, normal_pow2)
    if g is not None and demodulate:
        with np.errstate(all="ignore"):
            c = (c * DG.alb_of(g, True)).astype(F)
    return c, _to_u8(c), var


def step(state, gen, key):
    """plan.h's temporal_step on state = (has_history, key, gen, read) or None:
    (action, read, write, next state)."""
    has, hkey, hgen, hread = state if state is not None else (False, None, None, 0)
    if has and hkey == key and hgen == gen:
        action, read = "keep", hread
    elif has and hkey == key:
        action, read = "reproject", hread ^ 1
    else:
        action, read = "empty", 0
    return action, read, read ^ 1, (True, key, gen, read)


class Temporal:
    """A context's temporal state over a sequence of calls: call() returns the dict of FIELDS
    plus "action", "mean", "u8" and "var"."""

    def __init__(self):
        self.state = self.hist = self.prior = None

    def reset(self):
        self.state = None

    def call(self, gen, key, a, q, n, frames, g, cam, cls, levels=D.LEVELS, k=D.K, guide=None, **opt):
        """gen: the accumulation generation; key: (scene, width, height, max_depth); guide: None,
        or a dict of sigma_z, normal_pow2, demodulate for the guided levels."""
        action, _, _, self.state = step(self.state, gen, key)
        h, w = g["prim"].shape
        if action == "reproject":
            self.prior = reproject(g, cls, self.hist, **opt)
        elif action == "empty":
            self.prior = empty_prior(h, w)
        tot = totals(a, q, n, frames, self.prior)
        if action != "keep":
            self.hist = dict(g=g, cam=cam_fields(cam))
        self.hist = dict(self.hist, **tot)
        mean, u8, var = show(tot, np.asarray(g["prim"]) == NONE, levels, k, g if guide is not None else None,
                             **(guide or {}))
        return dict(self.prior, **tot, action=action, mean=mean, u8=u8, var=var)
