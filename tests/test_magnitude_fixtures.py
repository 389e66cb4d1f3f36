"""The magnitude fixtures (tests/magnitude_fixtures.py) reach the guards they are built for.

Checked against the oracle alone (no GPU): the guard predicates of rt_core.h are restated
here in numpy f32 and evaluated on the primary rays at the four corners of every pixel; a
fixture's named guard must be false for all of them ("all") or take both values inside one
8 x 8 tile, the 64 items a wave sets up together ("cross"). The declared condition must hold
in the oracle's counters and image, and apart from the named flat frames every frame must
show at least 128 distinct colours. tests/test_magnitude.py then compares the trace kernels
with the same oracle frames."""
import numpy as np
import pytest

from oracle import scene_ref as S
from tests import magnitude_fixtures as M
from tests.test_plan import _build_plan_check, _plan

F = np.float32
CAP = 128


def _distinct(mean):
    return len({tuple(p) for p in mean.reshape(-1, 3).view(np.uint32).tolist()})


def _v(x):
    return np.asarray([F(c) for c in x], dtype=F)


def primary_rays(cam):
    """d[H, W, 4, 3] at the corners of every pixel, in get_ray's order of operations with the
    pixel's s = (x + {0, 1}) / W and t = (H - y + {0, 1}) / H (no jitter, no lens offset)."""
    ll, hor, ver, pos = _v(cam["ll"]), _v(cam["hor"]), _v(cam["ver"]), _v(cam["pos"])
    c = np.arange(4)
    s = ((np.arange(M.W)[:, None] + (c & 1)[None, :]).astype(F) / F(M.W))[None, :, :, None]
    t = ((M.H - np.arange(M.H)[:, None] + (c >> 1)[None, :]).astype(F) / F(M.H))[:, None, :, None]
    with np.errstate(all="ignore"):
        return ((ll + s * hor) + t * ver) - pos


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _in(x, lo, hi, closed=True):
    return (x >= F(2.0) ** lo) & ((x <= F(2.0) ** hi) if closed else (x < F(2.0) ** hi))


def guard_ok(name, cam, prims):
    """(ok, counted): the guard's value per primary ray and the rays it is evaluated for."""
    with np.errstate(all="ignore"):
        d = primary_rays(cam)
        every = np.ones(d.shape[:3], dtype=bool)
        a = _dot(d, d)
        if name == "recip_nr":
            return _in(np.abs(d), -126, 126, closed=False).all(axis=3), every
        if name == "recip_box":
            return _in(np.abs(d), -100, 126, closed=False).all(axis=3), every
        if name == "sphere_seg":
            return _in(a, -60, 60), every
        if name == "sky":
            return _in(a, -96, 126), every
        if name == "reach":
            near = F(np.max(np.abs(_v(cam["pos"])))) <= F(100.0) * F(F(M.extent(prims)) + F(1.0))
            return np.full(d.shape[:3], bool(near)), every
        assert name == "sphere_roots"
        ok, counted = np.ones(d.shape[:3], dtype=bool), np.zeros(d.shape[:3], dtype=bool)
        for p in prims:
            if p["kind"] != S.SPHERE:
                continue
            oc = _v(cam["pos"]) - p["g"][:3]
            b = _dot(np.broadcast_to(oc, d.shape), d)
            disc = b * b - a * F(_dot(oc, oc) - p["g"][3] * p["g"][3])
            fast = _in(a, -60, 60) & _in(disc, -96, 126) & (np.abs(b) <= F(2.0) ** 40)
            live = disc > 0
            ok &= fast | ~live
            counted |= live
        return ok, counted


@pytest.mark.parametrize("k", [-20, 3, 30])
def test_scaled_is_exact_and_leaves_directions_alone(k):
    base = M.lattice("mixed", "small")
    got = M.scaled(base, k)
    f = M.p2(k)
    for p, q in zip(base, got):
        assert (p["kind"], p["material"]) == (q["kind"], q["material"]) and np.array_equal(p["color"], q["color"])
        same = [i for i in range(16) if i not in M._SCALED_WORDS[p["kind"]]]
        assert np.array_equal(p["g"][same], q["g"][same])
        assert np.array_equal(q["g"] / np.where(np.isin(np.arange(16), same), F(1), f), p["g"])
    obb = next(q for q in got if q["kind"] == S.OBB)
    assert set(np.abs(obb["g"][3:12]).tolist()) == {0.0, 1.0} and list(obb["g"][12:15]) == [f, f, f]
    assert M.extent(got) == M.extent(base) * float(f)


def test_every_guard_has_an_all_lanes_and_a_mixed_wave_fixture():
    """Each guard of the hot path is left by every primary ray of one fixture and straddled
    inside one batch by another. The reach is a property of the ray's origin, which the primary
    rays of a frame share: it has all-lanes fixtures on either side of the bound only."""
    seen = {}
    for kind in M.KINDS:
        for size in M.SIZES:
            for fx in M.families(kind, size):
                if fx.guard:
                    seen.setdefault(fx.guard, set()).add(fx.mode)
    assert set(seen) == {"recip_nr", "recip_box", "sphere_seg", "sphere_roots", "sky", "reach"}, seen
    for g in ("recip_nr", "recip_box", "sphere_seg", "sphere_roots", "sky"):
        assert seen[g] == {"all", "cross"}, (g, seen[g])
    assert seen["reach"] == {"all"}


def test_left_out_values_fall_under_the_cap(fr):
    """The values that are no fixtures (magnitude_fixtures.UNDER_CAP) are exactly the candidates
    whose oracle frame shows fewer than 128 colours without being a named flat frame."""
    short = {}
    for kind in M.KINDS:
        for size in M.SIZES:
            for fx in M.candidates(kind, size):
                mean = M.reference(fr, kind, size, "full", fx.name, 8)[1]
                colours, nan = _distinct(mean), int(np.isnan(mean).any(axis=2).sum())
                is_flat = colours == 1 or nan == mean.shape[0] * mean.shape[1]
                if colours < CAP and not (fx.flat and is_flat):
                    short.setdefault(fx.name, {})[kind, size] = colours
    assert short == M.UNDER_CAP


@pytest.mark.parametrize("kind,size,name", M.cases())
def test_fixture_reaches_its_guard(kind, size, name):
    fx = M.fixture(kind, size, name)
    if not fx.guard:
        return
    ok, counted = guard_ok(fx.guard, fx.cam, M.scene(kind, size, fx))
    assert counted.any(), "no primary ray evaluates the guard"
    if fx.mode == "all":
        assert not ok[counted].any(), f"{fx.guard} holds for {int(ok[counted].sum())} of {int(counted.sum())} rays"
        return
    # both sides inside one tile of 8 x 8 pixels
    tiles = [(ty, tx) for ty in range(0, M.H, 8) for tx in range(0, M.W, 8)]
    both = [t for t in tiles if (ok & counted)[t[0]:t[0] + 8, t[1]:t[1] + 8].any()
            and (~ok & counted)[t[0]:t[0] + 8, t[1]:t[1] + 8].any()]
    assert both, f"{fx.guard}: no tile holds both sides"


@pytest.mark.parametrize("kind,size,name", M.cases())
def test_fixture_reaches_its_condition(fr, kind, size, name):
    fx = M.fixture(kind, size, name)
    _, mean, _, cnt = M.reference(fr, kind, size, "full", name, 8)
    nan = int(np.isnan(mean).any(axis=2).sum())
    colours = _distinct(mean)
    if fx.flat:  # the named flat frames are flat: the set is exact
        assert colours == 1 or nan == M.W * M.H, (colours, nan)
    else:
        assert colours >= CAP, colours
    if fx.expect == "nan_all":
        assert nan == M.W * M.H
        if name.startswith("M1"):
            assert cnt["hits"] == 0
    elif fx.expect == "hit_mostly":
        assert nan == 0 and 2 * cnt["hits"] >= cnt["segments"], cnt
    elif fx.expect == "must_miss":
        assert nan == 0 and cnt["hits"] == 0, cnt
    elif fx.expect == "same_as_unscaled":
        _, tmean, _, tcnt = M.reference(fr, kind, size, "full", fx.twin, 8)
        assert cnt == tcnt and nan == 0
        # the hits scale exactly; the sky's unit(d) does too while dot(d, d) stays normal
        # (k = -64 puts it at 2^-128: denormal, the blend parameter moves by an ulp or so)
        if name.split("_")[1] != "k-64":
            assert np.array_equal(mean.view(np.uint32), tmean.view(np.uint32))
        else:
            assert np.allclose(mean, tmean, rtol=0, atol=1e-5)


M6_FRAMES = [(kind, size, variant, depth) for kind in ("box", "mixed") for size in ("small", "big")
             for variant in ("full", "diffuse", "classes") for depth in (8, 12)]


@pytest.mark.parametrize("kind,size,variant,depth", M6_FRAMES)
def test_attenuation_magnitudes_reach_denormals_and_infinities(fr, kind, size, variant, depth):
    """M6: a path's product of 2^-18 colours is denormal at 8 scatters and zero from 9 (or at
    the depth cap), one of 2^17 colours is inf from 8. The frames have one sample per pixel
    (magnitude_fixtures.frame), so the oracle's mean is the sample's own product chain: every
    frame of every variant, size and depth must show the condition it is named for."""
    assert M.frame(M.fixture(kind, size, "M6_2^-18")) == (32, 32, 1)
    mag = np.abs(M.reference(fr, kind, size, variant, "M6_2^-18", depth)[1])
    assert (mag < F(2.0) ** -126).any(), float(mag.min())  # denormal or zero
    big = M.reference(fr, kind, size, variant, "M6_2^17", depth)[1]
    assert (~np.isfinite(big)).any(), float(np.nanmax(big))  # inf or NaN
    if depth == 8:
        for name in ("M6_neg0", "M6_negative", "M6_inf", "M6_nan"):
            prims = M.scene(kind, size, M.fixture(kind, size, name), variant)
            odd = [p for p in prims if np.signbit(p["color"]).any() or not np.isfinite(p["color"]).all()]
            assert len(odd) == 1 and odd[0]["material"] == S.LAMBERTIAN
            mean = M.reference(fr, kind, size, variant, name, depth)[1]
            plain = M.reference(fr, kind, size, variant, "M6_2^-18", depth)[3]
            assert M.reference(fr, kind, size, variant, name, depth)[3] == plain  # the same paths: only colours differ
            if name == "M6_nan":
                assert np.isnan(mean).any()
            if name == "M6_inf":
                assert (~np.isfinite(mean)).any()
            if name == "M6_negative":
                assert (mean < 0).any()


def test_sign_of_a_tiny_component_changes_the_frame(fr):
    """M2: +c and -c are different rays (which face of a cell the fan grazes past)."""
    pos = M.reference(fr, "box", "small", "full", "M2_+2^-110_shifted", 8)[3]
    neg = M.reference(fr, "box", "small", "full", "M2_-2^-110_shifted", 8)[3]
    assert pos["segments"] != neg["segments"], (pos, neg)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan_magnitude") / "plan_check")
    _build_plan_check(out)
    return out


def _origin_reach(prims):
    """bvh.h bvh_origin_reach in f32: 100 (extent + 1), and for a scene with spheres no more than
    where the sphere test's rounding error stays inside half the cull's padding."""
    ext = F(M.extent(prims))
    unit = ext + F(1.0)
    reach = F(100.0) * unit
    radii = [abs(F(p["g"][3])) for p in prims if p["kind"] == S.SPHERE]
    if radii:
        pad = F(1e-4) * ext + F(1e-4)
        safe = np.sqrt((min(radii) * pad + F(0.25) * pad * pad) * (F(1048576.0) / F(3.0))) - ext
        reach = min(reach, max(unit, F(safe)))
    return float(reach), (float(min(radii)) if radii else -1.0)


@pytest.mark.parametrize("kind", M.KINDS)
def test_camera_reach_flips_the_plan_between_99_and_101(plan_exe, kind):
    """M5: the host's cam_near (plan.cpp) keeps the BVH for a camera within 100 (extent + 1)
    and falls back to the in-order loop beyond. A lattice with spheres (radius 1) has a shorter
    reach, its own extent + 1: from 50 extents the sphere test's rounding error is larger than
    the spheres, far beyond what the cull's padding covers."""
    prims = M.lattice(kind, "big")
    assert M.bvh_cost(prims) >= 48 and len(prims) >= 48
    limit, rmin = _origin_reach(prims)
    spheres = kind in ("sphere", "mixed")
    assert limit == (M.extent(prims) + 1.0) * (1 if spheres else 100) and (rmin == 1.0) == spheres
    for f in M.M5_FACTORS:
        cam = M.fixture(kind, "big", f"M5_x{f}").cam
        reach = max(abs(float(x)) for x in cam["pos"])
        assert reach == f * (M.extent(prims) + 1.0)
        r = _plan(plan_exe, n=len(prims), kinds=63, bvh_ok=1, diffuse=0, bvh_extent=M.extent(prims), bvh_sphere_rmin=rmin,
                  reach=repr(reach), w=M.W, h=M.H, spp=M.SPP)
        assert r["use_bvh"] == int(reach <= limit) == int(f <= (1 if spheres else 100)), (f, r["use_bvh"])
    near = _plan(plan_exe, n=len(prims), kinds=63, bvh_ok=1, diffuse=0, bvh_extent=M.extent(prims), bvh_sphere_rmin=rmin,
                 reach=repr(limit), w=M.W, h=M.H, spp=M.SPP)
    assert near["use_bvh"] == 1
