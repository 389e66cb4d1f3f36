"""Fixtures for the magnitude-edge parity tests (tests/test_magnitude.py): tiny, huge and
denormal ray directions, scenes and attenuations, over the lattice scenes of
tests/ray_edge_fixtures.py.

The hot path replaces a division, a square root or a reciprocal by a cheaper sequence only
inside a range guard (rt_core.h recip_nr_ok, recip_box_ok, sphere_seg, sphere_roots_fast,
sky_t_fast_from; the BVH kernels' origin reach) and takes the plain expression outside it.
Cameras from camera_new / camera_look over scenes of order 1..100 never leave any guard's
range, so the families here do, on purpose:

  M1  every direction component scaled by 2^k, camera at the origin
  M2  one tiny or huge component: a fan in the plane x = 0 with d.x = c, and fans whose d.x
      crosses a guard's bound inside one wave
  M3  scene and camera scaled together by 2^s
  M4  scene and camera position scaled by 2^s, directions left at unit scale
  M5  the camera at 50, 99, 101 and 1000 times the BVH's origin reach unit
  M6  attenuations of 2^-18, 2^17, -0.0, negative, inf and NaN
  M7  the scene at 2^20 seen from the origin with directions of 2^-64: a denormal dot(d, d)
  M8  M2's fan with every component tiny: hits at t ~ 2^100, where the box reciprocal's clamp
      decides them

The camera of M1 and M2 stands at the origin exactly: get_ray forms lower_left + s horizontal
+ t vertical - position, and any non-zero position absorbs a direction of 2^-31 into its ulp
(the ray becomes d = 0). With position = 0 the scaled fields and every d are exact.

Each Fixture names the condition it must reach (`expect`, as in ray_edge_fixtures, and
"same_as_unscaled": the oracle's counters equal those of the unscaled twin) and the guard it
must leave (`guard`, `mode` "all": false for every primary ray; "cross": both sides inside
one 64-item batch). tests/test_magnitude_fixtures.py checks both against the oracle alone.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests.ray_edge_fixtures import H, SEED, SPP, W, bvh_cost, cells, edge_camera, lattice  # noqa: F401 (re-exported)

F = np.float32
KINDS = ("box", "sphere", "obb", "tri", "mixed")
SIZES = ("small", "mid", "big")


def p2(k):
    """2^k as f32 (exact down to the least denormal 2^-149)."""
    return F(np.ldexp(np.float64(1.0), k))


def below(x):
    """The f32 next to x towards zero."""
    return np.nextafter(F(x), F(0.0))


# ---- scenes -------------------------------------------------------------------------

# the geometry words of fr_prim.g that hold lengths or positions, per kind (a plane's
# orientation and an oriented box's axes are directions and stay)
_SCALED_WORDS = {S.SPHERE: range(0, 4), S.PLANE: (0, 1, 2, 6, 7, 8), S.AABB: range(0, 6), S.OBB: (0, 1, 2, 12, 13, 14),
                 S.TRIANGLE: range(0, 9), S.STUB: ()}


def scaled(prims, k):
    """The scene times 2^k, exactly in f32: sphere centre and radius, plane position and
    size, both box corners, oriented-box centre and half extents, triangle vertices."""
    f = p2(k)
    out = []
    for p in prims:
        g = p["g"].copy()
        for i in _SCALED_WORDS[p["kind"]]:
            g[i] = g[i] * f
            assert g[i] / f == p["g"][i]  # no overflow, no bits lost to a denormal
        out.append(dict(p, g=g))
    return out


def coloured(prims, colour=None, one=None):
    """The scene with every colour replaced by `colour`, or with one component of the first
    lambertian primitive's colour replaced by `one`."""
    out = [dict(p, color=p["color"].copy()) for p in prims]
    if colour is not None:
        for p in out:
            p["color"][:] = F(colour)
    if one is not None:
        first = next(p for p in out if p["material"] == S.LAMBERTIAN and p["kind"] != S.STUB)
        first["color"][1] = F(one)
    return out


def extent(prims):
    """bvh.cpp scene_abs_max: the largest |coordinate| of any bounded primitive (planes and
    stubs have no bounds)."""
    m = 0.0
    for p in prims:
        g = [float(x) for x in p["g"]]
        if p["kind"] == S.SPHERE:
            m = max([m] + [abs(g[i] + s * g[3]) for i in range(3) for s in (-1, 1)])
        elif p["kind"] == S.AABB:
            m = max([m] + [abs(x) for x in g[:6]])
        elif p["kind"] == S.TRIANGLE:
            m = max([m] + [abs(x) for x in g[:9]])
        elif p["kind"] == S.OBB:
            r = [sum(abs(g[3 + 3 * a + i]) * g[12 + a] for a in range(3)) for i in range(3)]
            m = max([m] + [abs(g[i] + s * r[i]) for i in range(3) for s in (-1, 1)])
    return m


# ---- fixtures -----------------------------------------------------------------------

# name; shift: the lattice's x shift; scale: the scene's power of two; cam: edge_camera's
# arguments; expect: "hit_mostly", "must_miss", "nan_all", "same_as_unscaled" or None; twin: the
# unscaled fixture's name for same_as_unscaled; guard / mode: the guard the primary rays must
# leave ("all") or straddle inside one batch ("cross"); colour / one: coloured()'s arguments;
# flat: the oracle's frame may be constant or all NaN (the cap does not apply)
Fixture = namedtuple("Fixture", "name shift scale cam expect twin guard mode colour one flat")


def _fx(name, cam, shift=0, scale=0, expect=None, twin=None, guard=None, mode="all", colour=None, one=None, flat=False):
    return Fixture(name, shift, scale, cam, expect, twin, guard, mode if guard else None, colour, one, flat)


D0, HOR, VER = (-0.33, -0.5, -1.0), (0.8, 0.05, 0.0), (0.03, 1.0, 0.0)
CAM0 = dict(pos=(0.37, -0.79, 0.13), ll=(0.04, -1.29, -0.87), hor=HOR, ver=VER)  # R0_control's, without the lens


# M6: from between the mirror slab and the lattice, a cone onto the lattice's front: of its 1024
# paths some run to the depth cap in every variant, size and depth
M6_CAM = dict(pos=(1.0, 0.25, -1.5), ll=(0.75, 0.0, -2.5), hor=(0.5, 0.01, 0.0), ver=(0.02, 0.5, 0.0))


def _times(v, f):
    return tuple(F(x) * f for x in v)


def _m1_cam(k):
    f = p2(k)
    return dict(pos=(0.0, 0.0, 0.0), ll=_times(D0, f), hor=_times(HOR, f), ver=_times(VER, f))


def _m2_cam(c, hx=0.0):
    return dict(pos=(0.0, 0.0, 0.0), ll=(c, -0.5, -1.0), hor=(hx, 1.0, 0.0), ver=(0.0, 0.0, -0.5))


def _m3_cam(s):
    f = p2(s)
    return {k: _times(v, f) for k, v in CAM0.items()}


def _m4_cam(s):
    pos = _times(CAM0["pos"], p2(s))
    d0 = tuple(F(a) - F(b) for a, b in zip(CAM0["ll"], CAM0["pos"]))
    return dict(pos=pos, ll=tuple(p + d for p, d in zip(pos, d0)), hor=HOR, ver=VER)


def _m5_cam(unit, factor):
    """On the -z axis behind the lattice, a cone just wide enough for it (about +-8 at the
    lattice's distance), looking towards +z."""
    z = -F(factor) * F(unit)
    a = F(8.0) / -z
    return dict(pos=(1.0, 0.0, z), ll=(F(1.0) - a, -a, z + F(1.0)), hor=(F(2) * a, 0.0, 0.0), ver=(0.0, F(2) * a, 0.0))


# M1: the guard each k leaves for every primary ray (|d| ~ 2^k, dot(d, d) ~ 2^(2k)):
# a < 2^-60 from -31, dd < 2^-96 from -49, every |d.x| < 2^-100 at -100 (d.x spans
# [-0.33, 0.5] 2^k), denormal components at -140; a > 2^60 at +40, dd = inf at +64
M1_K = {-20: None, -31: "sphere_seg", -47: "sphere_seg", -49: "sky", -64: "sky", -75: "sky", -100: "recip_box",
        -120: "recip_box", -140: "recip_nr", 10: None, 40: "sphere_seg", 64: "sky"}
M1_SAME = (-20, -31, -47, -49, -64, 10)  # power-of-two scaling is exact: the k = 0 frame's counters
M2_TINY = (("2^-99", p2(-99)), ("2^-100", p2(-100)), ("below2^-100", below(p2(-100))), ("2^-110", p2(-110)),
           ("2^-126", p2(-126)), ("2^-127", p2(-127)), ("2^-149", p2(-149)))
# (c = nextbelow(2^126), 2^126, 2^127 and a fan crossing 2^126 miss everything and dot(d, d)
# overflows: one sky colour in the oracle on every lattice, under the cap, so they are no fixtures)

# the fans whose d.x = s horizontal.x crosses a bound between the first and the later columns
M2_CROSS = (("2^-100", "recip_box", p2(-96)), ("2^-126", "recip_nr", p2(-122)))

# direction scales that are no power of two, so that dot(d, d) in [1, 1.55] f^2 straddles a bound
# inside the frame: sphere_seg's 2^-60 and 2^60, the sky's 2^-96 and 2^126
M1_CROSS = (("a_lo", "sphere_seg", -30), ("a_hi", "sphere_seg", 30), ("dd_lo", "sky", -48), ("dd_hi", "sky", 63))

M3_S = (-12, -24, -30, -40, -50, 12, 18, 21, 24, 32, 62)
M4_S = (12, 21, 30)
M5_FACTORS = (1, 50, 99, 101, 1000)  # (1: a lattice with spheres has its own extent + 1 as its reach)
M6_COLOURS = (("2^-18", dict(colour=p2(-18))), ("2^17", dict(colour=p2(17))), ("neg0", dict(one=-0.0)),
              ("negative", dict(one=-0.5)), ("inf", dict(one=np.inf)), ("nan", dict(one=np.nan)))


def _guard_m2(c):
    a = abs(float(c))
    if a < 2.0 ** -126 or a >= 2.0 ** 126:
        return "recip_nr"
    return "recip_box" if a < 2.0 ** -100 else None


def families(kind, size):
    """Every fixture of one lattice: the candidates whose oracle frame meets the cap."""
    return [f for f in candidates(kind, size) if not under_cap(kind, size, f.name)]


def candidates(kind, size):
    fx = [_fx("M1_k0", _m1_cam(0), expect="hit_mostly" if kind in ("box", "tri") else None)]
    for shift in (0, -1):
        tag = "" if shift == 0 else "_shifted"
        for k, guard in M1_K.items():
            flat = k in (-140, 64)
            expect = "same_as_unscaled" if k in M1_SAME else ("must_miss" if k in (40, 64) and kind != "mixed" else None)  # (a plane gates on its denominator)
            twin = "M1_k0" + tag
            if kind in ("sphere", "mixed") and expect == "same_as_unscaled":
                # A glass sphere passes the scale on (reflect(d, n) and refract are not normalised),
                # and the ray that leaves its surface finds the surface again at a root of rounding
                # error / |d|, which is compared with t_min = 0.001: that does not scale (the diffuse
                # copies of these scenes do keep their counters). From k = -20 down every such root
                # is above t_min and the frames equal the k = -20 one while dot(d, d) stays normal.
                twin = "M1_k-20" + tag
                expect = expect if k in (-31, -47, -49) else None
            if k == -140 and kind in ("tri", "obb", "box"):
                expect = "nan_all"
            fx.append(_fx(f"M1_k{k}{tag}", _m1_cam(k), shift, expect=expect, twin=twin, guard=guard, flat=flat))
        if shift:
            fx.append(_fx("M1_k0" + tag, _m1_cam(0), shift))
        else:
            for cname, guard, k in M1_CROSS:
                f = F(0.85) * p2(k)
                cam = dict(pos=(0.0, 0.0, 0.0), ll=_times(D0, f), hor=_times(HOR, f), ver=_times(VER, f))
                fx.append(_fx(f"M1_cross_{cname}", cam, guard=guard, mode="cross"))
        for sign, sname in ((1.0, "+"), (-1.0, "-")):
            for cname, c in M2_TINY:
                fx.append(_fx(f"M2_{sname}{cname}{tag}", _m2_cam(F(sign) * c), shift, guard=_guard_m2(c),
                              expect="hit_mostly" if kind in ("box", "tri") else None))
        for cname, guard, hx in M2_CROSS:
            fx.append(_fx(f"M2_cross{cname}{tag}", _m2_cam(0.0, hx), shift, guard=guard, mode="cross"))
    for s in M3_S:
        guard, mode, kinds = M3_GUARD.get(s, (None, "all", ()))
        if kinds and kind not in kinds:
            guard = None
        fx.append(_fx(f"M3_s{s}", _m3_cam(s), scale=s, guard=guard, mode=mode))
    # M7: the scene at 2^20 with M1's camera at the origin and directions of 2^-64: a = dot(d, d)
    # ~ 2^-128 is a denormal (recip_nr's estimate of its reciprocal overflows) while disc ~ 2^-88
    # and |b| ~ 2^-42 are inside sphere_roots_fast's window, so only sphere_seg keeps the lane
    # off the fast sequence; the roots, of order 2^86, are hits.
    fx.append(_fx("M7_s20_k-64", _m1_cam(-64), scale=20, guard="sphere_seg"))
    # the same scene with directions of 2^-98: no component is clamped (all but a few are above
    # 2^-100) and the hits lie at t ~ 2^120: on the BVH lattices the tiny-direction list walk
    # (a sphere-only lattice misses everything there: no fixture)
    if kind != "sphere":
        fx.append(_fx("M7_s20_k-98", _m1_cam(-98), scale=20, guard="sky"))
    # M8: M2's fan with every component tiny: d.y, d.z of order 2^-98 put the hits at t of order
    # 2^99 .. 2^102, where the clamp of 1 / d.x = 2^110 to 2^100 decides which cells are hit (the
    # x slab of a cell is 2^100 (c - o), not 2^110 (c - o))
    # (a sphere-only lattice misses everything there, and +2^-110 on the shifted lattice shows
    # fewer than 50 colours: no fixtures)
    for shift, sign, sname in ((0, 1.0, "+"), (0, -1.0, "-"), (-1, -1.0, "-")):
        if kind != "sphere":
            f = p2(-98)
            cam = dict(pos=(0.0, 0.0, 0.0), ll=(F(sign) * p2(-110), F(-0.5) * f, -f), hor=(0.0, f, 0.0), ver=(0.0, 0.0, F(-0.5) * f))
            fx.append(_fx(f"M8_{sname}2^-110_at2^-98" + ("" if shift == 0 else "_shifted"), cam, shift, guard="recip_box"))
    for s in M4_S:
        if s == 30 and (kind, size) != ("box", "small"):
            continue  # all NaN: one such case is kept
        fx.append(_fx(f"M4_s{s}", _m4_cam(s), scale=s, flat=s == 30, expect="nan_all" if s == 30 else None))
    if size == "big":
        unit = F(extent(lattice(kind, size)) + 1.0)
        for f in M5_FACTORS:
            fx.append(_fx(f"M5_x{f}", _m5_cam(unit, f), guard="reach" if f > 100 else None))
    if kind in ("box", "mixed") and size in ("small", "big"):
        for cname, kw in M6_COLOURS:
            fx.append(_fx(f"M6_{cname}", M6_CAM, **kw))
    return fx


# M3: the guard left at each scale (measured on the primary rays): with spheres in the scene,
# disc ~ 2^-120 at -30 and |b| > 2^40 from +18 (+21 with the mixed lattice's fewer spheres) put
# every root outside sphere_roots_fast's window, and at -24 disc = 2^-96 (r^2 |d|^2 - |oc x d|^2)
# crosses its lower bound inside each sphere's silhouette; a = dot(d, d) leaves [2^-60, 2^60]
# at -40 and +32, the sky's dd goes below 2^-96 at -50
_SPH = ("sphere", "mixed")
M3_GUARD = {-24: ("sphere_roots", "cross", _SPH), -30: ("sphere_roots", "all", _SPH), -40: ("sphere_seg", "all", ()),
            -50: ("sky", "all", ()), 18: ("sphere_roots", "all", ("sphere",)), 21: ("sphere_roots", "all", _SPH),
            24: ("sphere_roots", "all", _SPH), 32: ("sphere_seg", "all", ()), 62: ("sphere_seg", "all", ())}

# Fixtures whose oracle frame shows fewer than 128 distinct colours without being one of the
# named flat frames: {name: {(kind, size): the measured count}}. They are left out: a frame that
# is nearly constant or nearly all NaN compares little. (More than the values first expected to
# fall short: every sphere lattice is all NaN from k = -75, the mixed lattices keep too few
# colours at k = -100, -120 and, through their planes, at +64, the triangle lattices at s = -40.)
UNDER_CAP = {
    "M1_k-75": {("sphere", "small"): 1, ("sphere", "mid"): 1, ("sphere", "big"): 1, ("tri", "small"): 98},
    "M1_k-75_shifted": {("sphere", "small"): 1, ("sphere", "mid"): 1, ("sphere", "big"): 1,
        ("tri", "small"): 75, ("mixed", "big"): 121},
    "M1_k-100": {("box", "small"): 1, ("box", "mid"): 1, ("box", "big"): 1, ("sphere", "small"): 1,
        ("sphere", "mid"): 1, ("sphere", "big"): 1, ("tri", "small"): 98, ("mixed", "small"): 98,
        ("mixed", "mid"): 94, ("mixed", "big"): 112},
    "M1_k-120": {("box", "small"): 1, ("box", "mid"): 1, ("box", "big"): 1, ("sphere", "small"): 1,
        ("sphere", "mid"): 1, ("sphere", "big"): 1, ("tri", "small"): 98, ("mixed", "small"): 98,
        ("mixed", "mid"): 91, ("mixed", "big"): 101},
    "M1_k-100_shifted": {("box", "small"): 1, ("box", "mid"): 1, ("box", "big"): 1, ("sphere", "small"): 1,
        ("sphere", "mid"): 1, ("sphere", "big"): 1, ("tri", "small"): 75, ("mixed", "small"): 67,
        ("mixed", "mid"): 125, ("mixed", "big"): 110},
    "M1_k-120_shifted": {("box", "small"): 1, ("box", "mid"): 1, ("box", "big"): 1, ("sphere", "small"): 1,
        ("sphere", "mid"): 1, ("sphere", "big"): 1, ("tri", "small"): 75, ("mixed", "small"): 65,
        ("mixed", "mid"): 120, ("mixed", "big"): 98},
    "M1_k64": {("mixed", "small"): 31, ("mixed", "mid"): 103, ("mixed", "big"): 86},
    "M1_k64_shifted": {("mixed", "small"): 60, ("mixed", "mid"): 78, ("mixed", "big"): 94},
    "M7_s20_k-98": {("tri", "small"): 98},
    "M3_s-40": {("tri", "small"): 53, ("tri", "mid"): 20, ("tri", "big"): 14},
    "M3_s24": {("sphere", "mid"): 125, ("sphere", "big"): 91, ("obb", "mid"): 116},
    "M3_s32": {("box", "small"): 118, ("box", "mid"): 15, ("box", "big"): 62, ("obb", "small"): 115,
        ("obb", "mid"): 9, ("obb", "big"): 62, ("tri", "small"): 104, ("tri", "mid"): 45, ("tri", "big"): 26,
        ("mixed", "small"): 100, ("mixed", "mid"): 45, ("mixed", "big"): 38},
    "M3_s62": {("box", "small"): 118, ("box", "mid"): 15, ("box", "big"): 62, ("obb", "small"): 115,
        ("obb", "mid"): 9, ("obb", "big"): 62, ("mixed", "small"): 100, ("mixed", "mid"): 89,
        ("mixed", "big"): 62},
}


def under_cap(kind, size, name):
    return (kind, size) in UNDER_CAP.get(name, {})


_families = {}


def fixture(kind, size, name):
    if (kind, size) not in _families:
        _families[kind, size] = {f.name: f for f in candidates(kind, size)}
    return _families[kind, size][name]


def scene(kind, size, fx, variant="full"):
    prims = lattice(kind, size, fx.shift, variant)
    if fx.scale:
        prims = scaled(prims, fx.scale)
    if fx.colour is not None or fx.one is not None:
        prims = coloured(prims, fx.colour, fx.one)
    return prims


def frame(fx):
    """(width, height, spp) of a fixture's frames. M6 renders its 1024 samples as 32 x 32 pixels
    of one sample, so that the mean is the sample: a path's product of eight 2^-18 colours is a
    denormal that any shallower sample of the same pixel would swallow."""
    return (32, 32, 1) if fx.name.startswith("M6") else (W, H, SPP)


def cameras(fr, fx):
    w, h, _ = frame(fx)
    return edge_camera(fr, w=w, h=h, **fx.cam)


_reference = {}


def reference(fr, kind, size, variant, name, depth):
    """(prims, mean, u8, counters) of the oracle's render of one fixture, computed once and
    shared (read-only) by every test that compares against it."""
    key = (kind, size, variant, name, depth)
    if key not in _reference:
        fx = fixture(kind, size, name)
        prims = scene(kind, size, fx, variant)
        w, h, spp = frame(fx)
        mean, u8, cnt, _ = O.render(prims, cameras(fr, fx)[1], w, h, spp, depth, seed=SEED)
        mean.setflags(write=False)
        u8.setflags(write=False)
        _reference[key] = (prims, mean, u8, cnt)
    return _reference[key]


def cases():
    """(kind, size, family name): every value on the small and big lattices; on the mid one
    (12-B records) the guards' own bounds only."""
    mid = ("M1_k-31", "M1_k-49", "M1_k-140", "M1_k64", "M2_+below2^-100", "M2_-2^-149_shifted", "M2_cross2^-100",
           "M2_cross2^-126_shifted", "M3_s-30", "M3_s21", "M4_s21")
    out = []
    for kind in KINDS:
        for size in SIZES:
            for fx in families(kind, size):
                if fx.name.startswith("M1_k0"):
                    continue  # the unscaled twin: a reference for same_as_unscaled, nothing new for a kernel
                if size != "mid" or fx.name in mid:
                    out.append((kind, size, fx.name))
    return out
