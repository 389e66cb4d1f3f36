"""Ray batches and oracle references for the ray-query tests (fr_ctx_cast): shared by
tests/test_cast_fixtures.py, tests/test_cast_host.py and tests/test_cast.py; not a test module.

A batch for a lattice kind (tests/ray_edge_fixtures.py, the "big" lattice at shift 0) is, in order:
- the primary rays of the R0_control edge camera at 16 x 16;
- one bounce ray from every hit of those: o = P, d = N + r, r uniform in [-1, 1)^3 from a seeded
  numpy generator, in f32;
- the primary rays of every edge family of families(kind) at 8 x 8 (a family built for the shifted
  lattice has its origins moved by -shift in x, which is exact on the dyadic lattice);
- a tail of special rays: a zero direction, a NaN origin component, an origin at 1,000 reach
  units, a direction of 2^-80 in every component, and an origin of 2^30 beside a zero direction
  component (o / d overflows).
Copies of the first four specials are also placed in the first two waves of 64 rays, so a batch
holds waves that walk the tree and waves that fall back to the list, and one ordinary ray is
appended if the length is a multiple of 64.

The expected hit of a ray is the oracle's: winner and normal from oracle_closest_hit, the
winner's own root from the list cut after the winner, the point and the albedo restated in numpy
(tests/gbuffer_ref.py does the same per pixel)."""
import ctypes as C

import numpy as np

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import gbuffer_ref as G
from tests import ray_edge_fixtures as X

F = np.float32
MISS = G.MISS
SEED = 0xCA57
TINY_DIR = F(2.0 ** -60)      # bvh.h kBvhTinyDir
INV_CLAMP = F(2.0 ** 100)     # rt_core.h kBoxInvClamp, bvh.h kBvhInvClamp
REACH_UNITS = 100.0           # bvh.h kBvhOriginReach


# ---- the oracle's hit of arbitrary rays ------------------------------------------------------

def hits(prims, o, d):
    """{"prim" [n] u32, "t" [n], "normal", "position", "albedo" [n, 3] f32, "stale" [n] bool} of
    rays o, d ([n, 3] f32)."""
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    n = len(o)
    arr = O.prims_to_c(prims)
    hit = O.lib().oracle_closest_hit
    out = {"prim": np.full(n, MISS, np.uint32), "t": np.zeros(n, F), "normal": np.zeros((n, 3), F),
           "position": np.zeros((n, 3), F), "albedo": np.ones((n, 3), F), "stale": np.zeros(n, bool)}
    rec, own = (C.c_float * 7)(), (C.c_float * 7)()
    for i in range(n):
        oo = (C.c_float * 3)(*[float(c) for c in o[i]])
        dd = (C.c_float * 3)(*[float(c) for c in d[i]])
        best = hit(arr, len(prims), oo, dd, rec)
        if best < 0:
            continue
        assert hit(arr, best + 1, oo, dd, own) == best  # the list cut after the winner
        t = F(own[0])
        out["prim"][i] = best
        out["t"][i] = t
        out["normal"][i] = np.array(rec[4:7], F)
        with np.errstate(all="ignore"):
            out["position"][i] = (o[i] + (t * d[i]).astype(F)).astype(F)
        out["albedo"][i] = G.albedo_of(prims[best])
        out["stale"][i] = np.float32(rec[0]).view(np.uint32) != t.view(np.uint32)
    for a in out.values():
        a.setflags(write=False)
    return out


def same(got, want, sel=slice(None)):
    """The names whose bits differ between two hit dicts (an empty list: equal)."""
    bad = []
    for name in ("prim", "t", "normal", "position", "albedo"):
        a, b = np.ascontiguousarray(got[name][sel]), np.ascontiguousarray(want[name][sel])
        if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            diff = np.nonzero(a.view(np.uint32).reshape(len(a), -1) != b.view(np.uint32).reshape(len(b), -1))[0] \
                if a.shape == b.shape else []
            bad.append((name, len(np.unique(diff)), [int(i) for i in np.unique(diff)[:8]]))
    return bad


def as_gbuffer(h, w, hh):
    """A hit dict of w * hh rays in pixel order as the G-buffer dict of that view."""
    return {"prim": h["prim"].reshape(hh, w), "depth": h["t"].reshape(hh, w), "normal": h["normal"].reshape(hh, w, 3),
            "position": h["position"].reshape(hh, w, 3), "albedo": h["albedo"].reshape(hh, w, 3)}


# ---- rays ----------------------------------------------------------------------------------

def camera_rays(ocam, w, h):
    """(o [w h, 3], d [w h, 3]) f32: the pinhole rays of a view in pixel order."""
    pos, d = G.primary_rays(ocam, w, h)
    return np.tile(pos, (w * h, 1)).astype(F), d.reshape(w * h, 3).copy()


def bounce_rays(o, d, ref, seed=SEED):
    """One ray from every hit of `ref` (hits() of o, d): o = P, d = N + r."""
    sel = ref["prim"] != MISS
    r = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(int(sel.sum()), 3)).astype(F)
    with np.errstate(all="ignore"):
        return ref["position"][sel].copy(), (ref["normal"][sel] + r).astype(F)


def extent_bounds(prims):
    """(lo, hi): bounds of bvh.cpp's extent, the largest |coordinate| of the primitives' bounds:
    lo from the boxes, spheres, triangles and planes, hi with every oriented box's corners bounded
    by the sum of its half sizes."""
    lo = hi = 0.0
    for p in prims:
        g = [float(x) for x in p["g"]]
        k = p["kind"]
        if k == S.SPHERE:
            m = max(abs(c) + abs(g[3]) for c in g[:3])
        elif k == S.AABB:
            m = max(abs(c) for c in g[:6])
        elif k == S.TRIANGLE:
            m = max(abs(c) for c in g[:9])
        elif k == S.PLANE:
            m = max(abs(g[i]) + abs(g[6 + i]) for i in range(3))
        elif k == S.OBB:
            hi = max(hi, max(abs(c) for c in g[:3]) + sum(abs(c) for c in g[12:15]))
            continue
        else:
            continue
        lo, hi = max(lo, m), max(hi, m)
    return lo, hi


def specials(prims):
    """(names, o [5, 3], d [5, 3]) of the tail."""
    far = F(1000.0 * REACH_UNITS * (extent_bounds(prims)[1] + 1.0))
    assert far < 2.0 ** 27
    rows = [
        ("zero_direction", (0.25, 0.5, 0.5), (0.0, 0.0, 0.0)),
        ("nan_origin", (0.25, np.nan, 0.5), (0.1, 0.2, -1.0)),
        ("far_origin", (far, 0.25, -4.25), (-1.0, 0.0, 0.0)),
        ("tiny_direction", (0.25, 0.5, 0.5), (2.0 ** -80, 2.0 ** -80, -(2.0 ** -80))),
        ("overflow_oinv", (0.25, 2.0 ** 30, -4.25), (-1.0, 0.0, 0.0)),
    ]
    return [r[0] for r in rows], np.array([r[1] for r in rows], F), np.array([r[2] for r in rows], F)


def fallback_terms(o, d, reach_lo, reach_hi):
    """cast.h's three fallback conditions per ray, each as a ([n] bool "true for sure", [n] bool
    "false for sure") pair: the origin test against a reach known only to lie in [reach_lo,
    reach_hi]. A NaN component of o fails the first and the third; the second asks for one
    direction component of 2^-60 or more."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    with np.errstate(all="ignore"):
        ad = np.fmax.reduce(np.abs(d), axis=1)
        inv = (F(1.0) / d).astype(F)
        inv = np.fmin(np.fmax(inv, -INV_CLAMP), INV_CLAMP)  # minNum / maxNum: a NaN reciprocal becomes -2^100
        oi = np.abs((o * inv).astype(F))
        far = (~(np.abs(o) <= F(reach_hi)).all(axis=1), (np.abs(o) <= F(reach_lo)).all(axis=1))
        fin = (oi <= np.finfo(F).max).all(axis=1)
    return {"far_origin": far, "tiny_direction": (~(ad >= TINY_DIR), ad >= TINY_DIR), "overflow_oinv": (~fin, fin)}


def falls_back(prims, o, d):
    """[n] bool: the rays that take the list, which must not depend on where in its bounds the
    scene's reach lies."""
    terms = fallback_terms(o, d, *reach_bounds(prims))
    assert all((yes ^ no).all() for yes, no in terms.values())
    return terms["far_origin"][0] | terms["tiny_direction"][0] | terms["overflow_oinv"][0]


def reach_bounds(prims):
    """bvh_origin_reach lies in [extent + 1, 100 (extent + 1)]."""
    lo, hi = extent_bounds(prims)
    return lo + 1.0, REACH_UNITS * (hi + 1.0)


_batches = {}


def lattice_prims(kind):
    return X.lattice(kind, "big", 0)


def batch(fr, kind):
    """{"prims", "o", "d" [n, 3] f32, "label" [n] str: "primary", "bounce", "family:<name>" or
    "special:<name>" per ray, "special": the indices of the special rays} for a lattice kind,
    computed once."""
    if kind in _batches:
        return _batches[kind]
    prims = lattice_prims(kind)
    os_, ds_, lab = [], [], []

    def add(name, o, d):
        os_.append(np.asarray(o, F))
        ds_.append(np.asarray(d, F))
        lab.extend([name] * len(o))

    fx0 = X.fixture(kind, "R0_control")
    o, d = camera_rays(X.edge_camera(fr, w=16, h=16, **fx0.cam)[1], 16, 16)
    add("primary", o, d)
    add("bounce", *bounce_rays(o, d, hits(prims, o, d)))
    for fx in X.families(kind):
        o, d = camera_rays(X.edge_camera(fr, w=8, h=8, **fx.cam)[1], 8, 8)
        o[:, 0] = (o[:, 0] - F(fx.shift)).astype(F)
        add("family:" + fx.name, o, d)
    o, d = np.concatenate(os_), np.concatenate(ds_)
    names, so, sd = specials(prims)
    # copies of the first four specials inside waves 0 and 1 (ascending positions, each the final
    # index of its ray), then the tail
    for pos, k in ((3, 0), (40, 1), (64 + 17, 2), (64 + 50, 3)):
        o, d = np.insert(o, pos, so[k], axis=0), np.insert(d, pos, sd[k], axis=0)
        lab.insert(pos, "special:" + names[k])
    o, d = np.concatenate([o, so]), np.concatenate([d, sd])
    lab += ["special:" + nm for nm in names]
    if len(o) % 64 == 0:
        o, d = np.concatenate([o, o[200:201]]), np.concatenate([d, d[200:201]])
        lab.append(lab[200])
    lab = np.array(lab)
    special = [int(i) for i in np.nonzero(np.char.startswith(lab, "special:"))[0]]
    for a in (o, d, lab):
        a.setflags(write=False)
    _batches[kind] = {"prims": prims, "o": o, "d": d, "label": lab, "special": special}
    return _batches[kind]


_refs = {}


def expected(fr, kind):
    """hits() of the kind's batch, computed once and shared, read-only."""
    if kind not in _refs:
        b = batch(fr, kind)
        _refs[kind] = hits(b["prims"], b["o"], b["d"])
    return _refs[kind]


def fallback_waves(b):
    """The waves of 64 rays of batch b that hold a ray which falls back."""
    return sorted({int(i) // 64 for i in np.nonzero(falls_back(b["prims"], b["o"], b["d"]))[0]})


# ---- the generator's sphere scenes -------------------------------------------------------------

_gen = {}


def gen_spheres(fr, count, w, h):
    """(json text, oracle prims, OrCamera) of tools/gen_scene.py's sphere scene at w x h."""
    key = (count, w, h)
    if key not in _gen:
        import importlib.util
        import os
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(root, "tools", "gen_scene.py"))
        gs = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gs)
        text = gs.dumps(gs.generator_scene(count, "sphere"))
        prims, (frm, at, vup, fov) = S.load_json(text)
        _gen[key] = (text, prims, O.camera_look(frm, at, vup, fov, 0.1, w, h))
    return _gen[key]


def gen_batch(fr, count, w, h):
    """(prims, o, d) of the w x h primary rays of the generator's sphere scene and their bounce
    rays, with the oracle's hits: computed once per (count, w, h)."""
    key = ("batch", count, w, h)
    if key not in _gen:
        _, prims, ocam = gen_spheres(fr, count, w, h)
        o, d = camera_rays(ocam, w, h)
        first = hits(prims, o, d)
        bo, bd = bounce_rays(o, d, first)
        o, d = np.concatenate([o, bo]), np.concatenate([d, bd])
        o.setflags(write=False)
        d.setflags(write=False)
        _gen[key] = (prims, o, d, hits(prims, o, d))
    return _gen[key]
