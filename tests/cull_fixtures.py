"""Scenes and rays at the edge of the tree's cull (bvh.h): rays whose sphere test accepts a root by
rounding error although the ray passes outside the sphere. Shared by tests/test_cull_fixtures.py,
tests/test_cull_host.py and tests/test_cull.py; not a test module.

The sphere test's discriminant b b - a cc carries an absolute error of order 2^-24 |o - c|^2 a, so
from far away it accepts rays that pass a small sphere at several radii ("false accepts": the
oracle does, and the product must return what the oracle returns). The cull in front of the test
must not reject them. Families, each built from seeded numpy generators with f32 coordinates:

- sparse_extreme: 64 spheres of radius 0.25 with centres in +-4950 and sphere 0 at (5000, 0.5,
  -0.25), the scene's extreme on +x. Origins lie in the plane x = c0.x + r + delta, delta in
  [0.55, 0.95], which is beyond sphere 0's bounds padded by 1e-4 (extent + 1) = 0.5; y and z are
  uniform in +-5000. Each ray is aimed at (o.x, c0.y, c0.z) with a unit direction, so d.x == 0 ("flat"), or at a
  point up to 0.3 units farther from the scene, d.x >= 0 ("tilted").
- sparse_random: 10,000 spheres of radius 2.5 with centres in +-5000 (the shape of the generator's
  10,000-sphere scene); origins uniform in the scene, each ray aimed to pass a random sphere at
  1 to 2.5 radii.
- tiny_dir: 64 spheres of radius 1 (and of radius 0.125) in +-7.92 with sphere 0 at (8, 0.5,
  -0.25); origins in the plane x = c0.x + r + delta, delta = pad U(1.02, 1.6) for the scene's
  padding, y and z within +-min(8 + r, 20 r), aimed as above with d.x == 0 and the unit direction
  scaled by 2^k: at |d| ~ 2^-69 the products of the discriminant are denormals of a few ulps.
- other_kinds: 2,000 boxes, triangles or oriented boxes of half size 0.25 or 0.004 in +-5000 with
  rays aimed within two sizes of a primitive, from inside the scene and, for the small size, from
  the shell at 99 (extent + 1). Their tests' error is linear in |o|: the padding holds them.

A family is {"prims", "o", "d" [n, 3] f32}; hits(), false_accepts() and subset() below are computed
once per family and shared, read-only."""
import numpy as np

from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import ray_edge_fixtures as X

F = np.float32
TINY_K = (-59.0, -66.0, -68.0, -69.0, -69.2, -69.45, -69.9)  # (-59: above the tiny-direction limit, the tree walks it)
TINY_R = (1.0, 0.125)
SPHERE_FAMILIES = (["sparse_extreme_flat", "sparse_extreme_tilted", "sparse_random"] +
                   [f"tiny_dir_r{r}_k{k}" for r in TINY_R for k in TINY_K])
OTHER = [(kind, half, where) for kind in ("box", "tri", "obb") for half, where in ((0.25, "inside"), (0.004, "inside"), (0.004, "shell"))]
OTHER_FAMILIES = [f"other_{kind}_{half}_{where}" for kind, half, where in OTHER]
# bvh.h: the sphere test accepts p^2 < r^2 + DISC_ERR |o - c|^2 + DISC_ABS
DISC_ERR = 20.0 * 2.0 ** -24  # kSphereDiscErr
DISC_ABS = 2.0 ** -28         # kSphereDiscAbs


def _mat(n):
    return n % 4, (0.25 + (n % 8) / 16.0, 0.25 + ((n // 8) % 8) / 16.0, 0.5 + (n % 3) / 8.0)


def _spheres(centres, radius):
    out = []
    for n, c in enumerate(np.asarray(centres, F)):
        mat, col = _mat(n)
        out.append(S.sphere([float(x) for x in c], radius, mat, col, 0.0))
    return out


def pad_of(prims):
    """The boxes' padding before sphere bounds grew: 1e-4 (extent + 1), from the upper bound of the extent."""
    return 1e-4 * (CF.extent_bounds(prims)[1] + 1.0)


def _plane_rays(rng, c0, r, delta, span, n, tilt=0.0):
    """Origins in the plane x = c0.x + r + delta, y and z uniform in +-span, aimed at (o.x, c0.y, c0.z)."""
    o = np.empty((n, 3), F)
    o[:, 0] = (F(c0[0]) + F(r) + delta.astype(F)).astype(F)
    o[:, 1:] = rng.uniform(-span, span, (n, 2)).astype(F)
    # a unit direction (formed in float64): with d = target - o in f32 the test's b would be -a
    # bit for bit and its rounding errors would cancel
    t = np.zeros((n, 3))
    t[:, 1:] = np.asarray(c0[1:], np.float64)[None, :] - o[:, 1:]
    if tilt:  # the target moved by up to `tilt` units away from the scene
        t[:, 0] = rng.uniform(0.0, tilt, n)
    return o, (t / np.linalg.norm(t, axis=1)[:, None]).astype(F)


def _sparse_extreme_prims():
    c = np.random.default_rng(2).uniform(-4950.0, 4950.0, (64, 3)).astype(F)
    c[0] = (5000.0, 0.5, -0.25)
    return _spheres(c, 0.25)


def _sparse_extreme(tilted):
    prims = _sparse_extreme_prims()
    rng = np.random.default_rng(31 if tilted else 30)
    n = 4096
    o, d = _plane_rays(rng, prims[0]["g"][:3], 0.25, rng.uniform(0.55, 0.95, n), 5000.0, n, 0.3 if tilted else 0.0)
    return prims, o, d


def _aimed(rng, centres, size, lo, hi, o):
    """Directions from o that pass a random centre at size * U(lo, hi)."""
    n = len(o)
    c = centres[rng.integers(0, len(centres), n)].astype(np.float64)
    to = c - o
    v = np.cross(to, rng.normal(size=(n, 3)))
    v /= np.linalg.norm(v, axis=1)[:, None]
    target = c + v * (size * rng.uniform(lo, hi, n))[:, None]
    return (target - o).astype(F)


def _sparse_random():
    rng = np.random.default_rng(4)
    c = rng.uniform(-5000.0, 5000.0, (10000, 3)).astype(F)
    o = rng.uniform(-5000.0, 5000.0, (50000, 3)).astype(F)
    return _spheres(c, 2.5), o, _aimed(rng, c, 2.5, 1.0, 2.5, o)


def _tiny_prims(radius):
    c = np.random.default_rng(5).uniform(-7.92, 7.92, (64, 3)).astype(F)
    c[0] = (8.0, 0.5, -0.25)
    return _spheres(c, radius)


def _tiny_dir(radius, k):
    prims = _tiny_prims(radius)
    rng = np.random.default_rng(6)
    n = 20000
    o, d = _plane_rays(rng, prims[0]["g"][:3], radius, pad_of(prims) * rng.uniform(1.02, 1.6, n), min(8.0 + radius, 20.0 * radius), n)
    d = (d * F(2.0 ** k)).astype(F)
    keep = np.abs(d).max(axis=1) >= F(2.0 ** -70)
    return prims, o[keep], d[keep]


def _other(kind, half, where):
    rng = np.random.default_rng(7)
    c = rng.uniform(-5000.0, 5000.0, (2000, 3)).astype(F)
    prims = []
    for n, cc in enumerate(c):
        mat, col = _mat(n)
        x, y, z = (float(v) for v in cc)
        if kind == "box":
            g = [x - half, y - half, z - half, x + half, y + half, z + half]
            prims.append(S.prim(S.AABB, mat, col, 0.0, g))
        elif kind == "tri":
            prims.append(S.prim(S.TRIANGLE, mat, col, 0.0, [x - half, y - half, z, x + half, y - half, z, x, y + half, z + half]))
        else:
            a = rng.normal(size=3)
            a /= np.linalg.norm(a)
            b = np.cross(a, rng.normal(size=3))
            b /= np.linalg.norm(b)
            prims.append(S.prim(S.OBB, mat, col, 0.0, [x, y, z] + list(a) + list(b) + list(np.cross(a, b)) + [half] * 3))
    n = 20000
    if where == "inside":
        o = rng.uniform(-5000.0, 5000.0, (n, 3))
    else:  # on the cube |o|_inf = 99 (extent + 1): inside the reach of 100
        o = rng.uniform(-1.0, 1.0, (n, 3))
        o /= np.abs(o).max(axis=1)[:, None]
        o *= 99.0 * (CF.extent_bounds(prims)[0] + 1.0)
    o = o.astype(F)
    return prims, o, _aimed(rng, c, half, 0.0, 2.0, o)


_families, _hits, _subsets = {}, {}, {}


def family(name):
    if name not in _families:
        if name.startswith("sparse_extreme"):
            prims, o, d = _sparse_extreme(name.endswith("tilted"))
        elif name == "sparse_random":
            prims, o, d = _sparse_random()
        elif name.startswith("tiny_dir"):
            _, _, r, k = name.split("_")
            prims, o, d = _tiny_dir(float(r[1:]), float(k[1:]))
        else:
            prims, o, d = _other(*OTHER[OTHER_FAMILIES.index(name)])
        o.setflags(write=False)
        d.setflags(write=False)
        _families[name] = {"prims": prims, "o": o, "d": d}
    return _families[name]


# the GPU subset of sparse_random is drawn from its first rays only: the oracle's loop over 10,000
# spheres takes 0.6 ms a ray, and the whole family is walked on the CPU (tests/test_cull_host.py)
POOL = {"sparse_random": 6144}


def hits(name, pool=None):
    """cast_fixtures.hits of the whole family (of its first `pool` rays), computed once."""
    if name in _hits:
        return _hits[name] if pool is None else {k: v[:pool] for k, v in _hits[name].items()}
    f = family(name)
    if pool is None:
        _hits[name] = CF.hits(f["prims"], f["o"], f["d"])
        return _hits[name]
    if (name, pool) not in _hits:
        _hits[name, pool] = CF.hits(f["prims"], f["o"][:pool], f["d"][:pool])
    return _hits[name, pool]


def passing_distance(prims, o, d, prim):
    """(p, r, L) in float64: the distance at which ray i passes the centre of sphere prim[i], that
    sphere's radius and |o - c| (nan where prim[i] is a miss or no sphere)."""
    n = len(o)
    p, r, dist = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    g = np.array([q["g"][:4] if q["kind"] == S.SPHERE else [np.nan] * 4 for q in prims], np.float64)
    sel = prim != CF.MISS
    gg = g[prim[sel]]
    oc = o[sel].astype(np.float64) - gg[:, :3]
    dd = d[sel].astype(np.float64)
    p[sel] = np.linalg.norm(np.cross(oc, dd), axis=1) / np.linalg.norm(dd, axis=1)
    r[sel] = np.abs(gg[:, 3])
    dist[sel] = np.linalg.norm(oc, axis=1)
    return p, r, dist


def false_accepts(name, pool=None):
    """[n] bool: the oracle's winner is a sphere the ray passes outside, in float64."""
    f, h = family(name), hits(name, pool)
    p, r, _ = passing_distance(f["prims"], f["o"][:pool], f["d"][:pool], h["prim"])
    return p > r


def outside_old_boxes(name):
    """[n] bool: o.x beyond sphere 0's +x face padded by 1e-4 (extent + 1) and d.x >= 0, where
    sphere 0 is the scene's extreme on +x: such a ray touches no box padded that way."""
    f = family(name)
    g = [p["g"] for p in f["prims"]]
    assert all(float(q[0]) + abs(float(q[3])) < float(g[0][0]) + abs(float(g[0][3])) for q in g[1:])
    face = float(g[0][0]) + abs(float(g[0][3])) + pad_of(f["prims"])
    return (f["o"][:, 0].astype(np.float64) > face) & (f["d"][:, 0] >= 0)


def subset(name):
    """The GPU batch of a family (of its first POOL rays): {"prims", "o", "d", "want" (hits),
    "false" [m] bool}: the false accepts first, then as many ordinary rays, 4096 at most and no multiple of 64."""
    if name not in _subsets:
        f, h, fa = family(name), hits(name, POOL.get(name)), false_accepts(name, POOL.get(name))
        a, b = np.nonzero(fa)[0][:2048], np.nonzero(~fa)[0]
        sel = np.concatenate([a, b[:max(len(a), 64)]])[:4095]
        if len(sel) % 64 == 0:
            sel = np.concatenate([sel, b[-1:]])
        want = {k: v[sel] for k, v in h.items()}
        for v in want.values():
            v.setflags(write=False)
        _subsets[name] = {"prims": f["prims"], "o": f["o"][sel], "d": f["d"][sel], "want": want, "false": fa[sel]}
    return _subsets[name]


GPU_FAMILIES = ["sparse_extreme_flat", "sparse_extreme_tilted", "sparse_random"] + \
    [f"tiny_dir_r{r}_k{k}" for r in TINY_R for k in (-59.0, -68.0, -69.2, -69.45)]


# ---- the views ---------------------------------------------------------------------------------

W, H, SPP, SEED = 16, 16, 4, 5


def _plane_fields(pos, aim, half, scale=1.0):
    """edge_camera fields of a view from pos whose rays stay in the plane x = pos.x (lower_left.x
    = pos.x and no x in horizontal or vertical: d.x == 0 exactly) and pass the point pos + aim at
    256 lateral offsets within about +-half: d = scale (aim + q half ((2u - 1) + (2v - 1) / 16)),
    q the unit vector across the aim."""
    ay, az = float(aim[0]), float(aim[1])
    n = np.hypot(ay, az)
    qy, qz = -az / n * half, ay / n * half
    ll = (float(pos[0]), float(pos[1]) + scale * (ay - qy * (1.0 + 1.0 / 16.0)), float(pos[2]) + scale * (az - qz * (1.0 + 1.0 / 16.0)))
    return dict(pos=tuple(float(F(v)) for v in pos), ll=tuple(float(F(v)) for v in ll),
                hor=(0.0, float(F(scale * 2.0 * qy)), float(F(scale * 2.0 * qz))),
                ver=(0.0, float(F(scale * qy / 8.0)), float(F(scale * qz / 8.0))))


def _view(fr, prims, fields, need=8):
    """The view's record if its oracle G-buffer holds `need` false-accept pixels of sphere 0 and
    the oracle's frames at depth 8 and 12 count a hit in `need` of them, else None."""
    from oracle import oracle_py as O
    from tests import gbuffer_ref as G
    cam, ocam = X.edge_camera(fr, w=W, h=H, **fields)
    gb = G.gbuffer(prims, ocam, W, H)
    pos, d = G.primary_rays(ocam, W, H)
    o = np.tile(pos, (W * H, 1)).astype(F)
    p, r, _ = passing_distance(prims, o, d.reshape(-1, 3), gb["prim"].reshape(-1))
    fa = ((p > r) & (gb["prim"].reshape(-1) == 0)).reshape(H, W)
    if fa.sum() < need or not (d[..., 0] >= 0).all():
        return None
    frames = {}
    for depth in (8, 12):
        mean, u8, cnt, _ = O.render(prims, ocam, W, H, SPP, depth, seed=SEED)
        # the frame without sphere 0 (a stub in its place): a pixel that differs counted a hit of it
        bare = O.render([S.prim(S.STUB)] + prims[1:], ocam, W, H, SPP, depth, seed=SEED)[0]
        hit = (mean.view(np.uint32) != bare.view(np.uint32)).any(axis=2)
        if (hit & fa).sum() < need:
            return None
        mean.setflags(write=False)
        u8.setflags(write=False)
        frames[depth] = (prims, mean, u8, cnt, hit)
    return {"prims": prims, "cam": cam, "ocam": ocam, "gbuffer": gb, "false": fa, "frames": frames, "o": o, "d": d.reshape(-1, 3)}


_views = {}


def extreme_view(fr):
    """A 16 x 16 view of the sparse_extreme scene from its outside plane (within the reach) whose
    oracle G-buffer holds at least 8 false-accept pixels with d.x >= 0, and whose oracle frames
    (4 spp, depth 8 and 12) count a hit in at least 8 of those pixels: the first of a seeded
    sequence of candidates."""
    if "extreme" not in _views:
        prims = _sparse_extreme_prims()
        c0 = prims[0]["g"][:3]
        rng = np.random.default_rng(40)
        for _ in range(200):
            delta, y, z = rng.uniform(0.55, 0.95), rng.uniform(-5000.0, 5000.0), rng.uniform(-5000.0, 5000.0)
            pos = (F(F(c0[0]) + F(0.25)) + F(delta), F(y), F(z))
            v = _view(fr, prims, _plane_fields(pos, (float(c0[1]) - float(pos[1]), float(c0[2]) - float(pos[2])), 1.0))
            if v:
                _views["extreme"] = v
                break
    return _views["extreme"]


def tiny_view(fr):
    """The tiny_dir scene of unit spheres moved so that a point of sphere 0's outside plane is the
    origin, seen from a camera at exactly 0 whose fields are scaled so that |d| is about 2^-69.45
    (an M1-style camera, tests/magnitude_fixtures.py): the same conditions as extreme_view, with
    the padding recomputed for the moved scene."""
    if "tiny" not in _views:
        base = _tiny_prims(1.0)
        c = np.array([p["g"][:3] for p in base], np.float64)
        rng = np.random.default_rng(41)
        for _ in range(200):
            y, z, f = rng.uniform(-9.0, 9.0), rng.uniform(-9.0, 9.0), rng.uniform(1.02, 1.6)
            delta = 3e-3
            for _ in range(3):  # delta = f pad of the moved scene, whose extent depends on delta
                at = np.array([c[0, 0] + 1.0 + delta, y, z])
                prims = _spheres((c - at).astype(F), 1.0)
                delta = f * pad_of(prims)
            c0 = prims[0]["g"][:3].astype(np.float64)
            if not -(c0[0] + 1.0) > 1.01 * pad_of(prims):
                continue
            aim = (c0[1], c0[2])
            v = _view(fr, prims, _plane_fields((0.0, 0.0, 0.0), aim, 0.02, 2.0 ** -69.45 / np.hypot(*aim)))
            if v:
                _views["tiny"] = v
                break
    return _views["tiny"]
