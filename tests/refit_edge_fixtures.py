"""Edge cases of the in-place scene edit (fr_scene_update): edits of a primitive's shape, edits at
the packed extent, radius edits in a scene whose reach is above its floor, and sequences of
updates. Shared by tests/test_refit_edge_fixtures.py, tests/test_refit_edges_host.py and
tests/test_refit_edges.py; not a test module.

Scenes and rays are those of tests/refit_fixtures.py (the big lattices, the batches of
tests/cast_fixtures.py), and an edit set touches the indices refit_fixtures.py holds to the
builder: two primitives of one leaf, a pair under the two children of one node and a primitive
under each child of the root. The shape edits leave a primitive where it is, deep in the lattice
for some, so every set comes with `aimed_rays`: short rays from around each edited primitive at
it. tests/test_refit_edge_fixtures.py holds the properties claimed here against the oracle and
tests/c/refit_check.cpp, so that none of the GPU tests passes vacuously."""
import copy

import numpy as np

from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import refit_fixtures as R

F = np.float32
KINDS = R.KINDS
NEG0 = -0.0


def touched(kind):
    """The indices every shape edit set of a kind holds (leaf pair, siblings, root sides)."""
    return list(dict.fromkeys(R.SAME_LEAF[kind] + R.SIBLINGS[kind] + R.ROOT_SIDES[kind]))


def with_g(p, changes):
    """A copy of primitive dict p with geometry words replaced: {word index: value}."""
    q = copy.deepcopy(p)
    g = [float(F(x)) for x in q["g"]]
    for k, v in changes.items():
        g[k] = float(F(v))
    q["g"] = g
    return q


def _rot(axis, degrees):
    """A rotation about a coordinate axis, in double."""
    a = np.deg2rad(degrees)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def rotated_obb(p, axis, degrees):
    """Oriented box p with its three axes turned about a coordinate axis, rounded to float32."""
    g = np.asarray(p["g"], np.float64)
    m = _rot(axis, degrees)
    ch = {}
    for j in range(3):
        v = (m @ g[3 + 3 * j:6 + 3 * j]).astype(F)
        for k in range(3):
            ch[3 + 3 * j + k] = v[k]
    return with_g(p, ch)


# ---- shape edits ---------------------------------------------------------------------------------

# What a set does to the boxes, which decides its control (tests/test_refit_edge_fixtures.py):
# "grows": a tree that is not refitted gives wrong hits (refit_check's stale >= 1);
# "shrinks": the old boxes still hold everything, so the control is that the refitted nodes differ
# from the first pack's; "same": the bounds keep their values (the records change).
EFFECT = {
    "sphere": {"shrink": "shrinks", "grow": "grows", "tiny": "shrinks", "zero_r": "shrinks", "neg_r": "grows",
               "neg_zero": "same"},
    "box": {"grow": "grows", "plate": "shrinks", "inverted": "same", "neg_zero": "shrinks"},  # (inverted: grow() sorts the corners)
    "obb": {"rotate": "grows", "halves": "grows", "neg_half": "shrinks", "zero_half": "shrinks", "turned_neg_half": "grows"},
    "tri": {"tilt": "grows", "degenerate": "shrinks", "collinear": "shrinks"},
    "mixed": {"all_kinds": "grows"},
}
# sets whose edited primitives no ray of the set hits in the oracle: a sphere of radius 0, an oriented
# box with two half sizes of 0, a box of no thickness. Their coverage is the equality of the tables.
# (A negative half size is no such set: the slab test takes the nearer and the farther plane of each
# pair, so the box is hit like the one with the half's magnitude.)
UNHITTABLE = {("sphere", "zero_r"), ("obb", "zero_half"), ("box", "plate"), ("tri", "degenerate"), ("tri", "collinear")}
# sets that change no hit of any ray: a zero's sign in a centre, and a box with two corners swapped
# (the slab test takes the nearer and the farther plane of each pair). The tables' bits are the check.
NO_HIT_CHANGE = {("sphere", "neg_zero"), ("box", "inverted")}
ROTATIONS = ((2, 17.0), (0, 30.0), (1, 45.0), (2, 60.0), (0, 17.0))  # (axis, degrees) per touched index


def _tilted(prims, i):
    """Triangle i with its quad's corner v11 (vertex 2 of the even triangle, vertex 0 of the odd
    one) lifted off the quad's plane by 0.75."""
    return with_g(prims[i], {8: float(prims[i]["g"][8]) + 0.75} if i % 2 == 0 else {2: float(prims[i]["g"][2]) + 0.75})


def shape_edits(kind):
    """{name: (indices [k] uint32, new primitive dicts [k])} against CF.lattice_prims(kind)."""
    prims = CF.lattice_prims(kind)
    idx = touched(kind)
    arr = np.array(idx, np.uint32)

    own = {"sphere": S.SPHERE, "box": S.AABB, "obb": S.OBB, "tri": S.TRIANGLE}.get(kind)

    def each(fn, mirror=0.0):
        """fn(position in the set, primitive) for the kind's own primitives. The set's last index is
        the mirror behind the camera, a box in every lattice but the spheres': it gets `mirror`
        added to its far side (z) where fn is for another kind."""
        return arr, [fn(n, prims[i]) if prims[i]["kind"] == own else with_g(prims[i], {5: float(prims[i]["g"][5]) + mirror})
                     for n, i in enumerate(idx)]

    if kind == "sphere":
        return {
            "shrink": each(lambda n, p: with_g(p, {3: 0.125})),
            "grow": each(lambda n, p: with_g(p, {3: 2.75})),
            "tiny": each(lambda n, p: with_g(p, {3: 2.0 ** -20})),
            "zero_r": each(lambda n, p: with_g(p, {3: 0.0})),
            "neg_r": each(lambda n, p: with_g(p, {3: -1.5})),
            # every centre component that is 0 (x and y of the cell on the axis and of the mirror, one of
            # them in the cells beside it) becomes -0.0: the records change, no bound does
            "neg_zero": each(lambda n, p: with_g(p, {k: NEG0 for k in range(2) if float(p["g"][k]) == 0.0})),
        }
    if kind == "box":
        a, c = R.SAME_LEAF[kind]

        def neg_zero(n, p):
            # The leaf pair's cells span x and y about 0. One gets the corner (-0.0, +0.0), the other
            # (+0.0, -0.0): the compare-select keeps the first of two equal values, so the leaf's union
            # takes a zero of each sign, whichever way round the builder ordered the two slots, and
            # fmin / fmax in its place would give -0.0 twice. The pair's sibling is cut to y >= 0.5 so
            # that the node's own union shows both zeros, and the mirror gets a far corner at -0.0.
            i = idx[n]
            if i == a:
                return with_g(p, {0: NEG0, 1: 0.0})
            if i == c:
                return with_g(p, {0: 0.0, 1: NEG0})
            if float(p["g"][0]) < 0.0 < float(p["g"][3]):
                return with_g(p, {3: NEG0})
            return with_g(p, {1: 0.5})

        return {
            # (along z for all: the mirror, the last of the set, fills the extent in x and y)
            "grow": each(lambda n, p: with_g(p, {5: float(p["g"][5]) + 1.5, 2: float(p["g"][2]) - 0.25})),
            "plate": each(lambda n, p: with_g(p, {5: float(p["g"][2])})),
            "inverted": each(lambda n, p: with_g(p, {0: float(p["g"][3]), 3: float(p["g"][0])})),
            "neg_zero": each(neg_zero),
        }
    if kind == "obb":
        return {
            "rotate": each(lambda n, p: rotated_obb(p, *ROTATIONS[n]), 0.5),
            "halves": each(lambda n, p: with_g(p, {12: 0.25, 13: 2.0, 14: 1.0}), 0.5),
            "neg_half": each(lambda n, p: with_g(p, {12 + n % 3: -0.5}), -0.5),
            # two halves of 0: a segment (with one, a ray in the plate's own plane is accepted: its slab is NaN, which min / max drop)
            "zero_half": each(lambda n, p: with_g(p, {12 + (n + 1) % 3: 0.0, 12 + (n + 2) % 3: 0.0}), -0.5),
            "turned_neg_half": each(lambda n, p: with_g(rotated_obb(p, *ROTATIONS[n]), {12 + n % 3: -1.0}), 0.5),
        }
    if kind == "tri":
        # both triangles of each quad, then the mirror
        quads = list(dict.fromkeys(j for i in idx[:-1] for j in (i - i % 2, i - i % 2 + 1)))
        m = prims[idx[-1]]
        return {
            "tilt": (np.array(quads + idx[-1:], np.uint32),
                     [_tilted(prims, i) for i in quads] + [with_g(m, {5: float(m["g"][5]) + 0.5})]),
            "degenerate": each(lambda n, p: with_g(p, {3: p["g"][0], 4: p["g"][1], 5: p["g"][2]}), -0.5),
            # v2 onto the line v0 v1, past v1
            "collinear": each(lambda n, p: with_g(p, {6 + k: 2.0 * float(p["g"][3 + k]) - float(p["g"][k]) for k in range(3)}), -0.5),
        }
    assert kind == "mixed"
    new = []
    idx = list(dict.fromkeys(idx + [i for i, _ in R.MOVES[kind]]))
    for i in idx:
        p = prims[i]
        if p["kind"] == S.AABB:
            q = with_g(p, {3: float(p["g"][3]) + 1.5, 1: float(p["g"][1]) - 0.25})
        elif p["kind"] == S.SPHERE:
            q = with_g(p, {3: 1.75})
        elif p["kind"] == S.OBB:
            q = rotated_obb(p, 0, 30.0)
        elif p["kind"] == S.TRIANGLE:
            q = _tilted(prims, i) if i in R.SAME_LEAF[kind] else with_g(p, {2: float(p["g"][2]) + 0.5})
        elif p["kind"] == S.PLANE:  # its position and its orientation (0.6, 0, -0.8 is a unit vector to a few ulps)
            q = with_g(p, {2: float(p["g"][2]) + 2.5, 3: 0.6, 4: 0.0, 5: -0.8})
        else:
            q = with_g(p, {0: 1.0, 1: 2.0, 2: 3.0, 7: -4.0})  # a stub's words, which nothing reads
        new.append(q)
    return {"all_kinds": (np.array(idx, np.uint32), new)}


def on_variant(prims, idx, new):
    """The geometry of an edit on another variant of the same lattice (tests/ray_edge_fixtures.py:
    the variants differ in materials and colours alone): (indices, prims)."""
    out = []
    for i, p in zip(idx, new):
        q = copy.deepcopy(prims[int(i)])
        assert q["kind"] == p["kind"]
        q["g"] = [float(F(x)) for x in p["g"]]
        out.append(q)
    return np.asarray(idx, np.uint32), out


def merged(*edits):
    """Edits of distinct indices as one: (indices, prims)."""
    idx = [int(i) for e in edits for i in e[0]]
    assert len(set(idx)) == len(idx)
    return np.array(idx, np.uint32), [p for e in edits for p in e[1]]


def centre_of(p):
    """A point inside primitive p (the middle of its own bounds; a plane's position), or None."""
    g = np.asarray(p["g"], np.float64)
    k = p["kind"]
    if k in (S.SPHERE, S.OBB, S.PLANE):
        return g[:3].copy()
    if k == S.AABB:
        return 0.5 * (g[:3] + g[3:6])
    if k == S.TRIANGLE:
        return (g[:3] + g[3:6] + g[6:9]) / 3.0
    return None


_DIRS = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
_SKEW = np.array([(1, 2, 3), (-3, 1, 2), (2, -3, 1), (-1, -2, -3), (3, -1, -2), (-2, 3, -1)], np.float64) / np.sqrt(14.0)


def aimed_rays(new, dist=(1.3, 2.6)):
    """(o, d) f32: for every primitive of `new` that has a centre, a ray from each of the 26
    lattice directions, at the distances of `dist` in turn, towards a point a little off its
    centre (a ray through the centre itself would run along a triangle's diagonal or a box's edge
    planes), and six rays from 2^-10 away at the centre itself: a sphere of radius 2^-20 is hit
    only from that close (farther out, r r is below half an ulp of |o - c|^2)."""
    o, d = [], []
    for p in new:
        c = centre_of(p)
        if c is None:
            continue
        for n, u in enumerate(_DIRS):
            org = (c + dist[n % len(dist)] * u).astype(F)
            tgt = (c + np.array([0.11, 0.07, 0.05]) * (1 + n % 3)).astype(F)
            o.append(org)
            d.append(tgt - org)
        for u in _SKEW:
            org = (c + 2.0 ** -10 * u).astype(F)
            o.append(org)
            d.append(c.astype(F) - org)
    return np.array(o, F).reshape(-1, 3), np.array(d, F).reshape(-1, 3)


def rays_for(fr, kind, new):
    """(o, d): the kind's batch and the aimed rays of an edit's primitives."""
    b = CF.batch(fr, kind)
    ao, ad = aimed_rays(new)
    return np.concatenate([b["o"], ao]), np.concatenate([b["d"], ad])


def cases():
    """[(kind, group, name)]: every shape and extent edit set, for parametrised tests."""
    return [(k, "shape", n) for k in KINDS for n in EFFECT[k]] + [(k, "extent", n) for k in KINDS for n in EXTENT_NAMES]


def edit_of(kind, group, name):
    return (shape_edits(kind) if group == "shape" else extent_edits(kind))[name]


# ---- the packed extent ---------------------------------------------------------------------------

EXTENT_NAMES = ("at_extent", "past_extent", "inward")


def own_reach(p):
    """The largest |coordinate| of p's own bounds, formed in float32 as bvh.cpp prim_bounds does."""
    g = np.asarray(p["g"], F)
    k = p["kind"]
    if k == S.SPHERE:
        r = np.abs(g[3])
        return float(max(np.abs(g[:3] - r).max(), np.abs(g[:3] + r).max()))
    if k == S.AABB:
        return float(np.abs(g[:6]).max())
    if k == S.TRIANGLE:
        return float(np.abs(g[:9]).max())
    assert k == S.OBB
    m = 0.0
    for c in range(3):
        e = F(F(F(np.abs(g[3 + c]) * np.abs(g[12])) + F(np.abs(g[6 + c]) * np.abs(g[13]))) + F(np.abs(g[9 + c]) * np.abs(g[14])))
        m = max(m, abs(float(F(g[c] - e))), abs(float(F(g[c] + e))))
    return m


def extent_edits(kind):
    """{"at_extent", "past_extent", "inward": (indices, prims)}: the first movable primitive put
    where its own bounds end exactly on the packed extent (y, the upper side), the same one float
    further, and the primitive that defines the extent (the last one, the mirror) moved inward."""
    prims = CF.lattice_prims(kind)
    i = R.first_movable(kind)
    p = prims[i]
    ext = F(R.EXTENT[kind])
    if p["kind"] == S.SPHERE:
        # a radius that is no dyadic fraction: c + r is rounded, to the extent
        r = F(0.3)
        cy = F(ext - r)
        while F(cy + r) < ext:
            cy = np.nextafter(cy, F(np.inf))
        while F(np.nextafter(cy, F(-np.inf)) + r) == ext:  # the lowest centre that still rounds to it
            cy = np.nextafter(cy, F(-np.inf))
        at = with_g(p, {1: cy, 3: r})
        py = cy
        while F(py + r) <= ext:
            py = np.nextafter(py, F(np.inf))
        past = with_g(p, {1: py, 3: r})
    elif p["kind"] == S.AABB:
        at = with_g(p, {1: 14.0, 4: ext})
        past = with_g(p, {1: 14.0, 4: np.nextafter(ext, F(np.inf))})
    elif p["kind"] == S.OBB:
        at = with_g(p, {1: 15.0})  # 15 + (1 * 1 + 0 + 0): exact with the lattice's 0 / +-1 frames
        py = F(15.0)
        while F(py + F(1.0)) <= ext:  # (the float after 15 still rounds to 16 with the half size added)
            py = np.nextafter(py, F(np.inf))
        past = with_g(p, {1: py})
    else:
        assert p["kind"] == S.TRIANGLE
        at = R.translated(p, (0.0, 14.0, 0.0))
        at = with_g(at, {7: ext})
        past = with_g(at, {7: np.nextafter(ext, F(np.inf))})
    last = len(prims) - 1
    m = prims[last]
    inward = with_g(m, {2: 63.0}) if m["kind"] == S.SPHERE else with_g(m, {0: -12.0, 1: -12.0, 3: 12.0, 4: 12.0})
    one = np.array([i], np.uint32)
    return {"at_extent": (one, [at]), "past_extent": (one, [past]), "inward": (np.array([last], np.uint32), [inward])}


# ---- a reach above its floor -----------------------------------------------------------------------

def origin_reach(extent, sphere_rmin):
    """bvh.h bvh_origin_reach in float32."""
    extent, rmin = F(extent), F(sphere_rmin)
    unit = F(extent + F(1.0))
    reach = F(F(CF.REACH_UNITS) * unit)
    if rmin >= 0:
        pad = F(F(F(1e-4) * extent) + F(1e-4))
        inner = F(F(F(rmin * pad) + F(F(F(0.25) * pad) * pad)) * F(F(1048576.0) / F(3.0)))
        safe = F(np.sqrt(inner, dtype=F) - extent)
        reach = min(reach, max(unit, safe))
    return float(reach)


REACH_SHELLS = (0.5, 0.97, 0.9999, 1.0001, 1.5)   # the first three inside the packed reach
REACH_DELTAS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)
REACH_SCALES = (1.0, 2.0 ** -20, 2.0 ** 20)
REACH_SEED = 0x5EAC4
REACH_EDITED = (62, 37)   # the centre sphere (0, 0, 0) and (-1.5, 0, 0): both interior
REACH_RADII = {"shrink": 2.0 ** -10, "grow": 0.74, "zero": 0.0}
REACH_ORIGINS = 3         # per edited sphere and shell


def reach_prims():
    """5 x 5 x 5 lambertian spheres of radius 0.5 at pitch 1.5 about the origin: the extent is 3.5
    and bvh_origin_reach(3.5, 0.5) is about 5.37, above its floor of extent + 1 = 4.5."""
    prims = []
    for n, (i, j, k) in enumerate((i, j, k) for i in range(5) for j in range(5) for k in range(5)):
        col = (0.25 + (n % 8) / 16.0, 0.25 + ((n // 8) % 8) / 16.0, 0.5 + (n % 3) / 8.0)
        prims.append(S.sphere((1.5 * (i - 2), 1.5 * (j - 2), 1.5 * (k - 2)), 0.5, S.LAMBERTIAN if n % 4 else S.LIGHT, col, 0.0))
    return prims


def _tangent_rays(c, r, reach, rng):
    """Rays of one sphere, shell by shell: origins on the cube |o|_inf = shell * reach, directions
    that pass the centre at r (1 + delta), formed in double and rounded, then scaled."""
    out = []
    for shell in REACH_SHELLS:
        o_s, d_s = [], []
        for _ in range(REACH_ORIGINS):
            o = rng.uniform(-1.0, 1.0, 3)
            o[rng.integers(3)] = rng.choice([-1.0, 1.0])
            o = (o * (shell * reach)).astype(F)
            # the largest component is shell * reach rounded to float32: on the side of the reach it is meant for
            big = int(np.argmax(np.abs(o)))
            want = F(shell * reach)
            if shell < 1.0:
                while want > F(reach):
                    want = np.nextafter(want, F(0))
            else:
                while want <= F(reach):
                    want = np.nextafter(want, F(np.inf))
            o[big] = np.sign(o[big]) * want
            oc = c - o.astype(np.float64)
            L = np.linalg.norm(oc)
            u = oc / L
            v = np.cross(u, rng.normal(size=3))
            v /= np.linalg.norm(v)
            for delta in REACH_DELTAS:
                s = min(1.0, r * (1.0 + delta) / L)
                dirn = np.sqrt(1.0 - s * s) * u + s * v
                for scale in REACH_SCALES:
                    o_s.append(o)
                    d_s.append((dirn * scale).astype(F))
        out.append((np.array(o_s, F), np.array(d_s, F)))
    return out


def _whole_waves(o, d):
    """Padded with copies of its first rays to a multiple of 64."""
    k = (-len(o)) % 64
    return np.concatenate([o, o[:k]]), np.concatenate([d, d[:k]])


_reach = {}


def reach_scene():
    """{"prims", "reach" (packed, float32), "edits": {name: (indices, prims)}, "rays": {name: (o, d)},
    "waves": {name: (tree waves, list waves)}}. The rays of an edit: per edited sphere and shell the
    tangent family at the edited radius; the rays of the three inner shells first, padded to whole
    waves of 64, then those of the two outer shells, padded likewise."""
    if _reach:
        return _reach
    prims = reach_prims()
    reach = origin_reach(3.5, 0.5)
    edits, rays, waves = {}, {}, {}
    for name, r in REACH_RADII.items():
        rng = np.random.default_rng(REACH_SEED)
        idx = np.array(REACH_EDITED, np.uint32)
        new = [with_g(prims[i], {3: r}) for i in REACH_EDITED]
        fam = [_tangent_rays(np.asarray(p["g"][:3], np.float64), r, reach, rng) for p in new]
        inner = [s for f in fam for s in f[:3]]
        outer = [s for f in fam for s in f[3:]]
        io, id_ = _whole_waves(np.concatenate([s[0] for s in inner]), np.concatenate([s[1] for s in inner]))
        oo, od = _whole_waves(np.concatenate([s[0] for s in outer]), np.concatenate([s[1] for s in outer]))
        edits[name] = (idx, new)
        rays[name] = (np.concatenate([io, oo]), np.concatenate([id_, od]))
        waves[name] = (len(io) // 64, len(oo) // 64)
    _reach.update(prims=prims, reach=reach, edits=edits, rays=rays, waves=waves)
    return _reach


# ---- sequences -----------------------------------------------------------------------------------

PACK, REFIT, NONE = 1, 2, 0   # FR_SCENE_SYNC_*


def _moved(cur, idx, delta):
    return np.array(idx, np.uint32), [R.translated(cur[i], delta) for i in idx]


def sequences(kind):
    """{name: {"steps": [...], "uses": [...], "final": prims, "restored": bool}}. A step is
    ("update", indices, prims), ("use",) or ("rebuild",); `uses` holds, per ("use",) step, what
    scene_info must read after it: last_sync, prims_patched, packs, refits, edit_seq. "restored":
    the final tables equal the first pack's."""
    prims = CF.lattice_prims(kind)
    a_idx, a_new = R.move_set(kind)
    a_idx = [int(i) for i in a_idx]
    a_state = R.applied(prims, a_idx, a_new)
    i0 = R.first_movable(kind)
    others = [i for i in a_idx if i != i0 and prims[i]["kind"] not in (S.PLANE, S.STUB) and i != len(prims) - 1]
    out = {}

    def use(sync, patched, packs, refits, seq):
        return {"last_sync": sync, "prims_patched": patched, "packs": packs, "refits": refits, "edit_seq": seq}

    def add(name, steps, uses, restored=False):
        cur = list(prims)
        for st in steps:
            if st[0] == "update":
                cur = R.applied(cur, st[1], st[2])
        assert sum(1 for st in steps if st[0] == "use") == len(uses)
        out[name] = {"steps": steps, "uses": uses, "final": cur, "restored": restored}

    first = [("use",)], [use(PACK, 0, 1, 0, 0)]
    # two and three updates with no use between them: one refit of the distinct stamped primitives
    # (each later update re-edits primitives of the first and brings one the first did not hold)
    extra = [i for i in range(len(prims) - 1) if i not in a_idx and prims[i]["kind"] not in (S.PLANE, S.STUB)][7::11][:2]
    b = _moved(a_state, [a_idx[0], extra[0]], (0.0, 2.0, -0.5))
    ab_state = R.applied(a_state, *b)
    c = _moved(ab_state, [others[0], extra[1], others[-1]], (0.0, -2.0, -1.0))
    n_ab = len(set(a_idx) | set(int(i) for i in b[0]))
    n_abc = len(set(a_idx) | set(int(i) for i in b[0]) | set(int(i) for i in c[0]))
    add("two_updates", first[0] + [("update", a_idx, a_new), ("update",) + b, ("use",)], first[1] + [use(REFIT, n_ab, 1, 1, 2)])
    add("three_updates", first[0] + [("update", a_idx, a_new), ("update",) + b, ("update",) + c, ("use",)],
        first[1] + [use(REFIT, n_abc, 1, 1, 3)])
    # a duplicate index in one call: the later entry wins
    p1 = R.translated(prims[i0], (0.0, -2.5, 2.5))
    p2 = R.translated(prims[i0], (0.0, 2.5, 3.0))
    q = R.translated(prims[others[0]], _move_of(kind, others[0]))
    add("duplicate", first[0] + [("update", [i0, others[0], i0], [p1, q, p2]), ("use",)], first[1] + [use(REFIT, 2, 1, 1, 1)])
    assert out["duplicate"]["final"][i0] is p2
    # an edit and its inverse before a use
    add("inverse", first[0] + [("update", a_idx, a_new), ("update", a_idx, [prims[i] for i in a_idx]), ("use",)],
        first[1] + [use(REFIT, len(a_idx), 1, 1, 2)], restored=True)
    # an update before the first use: one pack
    add("before_first_use", [("update", a_idx, a_new), ("use",)], [use(PACK, 0, 1, 0, 1)])
    # patch, colour change, patch
    col = copy.deepcopy(a_state[i0])
    col["color"] = [0.125, 0.5, 0.875]
    col_state = R.applied(a_state, [i0], [col])
    b2 = _moved(col_state, [i0, others[0]], (0.0, 2.0, -0.5))
    add("patch_colour_patch", first[0] + [("update", a_idx, a_new), ("use",), ("update", [i0], [col]), ("use",),
                                         ("update",) + b2, ("use",)],
        first[1] + [use(REFIT, len(a_idx), 1, 1, 1), use(PACK, 0, 2, 1, 1), use(REFIT, len(b2[0]), 2, 2, 2)])
    # a rebuild between two patches
    add("patch_rebuild_patch", first[0] + [("update", a_idx, a_new), ("use",), ("rebuild",), ("use",), ("update",) + b, ("use",)],
        first[1] + [use(REFIT, len(a_idx), 1, 1, 1), use(PACK, 0, 2, 1, 1), use(REFIT, len(b[0]), 2, 2, 2)])
    # past the extent (the patch is refused: a pack, with a larger extent), then an edit that is
    # outside the old extent and inside the new one (a refit)
    far = R.outside_move(kind)
    e = R.EXTENT[kind]
    between = _moved(prims, [others[0]], (0.0, 1.5 * e, 0.0))
    assert e < R.own_extent(between[1]) < R.own_extent(far[1])
    add("past_then_inside_the_new_extent", first[0] + [("update",) + far, ("use",), ("update",) + between, ("use",)],
        first[1] + [use(PACK, 0, 2, 0, 1), use(REFIT, 1, 2, 1, 2)])
    return out


def _move_of(kind, i):
    return next(d for j, d in R.MOVES[kind] if j == i)
