"""Fixtures for the edge-ray parity tests (tests/test_ray_edges.py): cameras whose rays
are exactly axis-parallel, start exactly on a surface or have no direction at all, over
scenes on a dyadic lattice.

fr_camera is a plain struct: the trace kernel and the oracle's Camera::get_ray both
evaluate lower_left + s horizontal + t vertical - position - offset on whatever the fields
hold. A camera with horizontal.x = vertical.x = 0 and lower_left.x == position.x therefore
sends every primary ray with d.x exactly zero, and one with horizontal = vertical = 0
sends the same ray for every sample of the frame. camera_new / camera_look with jittered
pixels never produce such rays.

The lattice: cell centres at even integers (odd ones in x on the shifted lattice), half
size 1, so every "exactly on" condition holds in f32. Cells touch: boxes share faces,
spheres are tangent, quads share edges. About a quarter of the cells are left empty so
that rays reach the deeper layers. A fuzz = 0 metal slab sits behind the camera (a large
fuzz = 0 metal sphere in the sphere-only scenes, which must stay of one kind), so a beam
that comes back keeps bouncing to the depth cap.

Each Fixture names the condition it is built to reach (`expect`); test_ray_edges.py checks
every condition against the oracle alone, without a GPU.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import oracle_py as O
from oracle import scene_ref as S

F = np.float32
NEG0 = F(-0.0)

KINDS = ("box", "sphere", "obb", "tri", "plane", "mixed")
SIZES = ("small", "mid", "mid_plane", "big")
# (nx, ny, nz) cells per kind and size: "small" gives <= 15 primitives, "mid" 16..47,
# "big" >= 49 cells (a quad cell is two triangles)
DIMS = {
    "small": {"tri": (2, 2, 2), None: (2, 3, 2)},
    "mid": {"tri": (2, 3, 3), None: (2, 4, 4)},
    "big": {None: (2, 6, 6)},
}
# exact 90-degree frames of the oriented boxes: identity, an axis permutation, sign flips
OBB_AXES = (
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    ((0, 1, 0), (0, 0, 1), (1, 0, 0)),
    ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    ((0, 0, 1), (-1, 0, 0), (0, -1, 0)),
)
PALETTE = ((0.75, 0.25, 0.25), (0.25, 0.75, 0.25), (0.25, 0.25, 0.75), (0.75, 0.75, 0.25), (0.5, 0.5, 0.5))


def edge_camera(fr, pos, ll, hor, ver, lens=0.0, u=(1, 0, 0), v=(0, 1, 0), w=16, h=16):
    """(FrCamera, OrCamera) filled field by field from the same float32 values; the two are
    compared as uint32, so a -0.0 survives on both sides."""
    vals = {"position": pos, "lower_left": ll, "horizontal": hor, "vertical": ver, "u": u, "v": v, "w": (0, 0, 1)}
    scal = {"aspect": F(w) / F(h), "lens_radius": lens, "focus_dist": 2.0, "radius": 5.0, "rotation": 0.0}
    cam, ocam = fr.FrCamera(), O.OrCamera()
    for c in (cam, ocam):
        for name, vec in vals.items():
            for k in range(3):
                getattr(c, name)[k] = float(F(vec[k]))
        for name, x in scal.items():
            setattr(c, name, float(F(x)))
    a, b = cam.to_array(), O.camera_to_array(ocam)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    want = np.concatenate([np.asarray(vals[n], dtype=F) for n in vals] + [np.asarray(list(scal.values()), dtype=F)])
    assert np.array_equal(a.view(np.uint32), want.view(np.uint32))
    return cam, ocam


# ---- scenes -------------------------------------------------------------------------

def _occupied(i, jj, k):
    return (i + jj + 2 * k) % 4 != 3  # cell (0, 0, 0), the one the beams and R5 aim at, is kept


def cells(kind, size, shift=0):
    """Centres of the kept cells: x in {0, 2} + shift, y about 0, z = -4, -6, ...; the cell
    at (shift, 0, -4) comes first (a lambertian box in the box and mixed scenes)."""
    table = DIMS["mid" if size == "mid_plane" else size]
    nx, ny, nz = table.get(kind, table[None])
    idx = [(i, j - ny // 2, k) for k in range(nz) for j in range(ny) for i in range(nx)]
    idx.sort(key=lambda c: c != (0, 0, 0))  # stable: the aimed-at cell first, the rest layer by layer
    return [(2.0 * i + shift, 2.0 * jj, -4.0 - 2.0 * k) for i, jj, k in idx if _occupied(i, jj, k)]


def _cell_prims(kind, n, c, mat, col, fuzz):
    cx, cy, cz = c
    if kind == "mixed":
        kind = ("box", "sphere", "obb", "tri", "plane", "stub")[n % 6]
    if kind == "box":
        return [S.prim(S.AABB, mat, col, fuzz, [cx - 1, cy - 1, cz - 1, cx + 1, cy + 1, cz + 1])]
    if kind == "sphere":
        return [S.sphere(c, 1.0, mat, col, fuzz)]
    if kind == "obb":
        ax = OBB_AXES[n % len(OBB_AXES)]
        return [S.prim(S.OBB, mat, col, fuzz, list(c) + list(ax[0]) + list(ax[1]) + list(ax[2]) + [1, 1, 1])]
    if kind == "tri":  # a quad in z = cz: two triangles sharing the diagonal v00-v11
        v00, v10, v11, v01 = (cx - 1, cy - 1, cz), (cx + 1, cy - 1, cz), (cx + 1, cy + 1, cz), (cx - 1, cy + 1, cz)
        return [S.prim(S.TRIANGLE, mat, col, fuzz, v00 + v10 + v11), S.prim(S.TRIANGLE, mat, col, fuzz, v11 + v01 + v00)]
    if kind == "plane":  # a tile facing +z (plane.rs: normal = -orientation)
        return [S.plane(c, (0, 0, -1), (1, 1, 1), mat, col, fuzz)]
    return [S.prim(S.STUB, mat, col, fuzz)]


def lattice(kind, size, shift=0, variant="full"):
    """The scene of one kind ("mixed": every kind and stubs in turn) as oracle primitive
    dicts. variant "full": lambertian, fuzz = 0 metal, glass and light in turn; "diffuse":
    no metal or glass (the diffuse-only shading step); "classes": diffuse with five colours
    (the BVH kernels' attenuation-class records)."""
    prims = []
    for n, c in enumerate(cells(kind, size, shift)):
        mat = n % 4
        col = (0.25 + (n % 8) / 16.0, 0.25 + ((n // 8) % 8) / 16.0, 0.5 + (n % 3) / 8.0)
        if variant != "full" and mat in (S.METAL, S.DIELECTRIC):
            mat = S.LAMBERTIAN if mat == S.METAL else S.LIGHT
        if variant == "classes":
            col = PALETTE[n % len(PALETTE)]
        prims += _cell_prims(kind, n, c, mat, col, 0.0)
    if size == "mid_plane":
        # A backdrop behind every layer: the kernels with the plane's stale records. Listed first:
        # Plane::hit gates on its denominator, not on t (plane.rs:26), so a plane listed after a
        # nearer winner replaces it.
        prims.insert(0, S.plane((0, 0, -16), (0, 0, -1), (16, 16, 1), S.LAMBERTIAN, PALETTE[4], 0.0))
    mirror = S.LAMBERTIAN if variant != "full" else S.METAL
    if kind == "sphere":
        prims.append(S.sphere((shift, 0.0, 66.0), 64.0, mirror, PALETTE[4], 0.0))  # surface at z = 2 on the axis
    else:
        prims.append(S.prim(S.AABB, mirror, PALETTE[4], 0.0, [-16, -16, 2, 16, 16, 4]))
    return prims


def bvh_cost(prims):
    """bvh.cpp's weighted test cost (the BVH is used at >= 48, with >= 48 primitives)."""
    w = {S.TRIANGLE: 2.5, S.OBB: 2.0, S.STUB: 0.0}
    return sum(w.get(p["kind"], 1.0) for p in prims)


def first_of(prims, kind):
    """The first primitive of a kind, a lambertian or light one if there is any (an origin
    inside a metal sphere only ever absorbs)."""
    own = [p for p in prims if p["kind"] == kind]
    return next((p for p in own if p["material"] in (S.LAMBERTIAN, S.LIGHT)), own[0] if own else None)


# ---- ray families ---------------------------------------------------------------------

# name: the family; shift: the lattice's x shift; cam: edge_camera's arguments; expect: the
# condition the fixture must reach in the oracle ("hit_mostly", "must_miss", "nan_all",
# "scatters", "absorbed" or None); varied: at least half the oracle's pixels have distinct colours
Fixture = namedtuple("Fixture", "name shift cam expect varied")


def _fan_x(x, zero=0.0, lens=0.0, y0=-0.75, z0=0.0):
    """A fan inside the plane of constant x: d = (zero, -0.5 + s, -1 - 0.5 t)."""
    cam = dict(pos=(x, y0, z0), ll=(x if x != 0.0 else zero, y0 - 0.5, z0 - 1.0), hor=(zero, 1.0, 0),
               ver=(zero, 0, -0.5), lens=lens)
    if lens:  # the lens disk inside the same plane
        cam.update(u=(0, 1, 0), v=(0, 0, 1))
    return cam


def _fan_y(x0, y, z0):
    """A fan inside the plane of constant y: d = (-0.4 + 0.8 s, 0, -1 - 0.5 t)."""
    return dict(pos=(x0, y, z0), ll=(x0 - 0.4, y, z0 - 1.0), hor=(0.8, 0, 0), ver=(0, 0, -0.5))


def _beam(x, y, z=0.0):
    return dict(pos=(x, y, z), ll=(x, y, z - 1.0), hor=(0, 0, 0), ver=(0, 0, 0))


def _still(p):
    return dict(pos=p, ll=p, hor=(0, 0, 0), ver=(0, 0, 0))


def _cone(p, zlo=-1.0, zspan=0.0):
    """An ordinary cone of directions from p: d = (-1 + 2 s, -1 + 2 t, zlo + zspan t)."""
    return dict(pos=p, ll=(p[0] - 1.0, p[1] - 1.0, p[2] + zlo), hor=(2, 0, 0), ver=(0, 2, zspan))


def families(kind):
    """Every fixture of a scene kind. The conditions follow from the geometry: a ray inside
    a box's face plane grazes it (hit for d_k = +0), an oriented box gives
    0 inf = NaN there and misses, a plane tile's rim is strict, a sphere is only touched."""
    solid = kind in ("box", "tri")
    fx = [
        Fixture("R0_control", 0, dict(pos=(0.37, -0.79, 0.13), ll=(0.04, -1.29, -0.87), hor=(0.8, 0.05, 0),
                                      ver=(0.03, 1.0, 0), lens=0.05), "hit_mostly" if solid else None, True),
        Fixture("R1_face", 0, _fan_x(1.0), {"box": "hit_mostly", "tri": "hit_mostly", "obb": "must_miss",
                                            "plane": "must_miss", "sphere": "must_miss"}.get(kind), True),
        Fixture("R1_mid", 0, _fan_x(0.0), "hit_mostly" if kind == "sphere" else None, True),
        # the same in the face plane y = -1 (d.y = +0: a constant sky, so only hits vary the image;
        # rays passing within rounding of a sphere's touching point may see a tiny disc > 0)
        Fixture("R1_face_y", 0, _fan_y(1.25, -1.0, 0.0), {"box": "hit_mostly", "tri": "hit_mostly", "obb": "must_miss",
                                                         "plane": "must_miss"}.get(kind), False),
        # faces and the scene kernel's compile-time-zero slab coordinates in x = 0; the zero's
        # sign in lower_left / horizontal / vertical decides the sign of d.x
        Fixture("R2_neg0", -1, _fan_x(0.0, zero=NEG0), None, True),
        Fixture("R2_pos0", -1, _fan_x(0.0), None, True),
        Fixture("R3_centre", 0, _beam(0.0, 0.0), None, False),
        Fixture("R3_edge", 0, _beam(1.0, -1.0), None, False),  # along the edge four cells share
        # inside the face two cells share, through the point where two spheres touch (disc == 0)
        Fixture("R3_face", 0, _beam(1.0, 0.0), "must_miss" if kind == "sphere" else None, False),
        Fixture("R4_lens", 0, _fan_x(1.0, lens=0.5), "hit_mostly" if solid else None, True),
        # d = 0: unit(d) is NaN in the sky; z = 5 is past every box's far side, so no box is "hit"
        Fixture("R5_sky", 0, _still((0.25, 0.5, 5.0)), "nan_all", False),
    ]
    if kind != "sphere":  # d = 0 in front of the mirror slab: entered at t = 1.5 * 2^100, p == o, absorbed
        fx.append(Fixture("R5_front", 0, _still((0.25, 0.5, 0.5)), "absorbed", False))
    if kind in ("box", "mixed"):  # cell (0, 0, -4) is a lambertian box in both
        fx.append(Fixture("R5_inbox", 0, _still((0.25, 0.5, -4.25)), "scatters", False))
    scene = lattice(kind, "small")
    sph, tri, pl = first_of(scene, S.SPHERE), first_of(scene, S.TRIANGLE), first_of(scene, S.PLANE)
    if sph is not None:
        c = [float(x) for x in sph["g"][:3]]
        fx.append(Fixture("R3_sphere", 0, _beam(c[0], c[1]), None, False))  # through the sphere's centre
        fx.append(Fixture("R6_sphere_centre", 0, _cone(c), None, True))
        # from the pole z = c.z + 1: inward, tangent (d.z = 0) and just outward
        fx.append(Fixture("R6_sphere_surface", 0, _cone((c[0], c[1], c[2] + 1.0), zspan=1.0), None, True))
    if tri is not None:
        v0, v1 = [float(x) for x in tri["g"][0:3]], [float(x) for x in tri["g"][3:6]]
        fx.append(Fixture("R6_tri_vertex_origin", 0, _cone(tuple(v1)), None, True))
        mid = tuple(0.5 * (a + b) for a, b in zip(v0, v1))
        fx.append(Fixture("R6_tri_edge_origin", 0, _cone(mid), None, True))
    if pl is not None:
        p = [float(x) for x in pl["g"][:3]]
        fx.append(Fixture("R6_plane_rim", 0, _fan_y(p[0] + 0.25, p[1] + 1.0, p[2] + 3.0), "must_miss" if kind == "plane" else None, False))
    return fx


def fixture(kind, name):
    return next(f for f in families(kind) if f.name == name)


# ---- frames and the shared oracle reference ---------------------------------------------

W, H, SPP, SEED = 16, 16, 4, 5  # four waves of items; the oracle renders a frame in milliseconds
_reference = {}


def cameras(fr, fx):
    return edge_camera(fr, w=W, h=H, **fx.cam)


def reference(fr, kind, size, variant, name, depth):
    """(prims, mean, u8, counters) of the oracle's render of one fixture, computed once and
    shared (read-only) by every test that compares against it."""
    key = (kind, size, variant, name, depth)
    if key not in _reference:
        fx = fixture(kind, name)
        prims = lattice(kind, size, fx.shift, variant)
        mean, u8, cnt, _ = O.render(prims, cameras(fr, fx)[1], W, H, SPP, depth, seed=SEED)
        mean.setflags(write=False)
        u8.setflags(write=False)
        _reference[key] = (prims, mean, u8, cnt)
    return _reference[key]


def cases():
    """(kind, size, family name): every family on the small scenes (the 8-B-record
    kernels), the families with the most special cases on the larger ones."""
    often = ("R0_control", "R1_face", "R1_face_y", "R2_neg0", "R3_edge", "R3_face", "R4_lens", "R5_inbox", "R5_sky", "R6_sphere_surface",
             "R6_tri_edge_origin", "R6_plane_rim")
    out = []
    for kind in KINDS:
        for size in SIZES:
            for fx in families(kind):
                if size == "small" or fx.name in often:
                    out.append((kind, size, fx.name))
    return out
