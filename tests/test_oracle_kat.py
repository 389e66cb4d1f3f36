"""Pin the oracle (oracle/oracle.cpp) before trusting it.

1. The reference's own Vec3 known-answer tests, cpu_ray_tracer/primitives.rs:159-255
   (never compiled upstream; values verified to hold in IEEE f32).
2. Analytic known answers for utility.rs (reflect/refract/schlick), the shapes'
   hit() root cases (sphere.rs:23-51, plane.rs:24-44) and the build's box.
3. RNG vectors: splitmix64 (seed 0, published) and xoshiro128+ (state 1,2,3,4),
   checked against a pure-Python restatement of both.
"""
import math

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S

f32 = np.float32


# ---- 1. primitives.rs:159-255 -------------------------------------------------

def test_length():  # :163-168
    a = (2.0, -3.0, -1.2)
    assert O.vec3(0, a)[0] == f32(14.440001)
    assert O.vec3(1, a)[0] == f32(3.8)


def test_dot():  # :170-179
    a, b = (1.0, 1.0, 1.0), (2.0, -3.0, -0.2)
    assert O.vec3(2, a, a)[0] == f32(3.0)
    assert O.vec3(2, b, b)[0] == f32(13.04)
    assert O.vec3(2, a, b)[0] == f32(-1.2)
    assert O.vec3(2, b, a)[0] == f32(-1.2)
    assert O.vec3(2, a, b)[0] == O.vec3(2, b, a)[0]


def test_cross():  # :181-189
    a, b = (1.0, 2.0, 3.0), (-3.0, -2.0, 1.0)
    assert O.vec3(3, a, a)[0] == 0.0
    assert O.vec3(3, b, b)[1] == 0.0
    assert O.vec3(3, a, b)[0] == 8.0
    assert O.vec3(3, b, a)[2] == -4.0


def test_addition():  # :191-204
    a, b = (1.0, 2.0, 3.0), (-3.0, -2.0, 1.0)
    assert list(O.vec3(4, a, b)) == [-2.0, 0.0, 4.0]
    assert list(O.vec3(4, a, b)) == list(O.vec3(4, b, a))


def test_subtraction():  # :206-219
    a, b = (1.0, 2.0, 3.0), (-3.0, -2.0, 1.0)
    assert list(O.vec3(5, a, b)) == [4.0, 4.0, 2.0]
    assert list(O.vec3(5, a, b)) == list(O.vec3(6, O.vec3(5, b, a), (-1.0, 0, 0)))


def test_multiplication():  # :221-241
    a, b = (1.0, 2.0, 3.0), (-3.0, -2.0, 1.0)
    assert list(O.vec3(6, a, (3.0, 0, 0))) == [3.0, 6.0, 9.0]
    assert list(O.vec3(7, a, b)) == [-3.0, -4.0, 3.0]


def test_division():  # :243-254
    assert list(O.vec3(8, (1.0, 2.0, 3.0), (2.0, 0, 0))) == [0.5, 1.0, 1.5]


# ---- 2. analytic known answers -------------------------------------------------

def test_unit_vector_and_reflect():
    u = O.vec3(9, (3.0, 0.0, 4.0))
    assert list(u) == [f32(0.6), 0.0, f32(0.8)]
    # reflect off the floor flips y only: v - 2*dot(v,n)*n
    assert list(O.vec3(10, (1.0, -1.0, 0.5), (0.0, 1.0, 0.0))) == [1.0, 1.0, 0.5]


def test_refract_normal_incidence_and_tir():
    ok, r = O.refract((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), 1.0 / 1.3)
    assert ok and list(r) == [0.0, -1.0, 0.0]  # straight through
    ok, _ = O.refract((1.0, -0.05, 0.0), (0.0, 1.0, 0.0), 1.3)  # grazing, n1 > n2: total internal reflection
    assert not ok


def test_schlick_closed_form():
    r0 = ((1 - 1.3) / (1 + 1.3)) ** 2
    for c in (0.0, 0.25, 0.5, 1.0):
        want = r0 + (1 - r0) * (1 - c) ** 5
        assert abs(O.vec3(12, (c, 1.3, 0))[0] - want) < 2e-7
    assert O.vec3(12, (1.0, 1.3, 0))[0] == f32(f32(1 - f32(1.3)) / f32(1 + f32(1.3))) ** 2


def _sphere(c, r):
    return S.sphere(c, r, 0, (0.5, 0.5, 0.5), 0.0)


def test_sphere_outside_hit_near_root():
    best, rec = O.closest_hit([_sphere((0.0, 0.0, -5.0), 1.0)], (0, 0, 0), (0, 0, -1))
    assert best == 0 and rec[0] == 4.0 and list(rec[1:4]) == [0.0, 0.0, -4.0] and list(rec[4:]) == [0, 0, 1.0]


def test_sphere_inside_takes_far_root_with_outward_normal():
    best, rec = O.closest_hit([_sphere((0.0, 0.0, 0.0), 2.0)], (0, 0, 0), (0, 0, -1))
    assert best == 0 and rec[0] == 2.0 and list(rec[4:]) == [0, 0, -1.0]  # never flipped (sphere.rs:35,44)


def test_sphere_tangent_is_a_miss():
    best, _ = O.closest_hit([_sphere((1.0, 0.0, -5.0), 1.0)], (0, 0, 0), (0, 0, -1))
    assert best == -1  # discriminant > 0 is strict (sphere.rs:30)


def test_closest_wins_and_exact_ties_keep_the_first():
    a, b = _sphere((0, 0, -5.0), 1.0), _sphere((0, 0, -10.0), 1.0)
    assert O.closest_hit([b, a], (0, 0, 0), (0, 0, -1))[0] == 1
    assert O.closest_hit([a, a], (0, 0, 0), (0, 0, -1))[0] == 0  # t < t_max strict


def test_plane_gates_on_denominator_and_allows_negative_t():
    # plane.rs:26: `denom > t_min && denom < t_max` with denom = dot(orientation, d)
    p = S.plane((0.0, 0.0, -1.0), (0.0, 0.0, -1.0), (5.0, 5.0, 5.0), 0, (1, 1, 1), 0.0)
    best, rec = O.closest_hit([p], (0, 0, 0), (0, 0, -1))
    assert best == 0 and rec[0] == 1.0 and list(rec[4:]) == [0.0, 0.0, 1.0]
    best, rec = O.closest_hit([p], (0, 0, -2.0), (0, 0, -1))  # plane behind the origin: t = -1 accepted
    assert best == 0 and rec[0] == -1.0


def test_plane_failed_bounds_leave_stale_t_and_p():
    s = _sphere((0.0, 0.0, -5.0), 1.0)
    p = S.plane((0.0, 0.0, -2.0), (0.0, 0.0, -1.0), (0.1, 0.1, 0.1), 0, (1, 1, 1), 0.0)  # tiny plane
    best, rec = O.closest_hit([s, p], (0.5, 0.0, 0.0), (0, 0, -1))
    # the sphere wins, but the plane overwrote t and p before failing its bounds (plane.rs:28-29)
    assert best == 0 and rec[0] == 2.0 and list(rec[1:4]) == [0.5, 0.0, -2.0]
    assert rec[4] > 0  # normal is still the sphere's


def test_box_entry_exit_and_outward_normals():
    box = S.prim(S.AABB, 0, (1, 1, 1), 0.0, [-1, -1, -6, 1, 1, -4])
    best, rec = O.closest_hit([box], (0, 0, 0), (0, 0, -1))
    assert best == 0 and rec[0] == 4.0 and list(rec[4:]) == [0.0, 0.0, 1.0]
    best, rec = O.closest_hit([box], (0, 0, -5.0), (0, 0, -1))  # inside: exit face
    assert best == 0 and rec[0] == 1.0 and list(rec[4:]) == [0.0, 0.0, -1.0]
    assert O.closest_hit([box], (0, 2.0, 0), (0, 0, -1))[0] == -1


def test_obb_matches_aabb_for_identity_axes():
    obb = S.prim(S.OBB, 0, (1, 1, 1), 0.0, [0, 0, -5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1])
    best, rec = O.closest_hit([obb], (0.25, 0.5, 0), (0, 0, -1))
    assert best == 0 and rec[0] == 4.0 and list(rec[4:]) == [0.0, 0.0, 1.0]


def _tri(v0, v1, v2, material=0):
    return S.prim(S.TRIANGLE, material, (1, 1, 1), 0.0, list(v0) + list(v1) + list(v2))


def test_triangle_hit_barycentric_bounds_and_facing_normal():
    # triangle in z = -4; counter-clockwise seen from +z, so the winding normal is +z
    t = _tri((-1.0, -1.0, -4.0), (1.0, -1.0, -4.0), (0.0, 1.0, -4.0))
    best, rec = O.closest_hit([t], (0, 0, 0), (0, 0, -1))
    assert best == 0 and rec[0] == 4.0 and list(rec[1:4]) == [0.0, 0.0, -4.0] and list(rec[4:]) == [0, 0, 1.0]
    # from behind: the normal still faces the ray (double-faced meshes)
    best, rec = O.closest_hit([t], (0, 0, -8.0), (0, 0, 1))
    assert best == 0 and rec[0] == 4.0 and list(rec[4:]) == [0, 0, -1.0]
    # dielectric keeps the winding normal (inside/outside for refraction)
    best, rec = O.closest_hit([_tri((-1.0, -1.0, -4.0), (1.0, -1.0, -4.0), (0.0, 1.0, -4.0), 2)], (0, 0, -8.0), (0, 0, 1))
    assert best == 0 and list(rec[4:]) == [0, 0, 1.0]
    # outside the edges, behind t_min, and parallel rays miss
    assert O.closest_hit([t], (1.5, 0, 0), (0, 0, -1))[0] == -1
    assert O.closest_hit([t], (0, 0, -4.0005), (0, 0, 1))[0] == -1      # t = 0.0005 < t_min 0.001
    assert O.closest_hit([t], (0, 0, 0), (1, 0, 0))[0] == -1            # det = 0
    # a vertex and an edge point are inside (u, v >= 0, u + v <= 1 are closed)
    assert O.closest_hit([t], (-1.0, -1.0, 0), (0, 0, -1))[0] == 0
    assert O.closest_hit([t], (0.0, -1.0, 0), (0, 0, -1))[0] == 0


def test_triangle_list_order_and_ties():
    a = _tri((-1.0, -1.0, -4.0), (1.0, -1.0, -4.0), (0.0, 1.0, -4.0))
    b = _tri((-1.0, -1.0, -6.0), (1.0, -1.0, -6.0), (0.0, 1.0, -6.0))
    assert O.closest_hit([b, a], (0, 0, 0), (0, 0, -1))[0] == 1
    assert O.closest_hit([a, a], (0, 0, 0), (0, 0, -1))[0] == 0


# ---- edge rays: exact zeros and on-surface origins -------------------
# The single-ray definitions behind tests/test_ray_edges.py, on the lattice its scenes use.

def _box(lo, hi):
    return S.prim(S.AABB, 0, (1, 1, 1), 0.0, list(lo) + list(hi))


P100 = f32(2.0) ** 100  # the clamp of the box's reciprocal direction


def test_box_face_grazing_ray_hits_only_with_the_zero_pointing_inward():
    """An origin in a face plane with d_k = 0: inv_k = +-2^100, so the face's own distance is
    fma(c, inv, -c inv) = 0 and the other face's +-2^101. The x slab is [0, 2^101] when the
    zero points into the box (+0 in the low face, -0 in the high face) and [-2^101, 0]
    otherwise, which leaves tf = 0: a miss. The hit enters through z: normal axis z, sign +."""
    left, right = _box((-1, -1, -6), (1, 1, -4)), _box((1, -1, -6), (3, 1, -4))
    for box, plane_x, inward in ((left, -1.0, 0.0), (left, 1.0, -0.0), (right, 1.0, 0.0), (right, 3.0, -0.0)):
        best, rec = O.closest_hit([box], (plane_x, 0.5, 0), (inward, 0, -1))
        assert best == 0 and rec[0] == 4.0 and list(rec[1:4]) == [plane_x, 0.5, -4.0] and list(rec[4:]) == [0, 0, 1.0]
        assert O.closest_hit([box], (plane_x, 0.5, 0), (-inward, 0, -1))[0] == -1
    # in the plane two boxes share, +0 takes the box on the high side and -0 the one on the low side
    assert O.closest_hit([left, right], (1.0, 0.5, 0), (0.0, 0, -1))[0] == 1
    assert O.closest_hit([left, right], (1.0, 0.5, 0), (-0.0, 0, -1))[0] == 0


def test_box_origin_on_a_shared_face_takes_the_neighbours_far_root():
    a, b = _box((-1, -1, -1), (1, 1, 1)), _box((1, -1, -1), (3, 1, 1))
    best, rec = O.closest_hit([a, b], (1.0, 0, 0), (1, 0, 0))
    # a: slab [-2, 0], no root above t_min; b: tn = 0 is not above t_min either, so its far root
    assert best == 1 and rec[0] == 2.0 and list(rec[1:4]) == [3.0, 0, 0] and list(rec[4:]) == [1.0, 0, 0]
    best, rec = O.closest_hit([a, b], (1.0, 0, 0), (-1, 0, 0))
    assert best == 0 and rec[0] == 2.0 and list(rec[4:]) == [-1.0, 0, 0]


def test_box_zero_direction_exits_at_2_pow_100_with_sign_zero_negative():
    """d = 0 inside a box: every far distance is 2^100 (hi - o) for +0 and 2^100 (o - lo) for
    -0; the least one wins, p == o, and the exit normal +sign(d_k) counts sign(0) as negative:
    -1 on the winning axis, whichever face that is."""
    box = _box((-1, -1, -5), (1, 1, -3))
    o = (0.25, 0.5, -4.25)
    best, rec = O.closest_hit([box], o, (0.0, 0.0, 0.0))
    assert best == 0 and rec[0] == f32(0.5) * P100 and list(rec[1:4]) == list(o) and list(rec[4:]) == [0, -1.0, 0]
    best, rec = O.closest_hit([box], o, (-0.0, -0.0, -0.0))
    assert best == 0 and rec[0] == f32(0.75) * P100 and list(rec[1:4]) == list(o) and list(rec[4:]) == [0, 0, -1.0]
    # outside, just below the low z face: entered at 2^100 (lo - o), entry normal -sign(0) = +1;
    # further below than the x and y exits are away, or above the high face: no root
    best, rec = O.closest_hit([box], (0.0, 0.0, -5.25), (0.0, 0.0, 0.0))
    assert best == 0 and rec[0] == f32(0.25) * P100 and list(rec[4:]) == [0, 0, 1.0]
    assert O.closest_hit([box], (0.25, 0.5, -6.5), (0.0, 0.0, 0.0))[0] == -1
    assert O.closest_hit([box], (0.25, 0.5, 0.0), (0.0, 0.0, 0.0))[0] == -1


def test_obb_face_grazing_ray_misses():
    """The oriented box keeps (lo - o) * (1 / d): in a face plane that is 0 * inf = NaN, which
    minNum / maxNum ignore, leaving near = far = +-inf on that axis: a miss for either zero."""
    obb = S.prim(S.OBB, 0, (1, 1, 1), 0.0, [0, 0, -5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1])
    for x in (-1.0, 1.0):
        for z in (0.0, -0.0):
            assert O.closest_hit([obb], (x, 0.5, 0), (z, 0, -1))[0] == -1
    assert O.closest_hit([obb], (0.5, 0.5, 0), (0.0, 0, -1))[0] == 0  # d_k = 0 off the face planes hits
    assert O.closest_hit([obb], (0.25, 0.5, -5.25), (0.0, 0.0, 0.0))[0] == -1  # d = 0: tf = inf is no root


def _quad(cx, cy, cz):
    v00, v10, v11, v01 = (cx - 1, cy - 1, cz), (cx + 1, cy - 1, cz), (cx + 1, cy + 1, cz), (cx - 1, cy + 1, cz)
    return [_tri(v00, v10, v11), _tri(v11, v01, v00)]


def test_triangle_edges_are_inclusive_and_the_first_listed_wins():
    q = _quad(0.0, 0.0, -4.0)
    # on the shared diagonal u == 0 in both triangles: both hit at t = 4, the first listed wins
    for order in (q, q[::-1]):
        best, rec = O.closest_hit(order, (0.5, 0.5, 0), (0, 0, -1))
        assert best == 0 and rec[0] == 4.0
    assert O.closest_hit([q[1]], (0.5, 0.5, 0), (0, 0, -1))[0] == 0
    # the edge x = 1 is v1-v2 (u + v == 1) of the first triangle here and of the neighbour's second
    r = _quad(2.0, 0.0, -4.0)
    assert O.closest_hit([q[0]], (1.0, 0.5, 0), (0, 0, -1))[0] == 0
    assert O.closest_hit([r[1]], (1.0, 0.5, 0), (0, 0, -1))[0] == 0
    assert O.closest_hit(q + r, (1.0, 0.5, 0), (0.0, 0, -1))[0] == 0
    assert O.closest_hit(r + q, (1.0, 0.5, 0), (-0.0, 0, -1))[0] == 1  # r[0] does not hold the edge
    # an origin on a vertex or an edge: t = 0 is below t_min; det == 0 (d in the plane, d = 0): NaN fails
    assert O.closest_hit(q, (1.0, 1.0, -4.0), (0.25, 0.5, -1))[0] == -1
    assert O.closest_hit(q, (0.0, -1.0, -4.0), (1, 0, 0))[0] == -1
    assert O.closest_hit(q, (0.25, 0.5, 0), (0.0, 0.0, 0.0))[0] == -1


def test_plane_rim_misses_and_leaves_a_stale_t():
    tile = S.plane((0.0, 0.0, -4.0), (0.0, 0.0, -1.0), (1.0, 1.0, 1.0), 0, (1, 1, 1), 0.0)
    best, rec = O.closest_hit([tile], (1.0, 0.5, 0), (0, 0, -1))  # p.x == position.x + size.x: strict
    assert best == -1 and rec[0] == 4.0 and list(rec[1:4]) == [1.0, 0.5, -4.0]
    assert O.closest_hit([tile], (0.5, -1.0, 0), (0, 0, -1))[0] == -1
    assert O.closest_hit([tile], (0.5, 0.5, 0), (0.0, -0.0, -1))[0] == 0
    assert O.closest_hit([tile], (0.5, 0.5, 0), (0.0, 0.0, 0.0))[0] == -1  # denom = 0 is not above t_min


def test_plane_listed_after_a_nearer_winner_replaces_it():
    """plane.rs:26 gates on t_min < dot(orientation, d) < closest, not on t: a plane behind
    the winner still wins when its denominator is below the winner's t."""
    box = _box((-1, -1, -5), (1, 1, -3))
    back = S.plane((0.0, 0.0, -16.0), (0.0, 0.0, -1.0), (16.0, 16.0, 1.0), 0, (1, 1, 1), 0.0)
    best, rec = O.closest_hit([box, back], (0.5, 0.5, 0), (0, 0, -1))
    assert best == 1 and rec[0] == 16.0
    best, rec = O.closest_hit([back, box], (0.5, 0.5, 0), (0, 0, -1))
    assert best == 1 and rec[0] == 3.0


def test_sphere_zero_discriminant_and_zero_direction_miss():
    a, b = _sphere((0.0, 0.0, -4.0), 1.0), _sphere((2.0, 0.0, -4.0), 1.0)
    # through the point where the two spheres touch: disc == 0 for both (strict, sphere.rs:30)
    assert O.closest_hit([a, b], (1.0, 0.0, 0), (0.0, 0, -1))[0] == -1
    assert O.closest_hit([a, b], (1.0, 0.0, 0), (-0.0, 0.5, -1))[0] == -1
    # a == 0: disc = b b - 0 c = 0, from the centre, the surface and outside
    for o in ((0.0, 0.0, -4.0), (0.0, 0.0, -3.0), (0.25, 0.5, 0.0)):
        assert O.closest_hit([a], o, (0.0, 0.0, 0.0))[0] == -1
    # from the centre both roots are +-r / |d|: the far one, outward normal
    best, rec = O.closest_hit([a], (0.0, 0.0, -4.0), (0.0, 0, -2))
    assert best == 0 and rec[0] == 0.5 and list(rec[4:]) == [0, 0, -1.0]
    # from the pole, tangent: b == 0 and c == 0, disc == 0; inward: the far root
    assert O.closest_hit([a], (0.0, 0.0, -3.0), (1, 0, 0.0))[0] == -1
    best, rec = O.closest_hit([a], (0.0, 0.0, -3.0), (0.0, 0, -1))
    assert best == 0 and rec[0] == 2.0


def test_camera_new_basis():
    # camera.rs:24-60 at 2:1 aspect: w = +z, u = +x, v = +y, tan(30deg) half height
    c = O.camera_to_array(O.camera_new(200, 100))
    hh = f32(math.tan(f32(f32(60.0) * f32(3.14159265359) / f32(180.0)) / 2))
    # aspect, lens_radius = aperture/2, focus_dist stored 2.0, radius 5, rotation 0 (camera.rs:52-59)
    assert list(c[21:26]) == [2.0, f32(0.05), 2.0, 5.0, 0.0]
    assert list(c[12:15]) == [1.0, 0.0, 0.0] and list(c[18:21]) == [0.0, 0.0, 1.0]
    assert abs(c[10] - 2 * hh) < 1e-6  # vertical.y


# ---- 3. RNG vectors ---------------------------------------------------------------

M64 = (1 << 64) - 1


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return x, z ^ (z >> 31)


def _rotl(v, k):
    return ((v << k) | (v >> (32 - k))) & 0xFFFFFFFF


def _xoshiro(s, n):
    s = list(s)
    out = []
    for _ in range(n):
        out.append((s[0] + s[3]) & 0xFFFFFFFF)
        t = (s[1] << 9) & 0xFFFFFFFF
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 11)
    return out


def test_published_vectors():
    assert _splitmix(0)[1] == 0xE220A8397B1DCDAF  # splitmix64, seed 0, first output
    # xoshiro128+ from state (1,2,3,4): s0 + s3 = 5, then state (7, 0, 1026, 12288) -> 12295, ...
    assert _xoshiro([1, 2, 3, 4], 2) == [5, 12295]


@pytest.mark.parametrize("seed,pixel,sample", [(0x5EED, 0, 0), (0x5EED, 2073599, 255), (7, 12345, 3), (0, 0, 0)])
def test_oracle_rng_matches_restatement(seed, pixel, sample):
    x = seed ^ ((pixel << 32) | sample)
    x, a = _splitmix(x)
    x, b = _splitmix(x)
    want = _xoshiro([a & 0xFFFFFFFF, a >> 32, b & 0xFFFFFFFF, b >> 32], 64)
    assert list(O.rng_stream(seed, pixel, sample, 64)) == want


# ---- magnitude edges: tiny, huge and denormal directions ----------------
# The single-ray definitions behind tests/test_magnitude.py.

def _p2(k):
    return f32(np.ldexp(1.0, k))


def test_box_tiny_direction_component_uses_the_clamped_reciprocal():
    """d_k = 2^-110 has 1 / d_k = 2^110, clamped to 2^100: the slab distances of that axis are
    2^100 (c - o), not 2^110 (c - o). Seen from x = 1.5 with d = (-2^-110, 0, -2^-100) the box's
    x slab is [0.5, 2.5] 2^100 and its z slab [1, 3] 2^100: entered through z at t = 2^100. With
    the unclamped reciprocal the x slab would start at 0.5 * 2^110: a miss."""
    box = _box((-1, -4, -3), (1, 4, -1))
    best, rec = O.closest_hit([box], (1.5, 0, 0), (-_p2(-110), 0.0, -_p2(-100)))
    assert best == 0 and rec[0] == P100 and list(rec[4:]) == [0, 0, 1.0]
    assert list(rec[1:4]) == [f32(1.5) - _p2(-10), 0.0, -1.0]  # p = o + t d with the true d
    # at unit scale the tiny component only decides which side of a face plane the ray is on
    unit = _box((-1, -1, -6), (1, 1, -4))
    assert O.closest_hit([unit], (0.0, 0.5, 0), (_p2(-110), 0, -1))[1][0] == 4.0
    assert O.closest_hit([unit], (1.0, 0.5, 0), (-_p2(-110), 0, -1))[0] == 0   # in the face plane, inward
    assert O.closest_hit([unit], (1.0, 0.5, 0), (_p2(-110), 0, -1))[0] == -1   # outward: slab [-2^101, 0]


def test_box_denormal_direction_component_is_clamped_like_a_zero():
    """1 / 2^-149 overflows to inf and is clamped to 2^100 with its sign, as 1 / +-0 is."""
    unit = _box((-1, -1, -6), (1, 1, -4))
    for tiny in (_p2(-149), _p2(-127)):
        best, rec = O.closest_hit([unit], (-1.0, 0.5, 0), (tiny, 0, -1))
        assert best == 0 and rec[0] == 4.0 and list(rec[4:]) == [0, 0, 1.0]
        assert O.closest_hit([unit], (-1.0, 0.5, 0), (-tiny, 0, -1))[0] == -1
    obb = S.prim(S.OBB, 0, (1, 1, 1), 0.0, [0, 0, -5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1])
    # the oriented box keeps 1 / d: inf off a face plane is a slab of [-inf, inf], a hit
    assert O.closest_hit([obb], (0.5, 0.5, 0), (_p2(-149), 0, -1))[0] == 0
    assert O.closest_hit([obb], (1.0, 0.5, 0), (-_p2(-149), 0, -1))[0] == -1  # 0 inf = NaN in the face plane


def test_sphere_with_a_underflowing_to_zero_misses():
    """d = (0, 0, -2^-75): a = 2^-150 rounds to 0 while b b = 25 * 2^-150 rounds to 12 * 2^-149, so
    disc > 0 and both roots are a positive numerator over 0 = +inf, which is not below t_max."""
    s = _sphere((0.0, 0.0, -5.0), 1.0)
    assert O.vec3(2, (0, 0, -_p2(-75)), (0, 0, -_p2(-75)))[0] == 0.0
    assert O.closest_hit([s], (0, 0, 0), (0, 0, -_p2(-75)))[0] == -1
    # one binade up a is the least denormal and the near root 4 / 2^-74 is found
    best, rec = O.closest_hit([s], (0, 0, 0), (0, 0, -_p2(-74)))
    assert best == 0 and list(rec[1:4]) == [0, 0, -4.0]


def test_sphere_with_an_infinite_discriminant_misses():
    """|oc| = 5, r = 4.8, d = (0, 0, -2^63): b b = 25 * 2^126 overflows while a c = 1.96 * 2^126
    does not, disc = inf, and the roots are (-b -+ inf) / a = -+inf: a miss, although the ray
    points at the sphere."""
    s = _sphere((0.0, 0.0, -5.0), 4.8)
    assert O.closest_hit([s], (0, 0, 0), (0, 0, -_p2(63)))[0] == -1
    assert O.closest_hit([s], (0, 0, 0), (0, 0, -1.0))[0] == 0


def _sky(d):
    """The sky colour of direction d: one sample of an empty scene."""
    cam = O.OrCamera()
    for k in range(3):
        cam.lower_left[k] = float(f32(d[k]))
    cam.aspect, cam.focus_dist = 1.0, 1.0
    mean, _, cnt, _ = O.render([], cam, 1, 1, 1, 8, seed=1)
    assert cnt["segments"] == 1 and cnt["hits"] == 0
    return mean[0, 0]


def test_sky_of_overflowing_and_denormal_directions():
    up, mid = [f32(0.5), f32(0.7), f32(1.0)], [f32(0.75), f32(0.85), f32(1.0)]
    assert list(_sky((0, 3.0, 4.0))) == list((f32(1.0) - f32(0.8)) * f32(1.0) + f32(0.8) * np.asarray(up, dtype=f32))
    # dot(d, d) = inf: unit(d) = d / inf = 0 and the blend parameter is 0.5 whatever d.y is
    assert list(_sky((0, _p2(64), _p2(64)))) == mid and list(_sky((0, -_p2(64), 0))) == mid
    # dot(d, d) = 2^-140 is a denormal whose root 2^-70 is exact: straight up
    assert list(_sky((0, _p2(-70), 0))) == up
    # dot(d, d) underflows to 0: d.y / 0 = inf, and (1 - inf) + inf 0.5 is NaN
    assert np.isnan(_sky((0, _p2(-80), 0))).all()
