"""Mirrored box pairs (rt_core.h slab_pair_root): two boxes adjacent in the list that share two
slabs and mirror each other on the third axis are tested by the scene kernel in ray order, with
one update of the closest hit. The compiled-in kernel and the oracle walk the list in order, so
the three must agree bit for bit (means, u8, counters) on scenes built to take the pair form and
on scenes built to refuse it:

  scene_08       its own pairs (0, 1) touching in y and (3, 4) separated in z; boxes 2 and 5 mirror
                 each other but are not adjacent
  pairs          a separated pair on x (boxes 0, 1) and a touching pair on z (boxes 2, 3), the box on
                 the negative side first
  reversed       the same boxes, the one on the positive side first
  ulp_off        one coordinate of each pair off by one ulp: no pair, the general path
  non_adjacent   the pairs' boxes interleaved: no pair
  wall_x/y/z     a thin wall of two boxes touching in the plane 0 of one axis, as scene_08's boxes 0
                 and 1 do in y; one view from inside the wall on that plane (every primary ray starts
                 in one of the two boxes and many leave through the shared plane, where the two
                 accepted roots are equal and the list's first box must win), one from outside

Cameras: look-at cameras at the goldens' frame shape (64 x 36, 4 spp, depth 8), then the edge-ray
cameras of tests/ray_edge_fixtures.py (exactly axis-parallel rays, rays inside a face plane or the
shared plane, d = 0) and the tiny, huge and far-away rays of tests/magnitude_fixtures.py, built by
edge_camera as those tests build them, at their 16 x 16 frame.
"""
import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import magnitude_fixtures as M
from tests import ray_edge_fixtures as X

F = np.float32
DEPTH = 8


def _up(x):
    return float(np.nextafter(F(x), F(np.inf)))


def _box(lo, hi, colour=(0.7, 0.7, 0.7), mat=S.LAMBERTIAN):
    return S.prim(S.AABB, mat, colour, 0.0, list(lo) + list(hi))


RED, BLUE, GREEN, AMBER = (0.75, 0.25, 0.25), (0.25, 0.25, 0.75), (0.25, 0.75, 0.25), (0.75, 0.6, 0.25)
# the separated pair on x and the touching pair on z (tests/c/pair_order_check.cpp's shapes)
SEP_LOW, SEP_UP = ((-3.0, -2.0, -4.0), (-1.0, 2.0, -2.0)), ((1.0, -2.0, -4.0), (3.0, 2.0, -2.0))
TOUCH_LOW, TOUCH_UP = ((-1.0, 0.5, -2.0), (1.5, 2.0, 0.0)), ((-1.0, 0.5, 0.0), (1.5, 2.0, 2.0))
REST = [_box((-8.0, -3.0, -8.0), (8.0, -2.5, 8.0)), _box((-8.0, 9.0, -8.0), (8.0, 10.0, 8.0), (1.0, 1.0, 1.0), S.LIGHT)]


def _four(order, sep_up=SEP_UP, touch_up=TOUCH_UP):
    b = {"sl": _box(*SEP_LOW, RED), "su": _box(*sep_up, BLUE), "tl": _box(*TOUCH_LOW, GREEN), "tu": _box(*touch_up, AMBER)}
    return [b[k] for k in order] + REST


def _wall(axis):
    """Two boxes touching in the plane 0 of `axis`, 0.5 thick on the next axis, 12 long on the
    third; a lambertian slab on one side of the wall and a light on the other."""
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3

    def at(va, vb, vc):
        p = [0.0, 0.0, 0.0]
        p[a], p[b], p[c] = va, vb, vc
        return p

    return [_box(at(-3.0, -0.25, -6.0), at(0.0, 0.25, 6.0), RED), _box(at(0.0, -0.25, -6.0), at(3.0, 0.25, 6.0), BLUE),
            _box(at(-5.0, 4.0, -8.0), at(5.0, 4.5, 8.0), GREEN),
            _box(at(-5.0, -6.0, -8.0), at(5.0, -5.5, 8.0), (1.0, 1.0, 1.0), S.LIGHT)]


def _wall_views(axis):
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3

    def at(va, vb, vc):
        p = [0.0, 0.0, 0.0]
        p[a], p[b], p[c] = va, vb, vc
        return tuple(p)

    up = at(1.0, 0.0, 0.0)
    return {"inside": (at(0.0, 0.0, -5.0), at(0.0, 0.0, 5.0), up), "outside": (at(1.0, 9.0, -9.0), at(0.0, 0.0, 0.0), up)}


SCENES = {
    "pairs": _four(("sl", "su", "tl", "tu")),
    "reversed": _four(("su", "sl", "tu", "tl")),
    "ulp_off": _four(("sl", "su", "tl", "tu"), sep_up=((_up(1.0), -2.0, -4.0), (3.0, 2.0, -2.0)),
                     touch_up=((-1.0, 0.5, 0.0), (1.5, 2.0, _up(2.0)))),
    "non_adjacent": _four(("sl", "tl", "su", "tu")),
    "wall_x": _wall(0),
    "wall_y": _wall(1),
    "wall_z": _wall(2),
}

LOOK = {  # (from, at, up)
    "look_front": ((0.5, 1.0, 9.0), (0.0, 0.0, -1.0), (0, 1, 0)),
    "look_in_touching": ((0.25, 1.25, 0.0), (0.0, 1.0, -6.0), (0, 1, 0)),  # inside the pair, on its shared plane
}
EDGE = {
    "fan_x0": X._fan_x(0.0),                          # d.x = +0, between the separated pair
    "fan_x_neg0": X._fan_x(0.0, zero=X.NEG0),         # d.x = -0
    "fan_face_x": X._fan_x(1.0),                      # inside the separated pair's inner face x = 1
    "fan_face_x_neg": X._fan_x(-1.0, lens=0.5),       # x = -1: its other inner face and the touching pair's
    "fan_face_y": X._fan_y(0.5, 0.5, 0.0),            # inside the touching pair's face y = 0.5, from its shared plane
    "beam_shared": X._beam(0.0, 1.0),                 # d = (0, 0, -1) from the shared plane z = 0
    "beam_edge": X._beam(1.0, 0.5),                   # along an edge of the touching pair
    "still_inside": X._still((0.25, 1.0, 0.0)),       # d = 0 on the shared plane: every reciprocal clamped
    "still_outside": X._still((0.25, 0.5, 5.0)),
    "m1_2^40": M._m1_cam(40),                         # every component huge
    "m1_2^64": M._m1_cam(64),                         # dot(d, d) = inf
    "m1_2^-100": M._m1_cam(-100),                     # the box reciprocal's fallback and clamp
    "m1_2^-140": M._m1_cam(-140),                     # denormal components
    "m2_2^-110": M._m2_cam(M.p2(-110)),               # one tiny component
    "m2_2^126": M._m2_cam(M.p2(126)),                 # one huge component: inv underflows
    "m2_cross": M._m2_cam(0.0, hx=M.p2(-96)),         # d.x crosses 2^-100 inside a wave
    "m4_2^21": M._m4_cam(21),                         # far origin: o inv ~ 2^121
    "m4_2^30": M._m4_cam(30),                         # o inv overflows: every slab distance infinite
}
FEW = ("fan_x_neg0", "beam_shared", "still_inside", "m2_cross")


def cases():
    out = [("scene_08", "own"), ("scene_08", "wall_up"), ("scene_08", "wall_down")]
    out += [("scene_08", v) for v in FEW]
    out += [("pairs", v) for v in list(LOOK) + sorted(EDGE)]
    for name in ("reversed", "ulp_off", "non_adjacent"):
        out += [(name, v) for v in list(LOOK) + list(FEW)]
    for name in ("wall_x", "wall_y", "wall_z"):
        out += [(name, "inside"), (name, "outside")]
    return out


def _prims(scene):
    if scene == "scene_08":
        import forma_rt as fr
        with open(fr.scene_path("scene_08")) as f:
            return S.load_json(f.read())[0]
    return SCENES[scene]


def test_scenes_have_the_pairs_they_are_built_for():
    """The fixtures' geometry, restated here. Which of these boxes the scene kernel pairs is asked
    of its own constant expression in tests/test_pair_predicate.py (the renders below cannot
    tell: both paths give the same bits)."""
    def mirrored(p, q):
        """the axis on which q mirrors p with the other two slabs equal, else None"""
        g, h = np.asarray(p["g"][:6], F), np.asarray(q["g"][:6], F)
        same = [k for k in range(3) if g[k] == h[k] and g[k + 3] == h[k + 3]]
        mir = [k for k in range(3) if h[k] == -g[k + 3] and h[k + 3] == -g[k] and (g[k + 3] <= 0 or g[k] >= 0)]
        return mir[0] if len(same) == 2 and len(mir) == 1 and mir[0] not in same else None

    def adjacent_pairs(prims):
        return [(i, mirrored(prims[i], prims[i + 1])) for i in range(len(prims) - 1)
                if mirrored(prims[i], prims[i + 1]) is not None]

    assert adjacent_pairs(_prims("scene_08")) == [(0, 1), (3, 2)]
    assert mirrored(_prims("scene_08")[2], _prims("scene_08")[5]) == 1
    assert adjacent_pairs(SCENES["pairs"]) == [(0, 0), (2, 2)] == adjacent_pairs(SCENES["reversed"])
    assert adjacent_pairs(SCENES["ulp_off"]) == [] == adjacent_pairs(SCENES["non_adjacent"])
    assert mirrored(SCENES["non_adjacent"][0], SCENES["non_adjacent"][2]) == 0
    for k in range(3):
        assert adjacent_pairs(SCENES["wall_" + "xyz"[k]]) == [(0, k)]


_frames = {}


def _frame(fr, scene, view):
    """(w, h, spp, seed, camera, oracle mean, u8, counters): the oracle's frame, rendered once."""
    if (scene, view) not in _frames:
        look = None
        if scene == "scene_08" and view in ("own", "wall_up", "wall_down"):
            # its own camera stands inside the wall of boxes 0 and 1 on their shared plane y = 0; the
            # other two look along the wall, up into box 1 and down into box 0
            with open(fr.scene_path("scene_08")) as f:
                frm, at, vup, _ = S.load_json(f.read())[1]
            look = {"own": (frm, at, vup), "wall_up": ((0.0, 0.0, -20.0), (0.0, 10.0, 20.0), (0, 1, 0)),
                    "wall_down": ((0.0, 0.0, 20.0), (0.0, -10.0, -20.0), (0, 1, 0))}[view]
        elif view in LOOK:
            look = LOOK[view]
        elif scene.startswith("wall_"):
            look = _wall_views("xyz".index(scene[-1]))[view]
        if look is not None:
            w, h, spp, seed = 64, 36, 4, None
            cam = fr.camera_look(look[0], look[1], look[2], 60.0, 0.1, w, h)
            ocam = O.camera_look(look[0], look[1], look[2], 60.0, 0.1, w, h)
            assert np.array_equal(cam.to_array().view(np.uint32), O.camera_to_array(ocam).view(np.uint32))
        else:
            w, h, spp, seed = X.W, X.H, X.SPP, X.SEED
            cam, ocam = X.edge_camera(fr, w=w, h=h, **EDGE[view])
        kw = {} if seed is None else {"seed": seed}
        mean, u8, cnt, _ = O.render(_prims(scene), ocam, w, h, spp, DEPTH, **kw)
        mean.setflags(write=False)
        u8.setflags(write=False)
        _frames[scene, view] = (w, h, spp, seed, cam, mean, u8, cnt)
    return _frames[scene, view]


def _render(fr, sc, cam, w, h, spp, seed, jit):
    ctx = fr.RenderContext(0)
    try:
        kw = {} if seed is None else {"seed": seed}
        ctx.render(sc, cam, fr.make_params(w, h, spp, DEPTH, scene_jit="wait" if jit else False, **kw))
        st = ctx.sync()
        mean, u8 = ctx.download(w, h)
        return mean, u8, st, ctx.jit_info()["used"]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,view", cases())
def test_scene_kernel_equals_compiled_in_kernel_and_oracle(gpu, scene, view):
    w, h, spp, seed, cam, omean, ou8, ocnt = _frame(gpu, scene, view)
    sc = (gpu.Scene.from_file(gpu.scene_path("scene_08"), w, h) if scene == "scene_08"
          else gpu.Scene.from_prims(_prims(scene)))
    got = {}
    for jit in (True, False):
        mean, u8, st, used = _render(gpu, sc, cam, w, h, spp, seed, jit)
        assert used == jit
        got[jit] = (mean.view(np.uint32), u8, (st["segments"], st["hits"], st["scatters"]))
    want = (omean.view(np.uint32), ou8, (ocnt["segments"], ocnt["hits"], ocnt["scatters"]))
    for tag, a, b in (("scene kernel vs compiled-in", got[True], got[False]), ("scene kernel vs oracle", got[True], want),
                      ("compiled-in vs oracle", got[False], want)):
        same = (a[0] == b[0]) | (np.isnan(a[0].view(F)) & np.isnan(b[0].view(F)))  # NaN equal to NaN
        assert same.all(), f"{scene}/{view}: {tag}: mean bits differ in {int((~same).any(axis=2).sum())} pixels"
        assert np.array_equal(a[1], b[1]), f"{scene}/{view}: {tag}: u8"
        assert a[2] == b[2], f"{scene}/{view}: {tag}: counters {a[2]} != {b[2]}"
    if w == 64:  # the look-at views are about the boxes
        assert ocnt["hits"] > 0
