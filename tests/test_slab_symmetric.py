"""Box slabs symmetric about a coordinate plane (rt_core.h slab_axis): the scene kernel, whose
records are compile-time constants, forms the near and far distance of a pair lo = -hi already
sorted and skips its min / max. The compiled-in kernel and the oracle do not, so the three must
agree bit for bit on a scene built to take the shortcut on some axes and to refuse it on others:

  box 0   symmetric about the origin on every axis (the cameras stand inside or outside it)
  box 1   symmetric in x only
  box 2   hi = -lo off by one ulp in x and in z (no shortcut: the plane would move by an ulp),
          unsymmetric in y
  box 3   a light above, symmetric in x and z

Cameras: look-at cameras inside and outside box 0 at the goldens' frame shape, then the
edge-ray cameras of tests/ray_edge_fixtures.py (exactly axis-parallel rays, rays inside a face
plane, d = 0) and the tiny, huge and far-away rays of tests/magnitude_fixtures.py, built by
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


def _down(x):
    return float(np.nextafter(F(x), F(0.0)))


def three_boxes():
    grey, red, blue = (0.7, 0.7, 0.7), (0.75, 0.25, 0.25), (0.25, 0.25, 0.75)
    return [
        S.prim(S.AABB, S.LAMBERTIAN, grey, 0.0, [-3.0, -2.0, -4.0, 3.0, 2.0, 4.0]),
        S.prim(S.AABB, S.LAMBERTIAN, red, 0.0, [-1.0, 2.5, -9.0, 1.0, 4.0, -6.0]),
        S.prim(S.AABB, S.LAMBERTIAN, blue, 0.0, [-1.5, -6.0, -6.0, _up(1.5), -3.0, _down(6.0)]),
        S.prim(S.AABB, S.LIGHT, (1.0, 1.0, 1.0), 0.0, [-8.0, 9.0, -8.0, 8.0, 10.0, 8.0]),
    ]


def test_scene_has_the_pairs_it_is_built_for():
    g = [p["g"] for p in three_boxes()]
    sym = [[bool(b[k] == -b[k + 3]) for k in range(3)] for b in g]
    assert sym == [[True, True, True], [True, False, False], [False, False, False], [True, False, True]]
    assert g[2][3] != -g[2][0] and abs(g[2][3] + g[2][0]) < 2e-7 and abs(g[2][5] + g[2][2]) < 1e-6


# name -> (width, height, spp, product camera and oracle camera of one frame)
def _look(fr, frm, at, w, h):
    cam = fr.camera_look(frm, at, (0, 1, 0), 60.0, 0.1, w, h)
    ocam = O.camera_look(frm, at, (0, 1, 0), 60.0, 0.1, w, h)
    assert np.array_equal(cam.to_array().view(np.uint32), O.camera_to_array(ocam).view(np.uint32))
    return cam, ocam


EDGE = {
    "fan_x0": X._fan_x(0.0),                      # d.x = +0 through the centre plane of box 0
    "fan_x_neg0": X._fan_x(0.0, zero=X.NEG0),     # d.x = -0
    "fan_face_x": X._fan_x(-3.0),                 # inside box 0's face plane x = -3: grazes it
    "fan_face_x_lens": X._fan_x(3.0, lens=0.5),
    "fan_face_y": X._fan_y(0.5, -2.0, 0.0),       # inside its face plane y = -2, d.y = +0
    "beam_centre": X._beam(0.0, 0.0),             # d = (0, 0, -1)
    "beam_edge": X._beam(-3.0, -2.0),             # along an edge of box 0
    "beam_outside": X._beam(0.5, 3.0, 6.0),       # onto box 1's z face
    "still_inside": X._still((0.25, 0.5, 0.5)),   # d = 0: every reciprocal clamped
    "still_outside": X._still((0.25, 0.5, 5.0)),
    "m1_2^40": M._m1_cam(40),                     # every component huge
    "m1_2^64": M._m1_cam(64),                     # dot(d, d) = inf
    "m1_2^-100": M._m1_cam(-100),                 # the box reciprocal's fallback and clamp
    "m1_2^-140": M._m1_cam(-140),                 # denormal components
    "m2_2^-110": M._m2_cam(M.p2(-110)),           # one tiny component
    "m2_2^126": M._m2_cam(M.p2(126)),             # one huge component: inv underflows
    "m2_cross": M._m2_cam(0.0, hx=M.p2(-96)),     # d.x crosses 2^-100 inside a wave
    "m4_2^21": M._m4_cam(21),                     # far origin: o inv ~ 2^121
    "m4_2^30": M._m4_cam(30),                     # o inv overflows: every slab distance infinite
}

_frames = {}


def _frame(fr, name):
    """(w, h, spp, seed, camera, oracle mean, u8, counters): the oracle's frame, rendered once."""
    if name not in _frames:
        if name in ("look_inside", "look_outside"):
            w, h, spp, seed = 64, 36, 4, None
            cam, ocam = _look(fr, (0.5, 0.25, 1.0) if name == "look_inside" else (2.0, 3.0, 20.0),
                              (0.0, 0.0, -1.0) if name == "look_inside" else (0.0, 0.0, 0.0), w, h)
        else:
            w, h, spp, seed = X.W, X.H, X.SPP, X.SEED
            cam, ocam = X.edge_camera(fr, w=w, h=h, **EDGE[name])
        kw = {} if seed is None else {"seed": seed}
        mean, u8, cnt, _ = O.render(three_boxes(), ocam, w, h, spp, DEPTH, **kw)
        mean.setflags(write=False)
        u8.setflags(write=False)
        _frames[name] = (w, h, spp, seed, cam, mean, u8, cnt)
    return _frames[name]


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
@pytest.mark.parametrize("name", ["look_inside", "look_outside"] + sorted(EDGE))
def test_scene_kernel_equals_compiled_in_kernel_and_oracle(gpu, name):
    w, h, spp, seed, cam, omean, ou8, ocnt = _frame(gpu, name)
    sc = gpu.Scene.from_prims(three_boxes())
    got = {}
    for jit in (True, False):
        mean, u8, st, used = _render(gpu, sc, cam, w, h, spp, seed, jit)
        assert used == jit
        got[jit] = (mean.view(np.uint32), u8, (st["segments"], st["hits"], st["scatters"]))
    want = (omean.view(np.uint32), ou8, (ocnt["segments"], ocnt["hits"], ocnt["scatters"]))
    for tag, a, b in (("scene kernel vs compiled-in", got[True], got[False]), ("scene kernel vs oracle", got[True], want),
                      ("compiled-in vs oracle", got[False], want)):
        same = (a[0] == b[0]) | (np.isnan(a[0].view(F)) & np.isnan(b[0].view(F)))  # NaN equal to NaN
        assert same.all(), f"{name}: {tag}: mean bits differ in {int((~same).any(axis=2).sum())} pixels"
        assert np.array_equal(a[1], b[1]), f"{name}: {tag}: u8"
        assert a[2] == b[2], f"{name}: {tag}: counters {a[2]} != {b[2]}"
    if name.startswith("look"):  # the frame is about the boxes: most paths hit one
        assert ocnt["hits"] * 2 >= ocnt["segments"] or name == "look_outside"
        assert ocnt["hits"] > 0
