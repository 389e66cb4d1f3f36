"""The camera ray's short form for axis-aligned cameras (trace_kernel.h cam_ray_axial, chosen
per frame by render.hip cam_axial).

  - the host classifier on the bundled cameras and on cameras that break one condition each
    (no GPU);
  - both forms on the device over an adversarial grid of lens points and jitters: the six
    words of o and d are the same bits, zero signs included;
  - whole frames: scene kernel and compiled-in kernel, short form (asserted through
    RenderContext.camera_path) and FR_CAM_GENERAL=1, all equal to the oracle's frame bit for
    bit; an orbiting camera takes the general form and matches the oracle too.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref

F = np.float32
W, H, SPP, DEPTH = 64, 36, 4, 8  # the goldens' shape
FIELDS = ("position", "lower_left", "horizontal", "vertical", "u", "v", "w")
SCALARS = ("aspect", "lens_radius", "focus_dist", "radius", "rotation")


def _axial(fr, cam):
    return fr.lib().fr_camera_axial(C.byref(cam))


def _copy(fr, cam):
    out = fr.FrCamera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(fr.FrCamera))
    return out


def _bundled(fr, name):
    return fr.Scene.from_file(fr.scene_path(name), W, H)


def _oracle_camera(cam):
    """The oracle's camera with the product camera's bits, field by field."""
    ocam = O.OrCamera()
    for name in FIELDS:
        for k in range(3):
            getattr(ocam, name)[k] = getattr(cam, name)[k]
    for name in SCALARS:
        setattr(ocam, name, getattr(cam, name))
    assert np.array_equal(cam.to_array().view(np.uint32), O.camera_to_array(ocam).view(np.uint32))
    return ocam


def _synthetic(fr, pos=(0.0, 0.0, 0.0), ll=(-1.0, -0.5, -1.0), hx=2.0, vy=1.0, ux=-1.0, by=-1.0, lens=0.05):
    """An axial camera none of the bundled ones is: position +0 on every axis and v.y < 0, so
    both lens offsets can be -0 beside a +0 position."""
    cam = fr.FrCamera()
    vals = {"position": pos, "lower_left": ll, "horizontal": (hx, 0.0, -0.0), "vertical": (-0.0, vy, 0.0),
            "u": (ux, -0.0, 0.0), "v": (0.0, by, -0.0), "w": (0.0, 0.0, 1.0)}
    for name, vec in vals.items():
        for k in range(3):
            getattr(cam, name)[k] = float(F(vec[k]))
    cam.aspect, cam.lens_radius, cam.focus_dist, cam.radius, cam.rotation = W / H, float(F(lens)), 1.0, 5.0, 0.0
    return cam


# ---- the classifier (host only) ---------------------------------------------------------

def test_bundled_cameras_are_axial(fr):
    for i in range(1, 10):
        assert _axial(fr, _bundled(fr, f"scene_{i:02d}").camera) == 1, i
    assert _axial(fr, _synthetic(fr)) == 1
    assert fr.lib().fr_camera_axial(None) == fr.FR_EARG


def _set(field, k, value):
    def f(cam):
        getattr(cam, field)[k] = value
    return f


def _lens(value):
    def f(cam):
        cam.lens_radius = value
    return f


BREAKS = {
    "pos.x=-0": _set("position", 0, -0.0),
    "pos.y=-0": _set("position", 1, -0.0),
    "pos.z=-0": _set("position", 2, -0.0),
    "llc.x=0": _set("lower_left", 0, 0.0),
    "llc.y=-0": _set("lower_left", 1, -0.0),
    "llc.z=0": _set("lower_left", 2, 0.0),
    "lens=0": _lens(0.0),
    "lens<0": _lens(-0.05),
    "lens=2^-140": _lens(float(np.ldexp(1.0, -140))),  # lens 2^-23 is not exact
    "lens*|ux|<2^-100": _lens(float(np.ldexp(1.0, -90))),  # lens_s = 2^-113
    "u.y=2^-149": _set("u", 1, float(np.ldexp(1.0, -149))),
    "u.z=2^-149": _set("u", 2, float(np.ldexp(1.0, -149))),
    "v.x=-2^-149": _set("v", 0, -float(np.ldexp(1.0, -149))),
    "v.z=1": _set("v", 2, 1.0),
    "hor.y=2^-149": _set("horizontal", 1, float(np.ldexp(1.0, -149))),
    "hor.z=2^-149": _set("horizontal", 2, float(np.ldexp(1.0, -149))),
    "ver.x=2^-149": _set("vertical", 0, float(np.ldexp(1.0, -149))),
    "ver.z=2^-149": _set("vertical", 2, float(np.ldexp(1.0, -149))),
    "u.x=0": _set("u", 0, 0.0),
    "v.y=0": _set("v", 1, -0.0),
    "pos.y=inf": _set("position", 1, float("inf")),
    "hor.x=inf": _set("horizontal", 0, float("inf")),
    "llc.z=nan": _set("lower_left", 2, float("nan")),
    "ver.y=-inf": _set("vertical", 1, float("-inf")),
    "lens=inf": _lens(float("inf")),
}


@pytest.mark.parametrize("name", sorted(BREAKS))
def test_one_broken_condition_is_general(fr, name):
    for base in (_bundled(fr, "scene_08").camera, _bundled(fr, "scene_01").camera, _synthetic(fr)):
        cam = _copy(fr, base)
        assert _axial(fr, cam) == 1
        BREAKS[name](cam)
        assert _axial(fr, cam) == 0, name


def test_orbit_and_default_cameras_are_general(fr):
    cam = _copy(fr, _bundled(fr, "scene_08").camera)
    fr.camera_orbit(cam, (0.3, 0.1, 0.2))  # Camera::orbit's formulas
    assert _axial(fr, cam) == 0
    # a quarter turn: u and v are axis-aligned to within cosf's rounding, not exactly
    cam = _copy(fr, _bundled(fr, "scene_01").camera)
    fr.camera_orbit(cam, (float(np.pi / 2), 0.0, 0.0))
    assert _axial(fr, cam) == 0
    assert _axial(fr, fr.camera_new(W, H)) == 0  # lens_radius 0


# ---- both forms on the device -----------------------------------------------------------

def _grid():
    k = [0.0, 1.0, -1.0, 2.0, -2.0, float(2 ** 23 - 1), -float(2 ** 23 - 1)]
    st = [0.0, float(np.ldexp(1.0, -24)), 0.5, float(1.0 - np.ldexp(1.0, -24))]
    g = np.array([(kx, ky, s, t) for kx in k for ky in k for s in st for t in st], dtype=F)
    assert g.shape == (784, 4)
    return g


def _camray(fr, cam, grid):
    out = np.zeros((len(grid), 12), dtype=np.uint32)
    fr.check(fr.lib().fr_selftest_camray(0, C.byref(cam), grid.ctypes.data_as(C.POINTER(C.c_float)), len(grid),
                                         out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene_08", "scene_01", "synthetic", "synthetic_pos", "synthetic_mixed"])
def test_device_short_form_equals_general_form(gpu, which):
    if which.startswith("scene"):
        cam = _bundled(gpu, which).camera
        # s = 0.5 makes lower_left.x + s horizontal.x exactly +0 for the bundled cameras
        assert F(cam.lower_left[0]) + F(0.5) * F(cam.horizontal[0]) == 0.0
    elif which == "synthetic":
        cam = _synthetic(gpu)
    elif which == "synthetic_pos":  # u.x, v.y > 0; lower_left - position exactly 0 in z
        cam = _synthetic(gpu, pos=(1.0, -0.5, -1.0), ll=(-1.0, 0.5, -1.0), ux=1.0, by=1.0)
    else:  # lower_left + s horizontal cancels position at s = 0.5, t = 0.5
        cam = _synthetic(gpu, pos=(0.0, 0.0, 2.0), ll=(-1.0, -0.5, 1.0), ux=-0.75, by=1.5, lens=0.3)
    assert _axial(gpu, cam) == 1
    grid = _grid()
    out = _camray(gpu, cam, grid)
    bad = np.nonzero((out[:, :6] != out[:, 6:]).any(axis=1))[0]
    assert bad.size == 0, (which, grid[bad[:4]], out[bad[:4]])
    # the grid reaches the zero-sign cases it is built for: a -0 lens offset and a zero in d
    o = out[:, :6].view(F)
    assert np.isfinite(o).all()
    if which != "synthetic_pos":
        assert (out[:, 3:5] << 1 == 0).any(), "no d component is a zero"


@pytest.mark.gpu
def test_device_self_test_refuses_a_general_camera(gpu):
    cam = _copy(gpu, _bundled(gpu, "scene_08").camera)
    gpu.camera_orbit(cam, (0.3, 0.1, 0.2))
    grid = _grid()[:4]
    out = np.zeros((4, 12), dtype=np.uint32)
    rc = gpu.lib().fr_selftest_camray(0, C.byref(cam), grid.ctypes.data_as(C.POINTER(C.c_float)), 4,
                                      out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == gpu.FR_EARG


# ---- frames -----------------------------------------------------------------------------

_oracle = {}


def _reference(fr, name, orbit):
    """(scene, camera, oracle mean, u8, counters), rendered once and shared read-only."""
    key = (name, orbit)
    if key not in _oracle:
        sc = _bundled(fr, name)
        with open(fr.scene_path(name)) as f:
            prims, _ = scene_ref.load_json(f.read())
        cam = _copy(fr, sc.camera)
        if orbit:
            fr.camera_orbit(cam, (0.3, 0.1, 0.2))
        mean, u8, cnt, _ = O.render(prims, _oracle_camera(cam), W, H, SPP, DEPTH)
        mean.setflags(write=False)
        u8.setflags(write=False)
        _oracle[key] = (sc, cam, mean, u8, cnt)
    return _oracle[key]


def _frame(fr, sc, cam, jit):
    ctx = fr.RenderContext(0)
    try:
        ctx.render(sc, cam, fr.make_params(W, H, SPP, DEPTH, scene_jit="wait" if jit else False))
        st = ctx.sync()
        mean, u8 = ctx.download(W, H)
        return mean, u8, st, ctx.camera_path(), ctx.jit_info()["used"]
    finally:
        ctx.close()


def _assert_equal(got, want, tag):
    mean, u8, st = got
    omean, ou8, ocnt = want
    assert np.array_equal(mean.view(np.uint32), omean.view(np.uint32)), f"{tag}: mean bits"
    assert np.array_equal(u8, ou8), f"{tag}: u8"
    for k in ("segments", "hits", "scatters"):
        assert st[k] == ocnt[k], f"{tag}: {k} {st[k]} != {ocnt[k]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_08", "scene_01"])
def test_frames_short_and_general_form_equal_the_oracle(gpu, name, monkeypatch):
    sc, cam, omean, ou8, ocnt = _reference(gpu, name, False)
    assert _axial(gpu, cam) == 1
    for jit in (True, False):
        for forced in (False, True):
            if forced:
                monkeypatch.setenv("FR_CAM_GENERAL", "1")
            else:
                monkeypatch.delenv("FR_CAM_GENERAL", raising=False)
            mean, u8, st, path, used = _frame(gpu, sc, cam, jit)
            assert path == ("general" if forced else "axial"), (jit, forced, path)
            assert used == jit
            _assert_equal((mean, u8, st), (omean, ou8, ocnt), f"{name} jit={jit} forced={forced}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_08", "scene_01"])
def test_frames_of_an_orbit_camera_take_the_general_form(gpu, name, monkeypatch):
    monkeypatch.delenv("FR_CAM_GENERAL", raising=False)
    sc, cam, omean, ou8, ocnt = _reference(gpu, name, True)
    assert _axial(gpu, cam) == 0
    for jit in (True, False):
        mean, u8, st, path, used = _frame(gpu, sc, cam, jit)
        assert path == "general" and used == jit
        _assert_equal((mean, u8, st), (omean, ou8, ocnt), f"{name} orbit jit={jit}")


@pytest.mark.gpu
def test_prepare_reports_the_path_too(gpu, monkeypatch):
    monkeypatch.delenv("FR_CAM_GENERAL", raising=False)
    sc = _bundled(gpu, "scene_08")
    ctx = gpu.RenderContext(0)
    try:
        ctx.prepare(sc, sc.camera, gpu.make_params(W, H, SPP, DEPTH))
        assert ctx.camera_path() == "axial"
        monkeypatch.setenv("FR_CAM_GENERAL", "1")
        ctx.prepare(sc, sc.camera, gpu.make_params(W, H, SPP, DEPTH))
        assert ctx.camera_path() == "general"
    finally:
        ctx.close()
