"""The trace kernel's segment set-up and its small frames on the device, after the lane loop shed
its copies and the reciprocal guard became one test over the three components.

- fr_selftest_boxinv returns the reciprocals rt_core.h seg_box_inv (the kernel's own function)
  forms for a list of directions: bit for bit numpy's RN(1 / x) clamped to +-2^100 over every
  triple of the guard's threshold values (tests/recip_guard_fixtures.py, the triples of
  tests/c/guard_root_check.cpp): the fast path where the guard admits it, the IEEE fallback
  elsewhere, and the lanes of one wave on both.
- Frames at 32 x 32, 1 and 4 spp, depth 8, of scene_08 and of the symmetric-slab scene of
  tests/test_slab_symmetric.py, with the axis-parallel and zero-component cameras of the edge-ray
  tests (the rays that reach the guard's fallback and the equal-distance roots): the scene kernel,
  the compiled-in kernel and the oracle agree bit for bit in mean, u8 and counters."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import ray_edge_fixtures as X
from tests.recip_guard_fixtures import clamped_recip, triples
from tests.test_slab_symmetric import EDGE, three_boxes

F = np.float32
DEPTH, W, H = 8, 32, 32
# d.x = +0 and -0, a ray inside a face plane, d = (0, 0, -1) through the centre and along an edge,
# d = 0 (every reciprocal clamped), a tiny and a denormal direction, a component crossing 2^-100
# inside a wave, one huge component
EDGE_NAMES = ["fan_x0", "fan_x_neg0", "fan_face_x", "fan_face_y", "beam_centre", "beam_edge", "still_inside",
              "m1_2^-100", "m1_2^-140", "m2_cross", "m2_2^126"]


@pytest.mark.gpu
def test_segment_reciprocals_equal_clamped_ieee_division(gpu):
    d = triples()
    out = np.zeros((len(d), 3), np.uint32)
    gpu.check(gpu.lib().fr_selftest_boxinv(0, d.ctypes.data_as(C.POINTER(C.c_float)), len(d),
                                           out.ctypes.data_as(C.POINTER(C.c_uint32))))
    want = clamped_recip(d).view(np.uint32)
    bad = np.flatnonzero((out != want).any(axis=1))
    assert len(d) == 28 ** 3 and bad.size == 0, (bad.size, d[bad[:4]], out[bad[:4]], want[bad[:4]])
    assert not np.isnan(out.view(F)).any() and (np.abs(out.view(F)) <= F(2.0 ** 100)).all()
    assert gpu.lib().fr_selftest_boxinv(0, None, 0, None) == gpu.FR_EARG


_want = {}


def _case(fr, scene, cam_name):
    """(prims for the product, camera, oracle camera, seed) of one scene and camera."""
    if scene == "scene_08":
        path = fr.scene_path("scene_08")
        with open(path) as f:
            prims, (frm, at, vup, fov) = S.load_json(f.read())
        sc = fr.Scene.from_file(path, W, H)
    else:
        prims = three_boxes()
        sc = fr.Scene.from_prims(prims)
        frm, at, vup, fov = (2.0, 3.0, 20.0), (0.0, 0.0, 0.0), (0, 1, 0), 60.0
    if cam_name == "look":
        cam = sc.camera if scene == "scene_08" else fr.camera_look(frm, at, vup, fov, 0.1, W, H)
        ocam = O.camera_look(frm, at, vup, fov, 0.1, W, H)
        assert np.array_equal(cam.to_array().view(np.uint32), O.camera_to_array(ocam).view(np.uint32))
    else:
        cam, ocam = X.edge_camera(fr, w=W, h=H, **EDGE[cam_name])
    return prims, sc, cam, ocam


def _oracle(fr, scene, cam_name, spp):
    key = (scene, cam_name, spp)
    if key not in _want:
        prims, _, _, ocam = _case(fr, scene, cam_name)
        mean, u8, cnt, _ = O.render(prims, ocam, W, H, spp, DEPTH, seed=X.SEED)
        mean.setflags(write=False)
        u8.setflags(write=False)
        _want[key] = (mean.view(np.uint32), u8, (cnt["segments"], cnt["hits"], cnt["scatters"]))
    return _want[key]


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("scene,cam_name", [("scene_08", "look"), ("three_boxes", "look")] +
                         [(s, n) for s in ("scene_08", "three_boxes") for n in EDGE_NAMES])
def test_small_frames_equal_the_oracle_on_both_kernels(gpu, scene, cam_name, spp):
    want = _oracle(gpu, scene, cam_name, spp)
    _, sc, cam, _ = _case(gpu, scene, cam_name)
    for jit in (True, False):
        ctx = gpu.RenderContext(0)
        try:
            ctx.render(sc, cam, gpu.make_params(W, H, spp, DEPTH, seed=X.SEED, scene_jit="wait" if jit else False))
            st = ctx.sync()
            mean, u8 = ctx.download(W, H)
            assert ctx.jit_info()["used"] == jit
        finally:
            ctx.close()
        got = (mean.view(np.uint32), u8, (st["segments"], st["hits"], st["scatters"]))
        tag = f"{scene} {cam_name} {spp} spp, {'scene' if jit else 'compiled-in'} kernel"
        same = (got[0] == want[0]) | (np.isnan(got[0].view(F)) & np.isnan(want[0].view(F)))  # NaN equal to NaN
        assert same.all(), f"{tag}: mean bits differ in {int((~same).any(axis=2).sum())} pixels"
        assert np.array_equal(got[1], want[1]), f"{tag}: u8"
        assert got[2] == want[2], f"{tag}: counters {got[2]} != {want[2]}"
