"""Ray queries (fr_ctx_cast) and the G-buffer's tree walk on the GPU against the oracle, bit for bit.

The contract (include/forma_rt.h): per ray the closest primitive in list order, its own accepted
root, its normal at that root, the point o + t d and the primitive's attenuation; a miss writes id
0xFFFFFFFF, zeros and albedo 1. A scene that has a tree is walked through it, with the bits of the
list loop; a wave of 64 rays holding a ray the tree's cull is not conservative for walks the
list. The cast touches nothing else of the context.

Expected values: tests/cast_fixtures.py (the oracle's closest-hit loop per ray: winner and normal
from oracle_closest_hit, own root from the list cut after the winner), which
tests/test_cast_host.py holds against the bits of the header the kernels compile, and
tests/gbuffer_ref.py for the views."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import cast_fixtures as CF
from tests import gbuffer_ref as G
from tests import ray_edge_fixtures as X
from tests.test_accum_error import SEED0, _composites, _refused
from tests.test_accumulate import _product_scene
from tests.test_denoise import _check_denoised, _check_state_untouched, _expected

pytestmark = pytest.mark.gpu
F = np.float32


def _waves(n):
    return (n + 63) // 64


def _pixel_rays(gpu, cam, w, h):
    o, d = np.zeros((w * h, 3), F), np.zeros((w * h, 3), F)
    for y in range(h):
        for x in range(w):
            o[y * w + x], d[y * w + x] = gpu.pixel_ray(cam, x, y, w, h)
    return o, d


@pytest.mark.parametrize("name", list(G.CASES))
def test_pixel_rays_equal_the_gbuffer_reference(gpu, name):
    _, cam, _, w, h, sc = G.case(gpu, name)
    want = G.expected(gpu, name)
    ctx = gpu.RenderContext(0)
    got = ctx.cast(sc, *_pixel_rays(gpu, cam, w, h))
    assert G.same(CF.as_gbuffer(got, w, h), want) == []
    info = ctx.cast_info()
    assert info["n"] == w * h and info["waves_tree"] + info["waves_list"] == _waves(w * h)
    if name in ("spheres200", "scene_08", "lattice_box"):  # 200 spheres are past the tree's threshold, 6 and 10 boxes are not
        assert info["tree"] == (1 if name == "spheres200" else 0)
    ctx.close()


@pytest.mark.parametrize("kind", X.KINDS)
def test_lattice_batches_equal_the_oracle(gpu, kind):
    b, want = CF.batch(gpu, kind), CF.expected(gpu, kind)
    sc = gpu.Scene.from_prims(b["prims"])
    n = len(b["o"])
    ctx = gpu.RenderContext(0)
    got = ctx.cast(sc, b["o"], b["d"])
    info = ctx.cast_info()
    assert CF.same(got, want) == []
    assert info["n"] == n and info["waves_tree"] + info["waves_list"] == _waves(n)
    if kind == "plane":  # 54 planes exceed kBvhMaxPlanes: no tree
        assert info["tree"] == 0 and info["waves_tree"] == 0
    else:
        assert info["tree"] == 1 and info["waves_tree"] > 0 and info["waves_list"] > 0
        assert info["waves_list"] == len(CF.fallback_waves(b))
    got = ctx.cast(sc, b["o"], b["d"], list_walk=True)  # FR_CAST_LIST
    info = ctx.cast_info()
    assert CF.same(got, want) == []
    assert info["tree"] == 0 and info["waves_tree"] == 0 and info["waves_list"] == _waves(n)
    ctx.close()


def _gen_scene(gpu, count, w, h):
    text, prims, ocam = CF.gen_spheres(gpu, count, w, h)
    sc = gpu.Scene.from_json(text, w, h)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(G.cam_fields(sc.camera), G.cam_fields(ocam)))
    return sc, prims, ocam


def test_generator_spheres_equal_the_oracle(gpu):
    """2,000 spheres: a tree about ten levels deep, so the per-lane stack is pushed and popped;
    batches of 1, 63, 64, 65 and 321 rays for the tail of the last wave."""
    w, h = 24, 16
    sc, _, _ = _gen_scene(gpu, 2000, w, h)
    prims, o, d, want = CF.gen_batch(gpu, 2000, w, h)
    ctx = gpu.RenderContext(0)
    got = ctx.cast(sc, o, d)
    info = ctx.cast_info()
    assert CF.same(got, want) == []
    assert info == {"n": len(o), "tree": 1, "waves_tree": _waves(len(o)), "waves_list": 0}
    assert CF.same(ctx.cast(sc, o, d, list_walk=True), want) == []
    for n in (1, 63, 64, 65, 321):
        sel = slice(100, 100 + n)
        got = ctx.cast(sc, o[sel], d[sel])
        assert len(got["prim"]) == n
        for name in ("prim", "t", "normal", "position", "albedo"):
            assert np.array_equal(got[name].view(np.uint32), want[name][sel].view(np.uint32)), (n, name)
        assert ctx.cast_info() == {"n": n, "tree": 1, "waves_tree": _waves(n), "waves_list": 0}
    ctx.close()


def test_gbuffer_walks_the_tree_of_a_tree_scene(gpu):
    """fr_ctx_gbuffer on scenes with a tree equals gbuffer_ref.gbuffer and says tree; from a
    camera beyond the tree's reach it says list, with the oracle's bits for that camera."""
    w, h = 24, 16
    sc, prims, ocam = _gen_scene(gpu, 2000, w, h)
    ctx = gpu.RenderContext(0)
    _refused(gpu, ctx.gbuffer_info, "no G-buffer")
    ctx.gbuffer(sc, sc.camera, w, h)
    assert ctx.gbuffer_info() == "tree"
    want = G.cached(("gen", 2000, w, h), prims, ocam, w, h)
    assert G.same(ctx.download_gbuffer(w, h), want) == []
    assert (want["prim"] != G.MISS).any() and (want["prim"] == G.MISS).any()
    # the view's pixel rays through the cast are the same pixels
    assert G.same(CF.as_gbuffer(ctx.cast(sc, *_pixel_rays(gpu, sc.camera, w, h)), w, h), want) == []
    # beyond the reach (at most 100 (extent + 1)): the list
    far = 200.0 * (CF.extent_bounds(prims)[1] + 1.0)
    frm, at, vup = (0.0, 0.25 * far, far), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    cam = gpu.camera_look(frm, at, vup, 40.0, 0.0, w, h)
    ocam_far = O.camera_look(frm, at, vup, 40.0, 0.0, w, h)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(G.cam_fields(cam), G.cam_fields(ocam_far)))
    ctx.gbuffer(sc, cam, w, h)
    assert ctx.gbuffer_info() == "list"
    assert G.same(ctx.download_gbuffer(w, h), G.cached(("gen_far", 2000, w, h), prims, ocam_far, w, h)) == []
    # the big mixed lattice: planes between the runs, stale records, stubs
    fx = X.fixture("mixed", "R0_control")
    prims = CF.lattice_prims("mixed")
    cam, ocam = X.edge_camera(gpu, w=16, h=16, **fx.cam)
    msc = gpu.Scene.from_prims(prims)
    ctx.gbuffer(msc, cam, 16, 16)
    assert ctx.gbuffer_info() == "tree"
    want = G.cached(("mixed_big", 16, 16), prims, ocam, 16, 16)
    assert G.same(ctx.download_gbuffer(16, 16), want) == [] and want["stale"].any()
    # a scene below the tree's threshold keeps the list
    _, cam8, _, w8, h8, sc8 = G.case(gpu, "scene_08")
    ctx.gbuffer(sc8, cam8, w8, h8)
    assert ctx.gbuffer_info() == "list"
    ctx.close()


def test_pick_is_the_gbuffer_pixel(gpu):
    w, h = 24, 16
    sc, prims, ocam = _gen_scene(gpu, 2000, w, h)
    want = G.cached(("gen", 2000, w, h), prims, ocam, w, h)["prim"]
    ctx = gpu.RenderContext(0)
    hit = np.argwhere(want != G.MISS)
    miss = np.argwhere(want == G.MISS)
    for y, x in list(hit[:: max(1, len(hit) // 6)]) + list(miss[:2]):
        got = ctx.pick(sc, sc.camera, int(x), int(y), w, h)
        assert got == (None if want[y, x] == G.MISS else int(want[y, x])), (x, y)
    ctx.close()


def test_a_grown_n_replaces_the_buffers(gpu):
    b, want = CF.batch(gpu, "mixed"), CF.expected(gpu, "mixed")
    sc = gpu.Scene.from_prims(b["prims"])
    ctx = gpu.RenderContext(0)
    for n in (70, 700, 65, len(b["o"])):
        got = ctx.cast(sc, b["o"][:n], b["d"][:n])
        for name in ("prim", "t", "normal", "position", "albedo"):
            assert np.array_equal(got[name].view(np.uint32), want[name][:n].view(np.uint32)), (n, name)
        assert ctx.cast_info()["n"] == n
    ctx.close()


def test_device_rays_equal_host_rays(gpu):
    import torch
    b, want = CF.batch(gpu, "mixed"), CF.expected(gpu, "mixed")
    sc = gpu.Scene.from_prims(b["prims"])
    n = len(b["o"])
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 4:7] = b["o"], b["d"]
    rays[:, 3], rays[:, 7] = 123.0, np.nan  # the pads are ignored
    t = torch.from_numpy(rays).to("cuda:0")
    torch.cuda.synchronize()
    ctx = gpu.RenderContext(0)
    host = ctx.cast(sc, b["o"], b["d"])
    dev = ctx.cast(sc, t)
    assert CF.same(dev, want) == [] and CF.same(dev, host) == []
    assert ctx.cast_info()["waves_list"] == len(CF.fallback_waves(b))
    ctx.close()
    del t


def test_the_cast_disturbs_nothing(gpu):
    """cast() between streamed accumulating frames and after a gbuffer(): download(),
    accum_error(), accum_info(), a following denoise() and the G-buffer are what they are without it."""
    key, w, h, depth, spps = "scene_08", 33, 17, 8, (4,) * 4
    states = _composites(key, w, h, depth, spps)
    sc = _product_scene(gpu, key, w, h)
    b, want = CF.batch(gpu, "box"), CF.expected(gpu, "box")
    bsc = gpu.Scene.from_prims(b["prims"])
    ctx = gpu.RenderContext(0)
    ctx.gbuffer(sc, sc.camera, w, h)
    for k, spp in enumerate(spps):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
        if k in (0, 2):
            assert CF.same(ctx.cast(bsc, b["o"], b["d"]), want) == []
    o, d = _pixel_rays(gpu, sc.camera, w, h)
    assert G.same(CF.as_gbuffer(ctx.cast(sc, o, d), w, h), G.expected(gpu, key)) == []
    ctx.denoise()
    _check_state_untouched(ctx, states[3], w, h)
    _check_denoised(ctx, _expected(key, w, h, depth, spps, 3), w, h)
    assert G.same(ctx.download_gbuffer(w, h), G.expected(gpu, key)) == []
    assert ctx.gbuffer_info() == "list"
    st = ctx.sync()
    assert st["samples"] == w * h * spps[3]  # the pending render's stats are its own
    ctx.close()


def test_the_log_times_casts_and_gbuffer_passes(gpu):
    _, cam, _, w, h, sc = G.case(gpu, "spheres200")
    ctx = gpu.RenderContext(0)
    ctx.trace_log(True)
    ctx.gbuffer(sc, cam, w, h)
    ctx.cast(sc, *_pixel_rays(gpu, cam, w, h))
    ctx.cast(sc, *_pixel_rays(gpu, cam, w, h), list_walk=True)
    ms = ctx.trace_log_read(cast=True)
    assert len(ms) == 3 and all(0.0 < x < 1000.0 for x in ms)
    ctx.trace_log(True)
    assert ctx.trace_log_read(cast=True) == []
    ctx.close()


def test_refusals(gpu):
    _, cam, _, w, h, sc = G.case(gpu, "builtin0")
    o, d = _pixel_rays(gpu, cam, w, h)
    L = gpu.lib()
    ctx = gpu.RenderContext(0)
    _refused(gpu, lambda: ctx.download_hits(1), "no hits")
    _refused(gpu, ctx.cast_info, "no hits")
    rays = np.zeros((4, 8), F)
    rays[:, 6] = -1.0
    rp = rays.ctypes.data_as(C.c_void_p)
    assert L.fr_ctx_cast(ctx._h, sc._h, rp, 0, 0) == gpu.FR_EARG  # n = 0
    assert L.fr_ctx_cast(ctx._h, sc._h, rp, (1 << 27) + 1, 0) == gpu.FR_EARG  # n > 2^27
    assert L.fr_ctx_cast(ctx._h, sc._h, None, 4, 0) == gpu.FR_EARG
    assert L.fr_ctx_cast(ctx._h, None, rp, 4, 0) == gpu.FR_EARG
    assert L.fr_ctx_cast(None, sc._h, rp, 4, 0) == gpu.FR_EARG
    assert L.fr_ctx_cast(ctx._h, sc._h, rp, 4, 4) == gpu.FR_EARG  # an unknown flag
    assert L.fr_ctx_cast(ctx._h, sc._h, rp, 4, 0x80000001) == gpu.FR_EARG
    _refused(gpu, lambda: ctx.download_hits(1), "no hits")  # the refused calls enqueued nothing
    want = G.expected(gpu, "builtin0")
    got = ctx.cast(sc, o, d)
    assert L.fr_ctx_cast(ctx._h, sc._h, rp, 0, 0) == gpu.FR_EARG
    assert G.same(CF.as_gbuffer(ctx.download_hits(w * h), w, h), want) == []  # the earlier hits are still there
    assert G.same(CF.as_gbuffer(got, w, h), want) == []
    prim = np.zeros(w * h, np.uint32)
    gpu.check(L.fr_ctx_download_hits(ctx._h, prim.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, None))
    assert np.array_equal(prim.reshape(h, w), want["prim"])  # any pointer may be NULL
    gpu.check(L.fr_ctx_download_hits(ctx._h, None, None, None, None, None))
    ctx.close()
    assert L.fr_ctx_download_hits(None, None, None, None, None, None) == gpu.FR_EARG
    assert L.fr_ctx_cast_info(None, None) == gpu.FR_EARG and L.fr_ctx_gbuffer_info(None, None) == gpu.FR_EARG
