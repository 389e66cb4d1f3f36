"""Occlusion queries (fr_ctx_occluded) and ranged casts (fr_ctx_cast with FR_CAST_TMAX) on the GPU
against the oracle-based reference, bit for bit.

The contract (include/forma_rt.h): a ray is occluded iff some primitive of the list passes its own
test within (0.001, t_max), which equals "the closest-hit loop started at closest = t_max finds a
winner"; the ranged cast returns that winner as fr_ctx_cast returns a hit. A t_max of NaN, an
infinity, 0 or a negative gives whatever the loop's comparisons give. A scene that has a tree is
walked through it; a wave of 64 rays holding a ray the tree's cull is not conservative for walks
the list. Neither call touches anything else of the context.

Expected values: tests/occlude_fixtures.py (every primitive's own root from the oracle on the
one-primitive list, then the list loop in Python), which tests/test_occlude_host.py holds against
the bits of the header the kernels compile."""
import ctypes as C

import numpy as np
import pytest

from tests import cast_fixtures as CF
from tests import gbuffer_ref as G
from tests import occlude_fixtures as OF
from tests import ray_edge_fixtures as X
from tests.test_accum_error import SEED0, _composites, _refused
from tests.test_accumulate import _product_scene
from tests.test_cast import _gen_scene, _pixel_rays, _waves
from tests.test_denoise import _check_state_untouched

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("prim", "t", "normal", "position", "albedo")


def _same(got, want, sel=slice(None)):
    return [name for name in NAMES if not np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                                                         np.ascontiguousarray(want[name][sel]).view(np.uint32))]


@pytest.mark.parametrize("kind", X.KINDS)
def test_lattice_batches_equal_the_reference(gpu, kind):
    b, t_max, want = OF.lattice(gpu, kind)
    sc = gpu.Scene.from_prims(b["prims"])
    n = len(t_max)
    has_tree = kind != "plane"  # 54 planes exceed kBvhMaxPlanes: no tree
    ctx = gpu.RenderContext(0)
    for list_walk in (False, True):
        got = ctx.occluded(sc, b["o"], b["d"], t_max=t_max, list_walk=list_walk)
        assert got.dtype == bool and got.shape == (n,)
        assert np.array_equal(got, want["occluded"]), np.nonzero(got != want["occluded"])[0][:8]
        info = ctx.occluded_info()
        assert info["n"] == n and info["waves_tree"] + info["waves_list"] == _waves(n)
        assert info["occluded"] == int(want["occluded"].sum())
        if has_tree and not list_walk:
            assert info["tree"] == 1 and info["waves_tree"] > 0 and info["waves_list"] == len(CF.fallback_waves(b))
        else:
            assert info["tree"] == 0 and info["waves_tree"] == 0 and info["waves_list"] == _waves(n)
        hits = ctx.cast(sc, b["o"], b["d"], t_max=t_max, list_walk=list_walk)
        assert _same(hits, want) == []
        ci = ctx.cast_info()
        assert ci["n"] == n and ci["tree"] == (1 if has_tree and not list_walk else 0)
        if has_tree and not list_walk:
            assert ci["waves_list"] == len(CF.fallback_waves(b))
    # a scalar t_max is every ray's; FLT_MAX is the plain cast, and occluded iff hit
    plain = CF.expected(gpu, kind)
    assert np.array_equal(ctx.occluded(sc, b["o"], b["d"]), plain["prim"] != CF.MISS)
    assert np.array_equal(ctx.occluded(sc, b["o"], b["d"], t_max=OF.FLT_MAX), plain["prim"] != CF.MISS)
    assert CF.same(ctx.cast(sc, b["o"], b["d"], t_max=OF.FLT_MAX), plain) == []
    ctx.close()


@pytest.mark.parametrize("kind", ["mixed", "plane"])
def test_without_the_flag_the_pad_is_ignored(gpu, kind):
    """fr_ctx_cast and fr_ctx_occluded without FR_CAST_TMAX on rays whose pads hold NaN and 0."""
    b, want = CF.batch(gpu, kind), CF.expected(gpu, kind)
    sc = gpu.Scene.from_prims(b["prims"])
    n = len(b["o"])
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 4:7] = b["o"], b["d"]
    rays[0::2, 7], rays[1::2, 7], rays[:, 3] = np.nan, 0.0, np.nan
    rp = rays.ctypes.data_as(C.c_void_p)
    ctx = gpu.RenderContext(0)
    for flags in (0, gpu.FR_CAST_LIST):
        gpu.check(gpu.lib().fr_ctx_cast(ctx._h, sc._h, rp, n, flags))
        assert CF.same(ctx.download_hits(n), want) == []
        gpu.check(gpu.lib().fr_ctx_occluded(ctx._h, sc._h, rp, n, flags, None))
        assert np.array_equal(ctx.download_occluded(n), want["prim"] != CF.MISS)
    # with the flag the same words are the ranges: NaN and 0 occlude nothing and hit nothing
    gpu.check(gpu.lib().fr_ctx_occluded(ctx._h, sc._h, rp, n, gpu.FR_CAST_TMAX, None))
    assert not ctx.download_occluded(n).any() and ctx.occluded_info()["occluded"] == 0
    gpu.check(gpu.lib().fr_ctx_cast(ctx._h, sc._h, rp, n, gpu.FR_CAST_TMAX))
    assert (ctx.download_hits(n)["prim"] == CF.MISS).all()
    ctx.close()


def test_generator_spheres_and_tails(gpu):
    """2,000 spheres: a tree about ten levels deep, so the per-lane stack is pushed and popped and
    lanes leave their wave's walk early; batches of 1, 63, 64, 65 and 321 rays for the last wave."""
    w, h = 24, 16
    sc, _, _ = _gen_scene(gpu, 2000, w, h)
    prims, o, d, t_max, want = OF.spheres(gpu, 2000, w, h)
    n = len(o)
    ctx = gpu.RenderContext(0)
    for list_walk in (False, True):
        assert np.array_equal(ctx.occluded(sc, o, d, t_max=t_max, list_walk=list_walk), want["occluded"])
        tree = 0 if list_walk else 1
        assert ctx.occluded_info() == {"n": n, "tree": tree, "waves_tree": _waves(n) * tree, "waves_list": _waves(n) * (1 - tree),
                                       "occluded": int(want["occluded"].sum())}
        assert _same(ctx.cast(sc, o, d, t_max=t_max, list_walk=list_walk), want) == []
    for k in (1, 63, 64, 65, 321):
        sel = slice(100, 100 + k)
        got = ctx.occluded(sc, o[sel], d[sel], t_max=t_max[sel])
        assert got.shape == (k,) and np.array_equal(got, want["occluded"][sel]), k
        assert ctx.occluded_info() == {"n": k, "tree": 1, "waves_tree": _waves(k), "waves_list": 0,
                                       "occluded": int(want["occluded"][sel].sum())}
        assert _same(ctx.cast(sc, o[sel], d[sel], t_max=t_max[sel]), want, sel) == [], k
        assert ctx.cast_info() == {"n": k, "tree": 1, "waves_tree": _waves(k), "waves_list": 0}
    ctx.close()


class _DeviceWords:
    """n 16-byte words at a device address, for torch.as_tensor."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n, 4), "typestr": "<f4", "data": (ptr, False), "version": 2}


def test_device_paths(gpu):
    import torch
    b, t_max, want = OF.lattice(gpu, "mixed")
    sc = gpu.Scene.from_prims(b["prims"])
    n = len(t_max)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = b["o"], b["d"], t_max
    rays[:, 3] = np.nan  # pad0 stays ignored
    t = torch.from_numpy(rays).to("cuda:0")
    torch.cuda.synchronize()
    ctx = gpu.RenderContext(0)
    # a device ray tensor with t_max in column 7
    assert np.array_equal(ctx.occluded(sc, t, t_max=True), want["occluded"])
    assert ctx.occluded_info()["waves_list"] == len(CF.fallback_waves(b))
    hits = ctx.cast(sc, t, t_max=True)
    assert _same(hits, want) == []
    # ... and without the flag column 7 is a pad
    assert CF.same(ctx.cast(sc, t), CF.expected(gpu, "mixed")) == []
    # out= a device tensor: filled on the device, nothing of the context's own bytes involved
    out = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    back = ctx.occluded(sc, t, t_max=True, out=out)
    assert back is out
    assert np.array_equal(out.cpu().numpy(), want["occluded"].astype(np.uint8))
    assert np.array_equal(ctx.download_occluded(n), want["occluded"])  # read from the caller's buffer
    out2 = torch.zeros((n,), dtype=torch.uint8, device="cuda:0")
    ctx.occluded(sc, b["o"], b["d"], t_max=t_max, out=out2, list_walk=True)  # host rays, device answers
    assert np.array_equal(out2.cpu().numpy(), want["occluded"].astype(np.uint8))
    with pytest.raises(gpu.ForMaError):
        ctx.occluded(sc, t, t_max=True, out=torch.zeros((n + 1,), dtype=torch.uint8, device="cuda:0"))
    # the last cast's hits, left on the device
    hits = ctx.cast(sc, t, t_max=True)
    g0, g1, alb, m = ctx.hit_buffers()
    assert m == n and g0 and g1 and alb
    w0, w1, wa = (torch.as_tensor(_DeviceWords(p, n), device="cuda:0").cpu().numpy() for p in (g0, g1, alb))
    assert np.array_equal(w0[:, 3].view(np.uint32), hits["t"].view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(w0[:, :3]).view(np.uint32), hits["normal"].view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(w1[:, :3]).view(np.uint32), hits["position"].view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(w1[:, 3]).view(np.uint32), hits["prim"])
    assert np.array_equal(np.ascontiguousarray(wa[:, :3]).view(np.uint32), hits["albedo"].view(np.uint32))
    assert _same(hits, want) == []
    ctx.close()
    del t, out, out2


def test_visible_is_not_occluded_between_two_points(gpu):
    w, h = 24, 16
    sc, _, _ = _gen_scene(gpu, 2000, w, h)
    prims, o, d, _, _ = OF.spheres(gpu, 2000, w, h)
    plain = CF.gen_batch(gpu, 2000, w, h)[3]
    hit = np.nonzero(plain["prim"][:w * h] != CF.MISS)[0][:6]
    a = o[hit]
    p = plain["position"][hit]
    # from the camera to a point past the first surface (hidden), to a point before it (seen)
    with np.errstate(all="ignore"):
        past = (a + (F(1.5) * (p - a)).astype(F)).astype(F)
        before = (a + (F(0.5) * (p - a)).astype(F)).astype(F)
    aa, bb = np.concatenate([a, a]), np.concatenate([past, before])
    ctx = gpu.RenderContext(0)
    vis = ctx.visible(sc, aa, bb)
    assert np.array_equal(vis, ~ctx.occluded(sc, aa, (bb - aa).astype(F), t_max=1.0))
    want = OF.ranged(prims, aa, (bb - aa).astype(F), np.ones(len(aa), F))["occluded"]
    assert np.array_equal(vis, ~want) and not vis[:len(a)].any() and vis[len(a):].all()
    ctx.close()


def test_the_query_disturbs_nothing(gpu):
    """occluded() between streamed accumulating frames, after a gbuffer() and a cast(): download(),
    accum_error(), accum_info(), the G-buffer and the cast's hits and info are what they are
    without it."""
    key, w, h, depth, spps = "scene_08", 33, 17, 8, (4,) * 4
    states = _composites(key, w, h, depth, spps)
    sc = _product_scene(gpu, key, w, h)
    b, t_max, want = OF.lattice(gpu, "box")
    plain = CF.expected(gpu, "box")
    bsc = gpu.Scene.from_prims(b["prims"])
    ctx = gpu.RenderContext(0)
    ctx.gbuffer(sc, sc.camera, w, h)
    assert CF.same(ctx.cast(bsc, b["o"], b["d"]), plain) == []
    cast_info = ctx.cast_info()
    for k, spp in enumerate(spps):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
        if k in (0, 2):
            assert np.array_equal(ctx.occluded(bsc, b["o"], b["d"], t_max=t_max), want["occluded"])
    o, d = _pixel_rays(gpu, sc.camera, w, h)
    occ = ctx.occluded(sc, o, d)  # another scene, fewer rays
    assert np.array_equal(occ, G.expected(gpu, key)["prim"].reshape(-1) != G.MISS)
    _check_state_untouched(ctx, states[3], w, h)
    assert G.same(ctx.download_gbuffer(w, h), G.expected(gpu, key)) == []
    assert CF.same(ctx.download_hits(len(b["o"])), plain) == [] and ctx.cast_info() == cast_info
    st = ctx.sync()
    assert st["samples"] == w * h * spps[3]  # the pending render's stats are its own
    ctx.close()


def test_the_log_times_occlusion_kernels(gpu):
    _, cam, _, w, h, sc = G.case(gpu, "spheres200")
    o, d = _pixel_rays(gpu, cam, w, h)
    ctx = gpu.RenderContext(0)
    ctx.trace_log(True)
    ctx.occluded(sc, o, d)
    ctx.cast(sc, o, d, t_max=5.0)
    ctx.occluded(sc, o, d, t_max=5.0, list_walk=True)
    ms = ctx.trace_log_read(cast=True)
    assert len(ms) == 3 and all(0.0 < x < 1000.0 for x in ms)
    ctx.close()


def test_refusals(gpu):
    import torch
    _, cam, _, w, h, sc = G.case(gpu, "builtin0")
    o, d = _pixel_rays(gpu, cam, w, h)
    want = G.expected(gpu, "builtin0")["prim"].reshape(-1) != G.MISS
    L = gpu.lib()
    ctx = gpu.RenderContext(0)
    _refused(gpu, lambda: ctx.download_occluded(1), "no query")
    _refused(gpu, ctx.occluded_info, "no query")
    _refused(gpu, ctx.hit_buffers, "no hits")
    rays = np.zeros((4, 8), F)
    rays[:, 6] = -1.0
    rp = rays.ctypes.data_as(C.c_void_p)
    dev = torch.zeros((4,), dtype=torch.uint8, device="cuda:0")
    dp = C.c_void_p(dev.data_ptr())
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, 0, 0, None) == gpu.FR_EARG  # n = 0
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, (1 << 27) + 1, 0, None) == gpu.FR_EARG  # n > 2^27
    assert L.fr_ctx_occluded(ctx._h, sc._h, None, 4, 0, None) == gpu.FR_EARG
    assert L.fr_ctx_occluded(ctx._h, None, rp, 4, 0, None) == gpu.FR_EARG
    assert L.fr_ctx_occluded(None, sc._h, rp, 4, 0, None) == gpu.FR_EARG
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, 4, 32, None) == gpu.FR_EARG  # an unknown flag
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, 4, 4, None) == gpu.FR_EARG
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, 4, 0x80000001, None) == gpu.FR_EARG
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, 4, gpu.FR_CAST_OUT_DEVICE, None) == gpu.FR_EARG  # a NULL device out
    assert L.fr_ctx_cast(ctx._h, sc._h, rp, 4, gpu.FR_CAST_OUT_DEVICE) == gpu.FR_EARG  # not a flag of the cast
    assert L.fr_ctx_cast(ctx._h, sc._h, rp, 4, 32) == gpu.FR_EARG
    _refused(gpu, lambda: ctx.download_occluded(1), "no query")  # the refused calls enqueued nothing
    _refused(gpu, ctx.occluded_info, "no query")
    _refused(gpu, lambda: ctx.download_hits(1), "no hits")
    _refused(gpu, ctx.hit_buffers, "no hits")
    got = ctx.occluded(sc, o, d)
    assert np.array_equal(got, want)
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, 0, 0, None) == gpu.FR_EARG
    assert L.fr_ctx_occluded(ctx._h, sc._h, rp, 4, gpu.FR_CAST_OUT_DEVICE, None) == gpu.FR_EARG
    assert np.array_equal(ctx.download_occluded(w * h), want)  # the earlier answers are still there
    assert ctx.occluded_info()["occluded"] == int(want.sum())
    _refused(gpu, ctx.hit_buffers, "no hits")  # a query is not a cast
    gpu.check(L.fr_ctx_download_occluded(ctx._h, None))  # NULL: only waits
    gpu.check(L.fr_ctx_occluded(ctx._h, sc._h, rp, 4, gpu.FR_CAST_OUT_DEVICE, dp))  # the valid form of the refused call
    gpu.check(L.fr_ctx_download_occluded(ctx._h, None))
    assert ctx.occluded_info()["n"] == 4
    ctx.cast(sc, o, d)
    gpu.check(L.fr_ctx_hit_buffers(ctx._h, None, None, None, None))  # any pointer may be NULL
    assert ctx.hit_buffers()[3] == w * h
    ctx.close()
    del dev
    assert L.fr_ctx_download_occluded(None, None) == gpu.FR_EARG and L.fr_ctx_occluded_info(None, None) == gpu.FR_EARG
    assert L.fr_ctx_hit_buffers(None, None, None, None, None) == gpu.FR_EARG
