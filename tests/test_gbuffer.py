"""The first-hit feature buffers (fr_ctx_gbuffer) on the GPU against the oracle, bit for bit.

The contract (include/forma_rt.h): per pixel the pinhole primary ray's closest primitive in list
order, its own accepted root, its normal at that root, the point o + t d and the primitive's
attenuation; a miss writes id 0xFFFFFFFF, zeros and albedo 1. The pass touches nothing else of
the context.

Expected values: tests/gbuffer_ref.py (the oracle's closest-hit loop on a numpy-f32 primary
ray), which tests/test_gbuffer_host.py holds against the bits of the header the kernel compiles.
The cases (gbuffer_ref.CASES) are small images that are no multiple of the 32 x 8 workgroup, one
lattice per primitive kind, exactly axis-parallel rays, roots past 2^40 and a 200-sphere scene
(a BVH scene for the trace kernel; this pass walks its list)."""
import ctypes as C

import numpy as np
import pytest

from tests import gbuffer_ref as G
from tests.test_accum_error import SEED0, _composites, _refused
from tests.test_accumulate import _product_scene
from tests.test_denoise import _check_denoised, _check_state_untouched, _expected

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.mark.parametrize("name", list(G.CASES))
def test_bits_equal_the_oracle(gpu, name):
    _, cam, _, w, h, sc = G.case(gpu, name)
    want = G.expected(gpu, name)
    ctx = gpu.RenderContext(0)
    ctx.gbuffer(sc, cam, w, h)
    got = ctx.download_gbuffer(w, h)
    assert G.same(got, want) == []
    miss = got["prim"] == gpu.FR_GBUFFER_MISS
    assert (got["depth"][miss] == 0).all() and (got["albedo"][miss] == 1).all()
    ctx.gbuffer(sc, cam, w, h)  # again into the kept buffers
    assert G.same(ctx.download_gbuffer(w, h), want) == []
    ctx.close()


def test_a_new_size_replaces_the_buffers(gpu):
    ctx = gpu.RenderContext(0)
    for name in ("scene_08", "builtin0", "spheres200"):
        _, cam, _, w, h, sc = G.case(gpu, name)
        ctx.gbuffer(sc, cam, w, h)
        assert G.same(ctx.download_gbuffer(w, h), G.expected(gpu, name)) == []
    ctx.close()


def test_the_pass_disturbs_nothing(gpu):
    """gbuffer() between streamed accumulating frames: download(), accum_error(), accum_info()
    and a following unguided denoise() are what they are without it."""
    key, w, h, depth, spps = "scene_08", 33, 17, 8, (4,) * 4
    states = _composites(key, w, h, depth, spps)
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k, spp in enumerate(spps):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
        if k in (0, 2):
            ctx.gbuffer(sc, sc.camera, w, h)
    ctx.gbuffer(sc, sc.camera, w, h)
    ctx.denoise()
    _check_state_untouched(ctx, states[3], w, h)
    _check_denoised(ctx, _expected(key, w, h, depth, spps, 3), w, h)
    assert G.same(ctx.download_gbuffer(w, h), G.expected(gpu, key)) == []
    st = ctx.sync()
    assert st["samples"] == w * h * spps[3]  # the pending render's stats are its own
    ctx.close()


def test_refusals(gpu):
    _, cam, _, w, h, sc = G.case(gpu, "builtin0")
    ctx = gpu.RenderContext(0)
    _refused(gpu, lambda: ctx.download_gbuffer(w, h), "no G-buffer")
    _refused(gpu, lambda: ctx.gbuffer(sc, cam, 0, h), "must be > 0")
    _refused(gpu, lambda: ctx.gbuffer(sc, cam, w, 0), "must be > 0")
    _refused(gpu, lambda: ctx.download_gbuffer(w, h), "no G-buffer")  # the refused calls enqueued nothing
    ctx.gbuffer(sc, cam, w, h)
    _refused(gpu, lambda: ctx.gbuffer(sc, cam, 0, 0), "must be > 0")
    assert G.same(ctx.download_gbuffer(w, h), G.expected(gpu, "builtin0")) == []  # the earlier one is still there
    prim = np.zeros((h, w), np.uint32)
    gpu.check(gpu.lib().fr_ctx_download_gbuffer(ctx._h, prim.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, None))
    assert np.array_equal(prim, G.expected(gpu, "builtin0")["prim"])  # any pointer may be NULL
    ctx.close()
    assert gpu.lib().fr_ctx_gbuffer(None, None, None, 1, 1) == gpu.FR_EARG
    assert gpu.lib().fr_ctx_download_gbuffer(None, None, None, None, None, None) == gpu.FR_EARG
