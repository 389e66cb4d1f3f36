"""The variance-guided denoise of a progressive accumulation (fr_ctx_denoise) on the GPU against
the oracle, bit for bit.

The contract (include/forma_rt.h): fr_ctx_denoise filters the live accumulation's mean with an
a-trous wavelet filter steered by the per-pixel variance of the mean that A, Q and the counts
give, in f32 operations of a fixed order; fr_ctx_download_denoised returns the filtered mean, its
u8 image and the variance map the filter steered by.

Expected values: the oracle's frames composited by tests/accum_error_ref.py's ErrorComposite
(tests/adaptive_ref.py's AdaptiveComposite for the tiled case), as tests/test_accum_error.py
builds them, then passed through tests/denoise_ref.py, which tests/test_denoise_host.py holds
against the bits of the header the kernels compile. The mean's bits, the variance's bits and the
u8 image are compared exactly.

Images are 33x17 or 32x24 as in test_accumulate.py (partial 8x8 tiles and a partial strip for
prep, partial 32x8 workgroups for the levels), and 70x21 for the seams: more than two 32x8
workgroup tiles plus a remainder in both directions."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import accum_error_ref as R
from tests import adaptive_ref as AR
from tests import denoise_ref as D
from tests.test_accum_error import SEED0, T, _composites, _refused
from tests.test_accumulate import _frame_sum, _oracle_frame, _product_scene, _same_bits, _to_u8

pytestmark = pytest.mark.gpu
F = np.float32


@functools.lru_cache(maxsize=None)
def _expected(key, w, h, depth, spps, frame, levels=D.LEVELS, k=D.K):
    """(mean, u8, var) of a denoise after frame index `frame` of the accumulation, computed once."""
    st = _composites(key, w, h, depth, spps)[frame]
    out = D.denoise(st["a"], st["q"], st["n"], st["frames"], levels, k)
    for x in out:
        x.setflags(write=False)
    return out


def _check_denoised(ctx, want, w, h):
    mean, u8, var = ctx.download_denoised(w, h, want_var=True)
    wm, wu, wv = want
    assert _same_bits(mean, wm), int(np.count_nonzero(mean.view(np.uint32) != wm.view(np.uint32)))
    assert _same_bits(var, wv), int(np.count_nonzero(var.view(np.uint32) != wv.view(np.uint32)))
    assert np.array_equal(u8, wu)
    assert not np.isnan(mean).any() and not np.isnan(var).any()  # (every pixel of these scenes is valid)
    mean2, u82 = ctx.download_denoised(w, h)
    assert _same_bits(mean2, wm) and np.array_equal(u82, wu)


def _check_state_untouched(ctx, state, w, h):
    """download(), accum_error() and accum_info() are what they are without a denoise."""
    ctx.sync()
    mean, u8 = ctx.download(w, h)
    assert _same_bits(mean, state["mean"]) and np.array_equal(u8, state["u8"])
    assert ctx.accum_info() == (state["frames"], state["n"])
    got, rel = ctx.accum_error(T, want_map=True)
    assert _same_bits(rel, state["rel"])
    assert (got["frames"], got["samples"], got["pixels"]) == (state["frames"], state["n"], w * h)
    assert got["converged"] == int(np.count_nonzero(state["rel"] <= F(T)))


def _frames(gpu, ctx, sc, w, h, depth, spps, first=0):
    for k in range(first, len(spps)):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spps[k], depth, SEED0 + k, accumulate="error"))


def _run(gpu, key, w, h, depth, spps, after=None):
    """Denoise at the defaults after the frames of index `after` (default: the last)."""
    spps = tuple(spps)
    after = (len(spps) - 1,) if after is None else after
    states = _composites(key, w, h, depth, spps)
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k, spp in enumerate(spps):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
        if k in after:
            ctx.denoise()
            _check_denoised(ctx, _expected(key, w, h, depth, spps, k), w, h)
            _check_state_untouched(ctx, states[k], w, h)
            _check_denoised(ctx, _expected(key, w, h, depth, spps, k), w, h)  # and still there after them
    ctx.close()
    return states


def test_ordinary_frames(gpu):
    states = _run(gpu, "scene_08", 33, 17, 8, (4,) * 4, after=(1, 2, 3))
    wm, _, wv = _expected("scene_08", 33, 17, 8, (4,) * 4, 3)
    assert not _same_bits(wm, states[3]["mean"]) and float(wv.max()) > 0  # the filter moved the picture


def test_every_step_and_other_k(gpu):
    key, w, h, depth, spps = "scene_08", 33, 17, 8, (4,) * 4
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    _frames(gpu, ctx, sc, w, h, depth, spps)
    seen = []
    # at levels 6 the last step is 32, as wide as the image: almost every tap is outside
    for levels, k in ((1, 4.0), (2, 4.0), (3, 4.0), (6, 4.0), (4, 0.5), (4, 64.0), (6, 0.5), (1, 64.0)):
        ctx.denoise(levels, k)
        want = _expected(key, w, h, depth, spps, 3, levels, k)
        _check_denoised(ctx, want, w, h)
        seen.append(want[0].tobytes())
    assert len(set(seen)) == len(seen)  # every setting is another picture
    ctx.close()


def test_tile_seams(gpu):
    """70x21: three 32-pixel workgroup columns (the last 6 wide) and three 8-row workgroup rows
    (the last 5 high), so taps cross every kind of workgroup seam and the partial ones."""
    _run(gpu, "scene_08", 70, 21, 8, (2,) * 3)


def test_colour_records_at_update_shape(gpu):
    _run(gpu, "builtin0", 32, 24, 50, (1,) * 6)


def test_bvh_scene(gpu):
    _run(gpu, "cubes100", 33, 17, 8, (16,) * 3)


def test_tiled_accumulation(gpu):
    """Two uniform frames, adapt, two adaptive frames, denoise: prep reads each tile's n_t and K_t."""
    key, w, h, depth, spp, thr, mins = AR.CASES["scene08_16"]
    comp = AR.AdaptiveComposite(w, h)
    mask = None
    for k in range(4):
        if k == 2:
            mask, summary = comp.select(thr, mins)
        omean, _, _, _ = _oracle_frame(key, w, h, spp, depth, AR.SEED0 + k)
        comp.add(_frame_sum(omean, spp), spp, mask)
    assert 0 < int(mask.sum()) < mask.size  # both active and inactive tiles
    assert len(np.unique(comp.n)) == 2 and len(np.unique(comp.k)) == 2
    want = D.denoise(comp.a, comp.q, comp.pixels(comp.n), comp.pixels(comp.k))
    uniform = D.denoise(comp.a, comp.q, int(comp.n.max()), int(comp.k.max()))
    assert not _same_bits(want[0], uniform[0])  # the tiles' own counts show in the result
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k in range(4):
        if k == 2:
            info = ctx.adapt(thr, mins)
            assert info["active_tiles"] == summary["active_tiles"] == int(mask.sum())
            assert 0 < info["active_tiles"] < info["tiles"]
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, AR.SEED0 + k,
                                                  accumulate="adaptive" if k >= 2 else "error"))
    ctx.denoise()
    _check_denoised(ctx, want, w, h)
    n, kk = ctx.download_counts()
    assert np.array_equal(n, comp.pixels(comp.n)) and np.array_equal(kk, comp.pixels(comp.k))
    ctx.sync()
    mean, u8 = ctx.download(w, h)
    assert _same_bits(mean, comp.mean) and np.array_equal(u8, _to_u8(comp.mean))
    ctx.close()


def test_streaming(gpu):
    """Frames, a denoise and another frame enqueued with one sync at the end: the denoised image
    is the state the call saw, the later frame's outputs are the composite's."""
    key, w, h, depth, spps = "scene_08", 33, 17, 8, (4,) * 4
    states = _composites(key, w, h, depth, spps)
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k in range(3):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spps[k], depth, SEED0 + k, accumulate="error"))
    ctx.denoise()
    ctx.render(sc, sc.camera, gpu.make_params(w, h, spps[3], depth, SEED0 + 3, accumulate="error"))
    ctx.sync()
    _check_denoised(ctx, _expected(key, w, h, depth, spps, 2), w, h)
    _check_state_untouched(ctx, states[3], w, h)
    dm, du = ctx.denoised_buffers()
    fm, fu = ctx.device_buffers()
    assert dm and du and len({dm, du, fm, fu}) == 4  # buffers of their own
    ctx.close()


def test_refusals(gpu):
    w, h = 32, 24
    sc = _product_scene(gpu, "builtin0", w, h)
    ctx = gpu.RenderContext(0)
    P = lambda k, mode, **kw: gpu.make_params(w, h, 2, 8, 5 + k, accumulate=mode, **kw)  # noqa: E731
    _refused(gpu, lambda: ctx.denoise(), "no live accumulation")
    _refused(gpu, lambda: ctx.download_denoised(w, h), "no denoised image")
    _refused(gpu, lambda: ctx.denoised_buffers(), "no denoised image")
    for k in range(2):
        ctx.render(sc, sc.camera, P(k, True))
    _refused(gpu, lambda: ctx.denoise(), "carries no Q")
    ctx.render(sc, sc.camera, P(2, "error"))
    _refused(gpu, lambda: ctx.denoise(), "needs two")
    ctx.render(sc, sc.camera, P(3, "error"))
    for levels in (0, 7):
        _refused(gpu, lambda: ctx.denoise(levels, 4.0), "levels")
    for k in (0.0, -1.0, float("nan"), float("inf"), 2048.0):
        _refused(gpu, lambda: ctx.denoise(4, k), "must be finite, > 0 and <= 1024")
    _refused(gpu, lambda: ctx.download_denoised(w, h), "no denoised image")  # the refused calls enqueued nothing
    ctx.denoise(1, 1024.0)  # the ends of both ranges are in
    ctx.denoise(6, 2.0 ** -20)
    mean, u8 = ctx.download_denoised(w, h)
    assert not np.isnan(mean).any() and np.array_equal(u8, _to_u8(mean))
    ctx.accum_reset()
    _refused(gpu, lambda: ctx.denoise(), "no live accumulation")
    for k in range(2):  # a shard of an image: the taps would cross to rows that live elsewhere
        ctx.render(sc, sc.camera, P(4 + k, "error", shard_index=1, shard_count=2))
    _refused(gpu, lambda: ctx.denoise(), "shard_count 2")
    assert ctx.accum_error(T)["frames"] == 2  # (the estimate itself has no such limit)
    ctx.close()
    rc = gpu.lib().fr_ctx_denoise(None, 4, C.c_float(4.0))
    assert rc == gpu.FR_EARG


def test_a_new_size_replaces_the_buffers(gpu):
    key, depth, spps = "scene_08", 8, (4,) * 4
    ctx = gpu.RenderContext(0)
    for w, h in ((33, 17), (70, 21)):
        spp_list = spps if (w, h) == (33, 17) else (2,) * 3
        sc = _product_scene(gpu, key, w, h)
        _frames(gpu, ctx, sc, w, h, depth, spp_list)
        ctx.denoise()
        _check_denoised(ctx, _expected(key, w, h, depth, spp_list, len(spp_list) - 1), w, h)
    ctx.close()


def test_update_shows_the_denoised_picture(gpu):
    w, h = 32, 24
    m = gpu.create_model(w, h)
    ocam = O.camera_new(w, h)
    d = (C.c_float * 3)()
    comp = R.ErrorComposite()
    for frame in range(4):
        pix = gpu.update(m, 0, 0.1, accumulate="error", denoise=True).copy()
        gpu.check(gpu.lib().fr_update_delta(0, 0.1, d))
        O.camera_orbit(ocam, list(d))
        seed = m.seed ^ (0x9E3779B97F4A7C15 * (frame + 1) & 0xFFFFFFFFFFFFFFFF)
        omean, _, _, _ = O.render(S.BUILTIN[0](), ocam, w, h, 1, 50, seed=seed)
        mean = comp.add(_frame_sum(omean, 1), 1)
        plain = _to_u8(mean)
        if frame == 0:
            assert np.array_equal(pix.reshape(h, w, 3), plain)
        else:
            _, want_u8, _ = D.denoise(comp.a, comp.q, comp.n, comp.frames)
            assert np.array_equal(pix.reshape(h, w, 3), want_u8), frame
            assert not np.array_equal(want_u8, plain)
        assert m.ctx.accum_info() == (frame + 1, frame + 1)
        assert np.array_equal(m.ctx.download(w, h)[1], plain)  # the frame's own u8 stays the plain one
    pix = gpu.update(m, 0b001000, 0.1, accumulate="error", denoise=True)  # a key press: a new accumulation
    gpu.check(gpu.lib().fr_update_delta(0b001000, 0.1, d))
    O.camera_orbit(ocam, list(d))
    seed = m.seed ^ (0x9E3779B97F4A7C15 * 5 & 0xFFFFFFFFFFFFFFFF)
    _, ou8, _, _ = O.render(S.BUILTIN[0](), ocam, w, h, 1, 50, seed=seed)
    assert np.array_equal(pix.reshape(h, w, 3), ou8) and m.ctx.accum_info() == (1, 1)
    assert pix.ctypes.data == m._pinned.u8.ctypes.data  # the same page-locked frame
    m.close()
