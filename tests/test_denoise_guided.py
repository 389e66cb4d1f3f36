"""The feature-guided denoise of a progressive accumulation (fr_ctx_denoise_guided) on the GPU
against the oracle, bit for bit.

The contract (include/forma_rt.h): fr_ctx_denoise's a-trous filter with every non-centre tap's
weight extended by the G-buffer of the same view (fr_ctx_gbuffer): taps between a hit and a miss
are skipped, taps between hits are weighted by the normals' clamped dot product to the power
2^normal_pow2 and by the tap's distance from the centre's tangent plane relative to sigma_z times
the depth; with demodulate the colour is filtered divided by the first hit's albedo. The results
land in fr_ctx_denoise's buffers.

Expected values: the oracle's frames composited as tests/test_denoise.py composites them, the
oracle's first hits (tests/gbuffer_ref.py), passed through tests/denoise_guided_ref.py, which
tests/test_denoise_guided_host.py holds against the bits of the header the kernels compile. The
mean's bits, the variance's bits and the u8 image are compared exactly.

normal_pow2 = 0 with a large sigma_z and demodulate = 0 is NOT required to equal the unguided
filter's bits (tests/test_denoise_guided_host.py says why); no test here asserts that."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import accum_error_ref as R
from tests import adaptive_ref as AR
from tests import denoise_guided_ref as DG
from tests import denoise_ref as D
from tests import gbuffer_ref as G
from tests import nonfinite_fixtures as N
from tests.test_accum_error import SEED0, _composites, _refused
from tests.test_accumulate import _frame_sum, _oracle_frame, _oracle_scene, _product_scene, _same_bits, _to_u8
from tests.test_denoise import _check_denoised, _check_state_untouched, _expected
from tests.test_denoise_guided_host import OTHER

pytestmark = pytest.mark.gpu
F = np.float32
SCENES = {"scene_08": (33, 17, 8, (4,) * 4), "builtin0": (32, 24, 50, (1,) * 6)}


def _features(key, w, h):
    prims, ocam = _oracle_scene(key, w, h)
    return G.cached((key, w, h), prims, ocam, w, h)


@functools.lru_cache(maxsize=None)
def _guided(key, frame, levels=D.LEVELS, k=D.K, other=False):
    """(mean, u8, var) of a guided denoise after frame index `frame` of SCENES[key], computed once."""
    w, h, depth, spps = SCENES[key]
    st = _composites(key, w, h, depth, spps)[frame]
    out = DG.denoise(st["a"], st["q"], st["n"], st["frames"], _features(key, w, h), levels, k, **(OTHER if other else {}))
    for x in out:
        x.setflags(write=False)
    return out


def _accumulation(gpu, key, frames=None):
    w, h, depth, spps = SCENES[key]
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k, spp in enumerate(spps[:frames]):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
    return ctx, sc, w, h


@pytest.mark.parametrize("key", list(SCENES))
def test_levels_and_guides(gpu, key):
    ctx, sc, w, h = _accumulation(gpu, key)
    last = len(SCENES[key][3]) - 1
    ctx.gbuffer(sc, sc.camera, w, h)
    seen = []
    for levels in (1, 4, 6):
        for other in (False, True):
            ctx.denoise(levels, guided=True, **(OTHER if other else {}))
            want = _guided(key, last, levels, D.K, other)
            _check_denoised(ctx, want, w, h)
            seen.append(want[0].tobytes())
    assert len(set(seen)) == len(seen)  # every setting is another picture
    unguided = _expected(key, w, h, SCENES[key][2], SCENES[key][3], last)
    assert not _same_bits(_guided(key, last)[0], unguided[0])
    _check_state_untouched(ctx, _composites(key, w, h, *SCENES[key][2:])[last], w, h)
    ctx.close()


def test_guided_then_unguided_share_the_buffers(gpu):
    key = "scene_08"
    ctx, sc, w, h = _accumulation(gpu, key)
    ctx.gbuffer(sc, sc.camera, w, h)
    ctx.denoise(guided=True)
    dm, du = ctx.denoised_buffers()
    _check_denoised(ctx, _guided(key, 3), w, h)
    ctx.denoise()
    _check_denoised(ctx, _expected(key, w, h, *SCENES[key][2:], 3), w, h)
    assert ctx.denoised_buffers() == (dm, du)
    ctx.denoise(guided=True)
    _check_denoised(ctx, _guided(key, 3), w, h)
    ctx.close()


def test_streaming(gpu):
    """Frames, the G-buffer, a guided denoise and another frame enqueued with one sync at the
    end: the denoised image is the state the call saw, the later frame's outputs the composite's."""
    key = "scene_08"
    w, h, depth, spps = SCENES[key]
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k in range(3):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spps[k], depth, SEED0 + k, accumulate="error"))
        if k == 0:
            ctx.gbuffer(sc, sc.camera, w, h)
    ctx.denoise(guided=True)
    ctx.render(sc, sc.camera, gpu.make_params(w, h, spps[3], depth, SEED0 + 3, accumulate="error"))
    ctx.sync()
    _check_denoised(ctx, _guided(key, 2), w, h)
    _check_state_untouched(ctx, _composites(key, w, h, depth, spps)[3], w, h)
    ctx.close()


def test_tiled_accumulation(gpu):
    """Two uniform frames, adapt, two adaptive frames, guided denoise: prep reads each tile's n_t
    and K_t beside the features."""
    key, w, h, depth, spp, thr, mins = AR.CASES["scene08_16"]
    comp = AR.AdaptiveComposite(w, h)
    mask = None
    for k in range(4):
        if k == 2:
            mask, summary = comp.select(thr, mins)
        omean, _, _, _ = _oracle_frame(key, w, h, spp, depth, AR.SEED0 + k)
        comp.add(_frame_sum(omean, spp), spp, mask)
    assert 0 < int(mask.sum()) < mask.size and len(np.unique(comp.n)) == 2
    g = _features(key, w, h)
    want = DG.denoise(comp.a, comp.q, comp.pixels(comp.n), comp.pixels(comp.k), g)
    uniform = DG.denoise(comp.a, comp.q, int(comp.n.max()), int(comp.k.max()), g)
    assert not _same_bits(want[0], uniform[0])  # the tiles' own counts show in the result
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    ctx.gbuffer(sc, sc.camera, w, h)
    for k in range(4):
        if k == 2:
            assert ctx.adapt(thr, mins)["active_tiles"] == summary["active_tiles"]
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, AR.SEED0 + k,
                                                  accumulate="adaptive" if k >= 2 else "error"))
    ctx.denoise(guided=True)
    _check_denoised(ctx, want, w, h)
    ctx.close()


def test_nonfinite_pixels(gpu):
    """The NaN colour on the mixed lattice (tests/nonfinite_fixtures.py): invalid pixels keep
    prep's bits, the map is free of the sign bit and of NaN, no valid pixel is NaN; the NaN
    albedo demodulates as 1."""
    case = N.SMALL["nan"]
    prims = N.prims(case)
    cam, ocam = N.cameras(gpu)
    g = G.cached(("nonfinite", case), prims, ocam, N.W, N.H)
    assert np.isnan(g["albedo"]).any()
    st = N.states(case)[3]
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    for k in range(4):
        ctx.render(sc, cam, gpu.make_params(N.W, N.H, case.spps[k], case.depth, N.seed_of(case, k), accumulate="error"))
    ctx.gbuffer(sc, cam, N.W, N.H)
    got = ctx.download_gbuffer(N.W, N.H)
    assert G.same({**got, "albedo": g["albedo"]}, g) == [] and N.same_bits_nan(got["albedo"], g["albedo"])
    for levels in N.LEVELS:
        for guide in ({}, OTHER):
            with np.errstate(all="ignore"):
                want_mean, want_u8, want_var = DG.denoise(st["a"], st["q"], st["n"], st["frames"], g, levels, **guide)
                c0, v0, valid = DG.prep(st["a"], st["q"], st["n"], st["frames"], g, guide.get("demodulate", True))
            assert (~valid).any() and valid.any()
            ctx.denoise(levels, guided=True, **guide)
            mean, u8, var = ctx.download_denoised(N.W, N.H, want_var=True)
            assert N.same_bits_nan(mean, want_mean), int(np.count_nonzero(N.bits(mean) != N.bits(want_mean)))
            assert np.array_equal(u8, want_u8)
            assert not np.isnan(var).any() and not np.signbit(var).any() and N.same_bits(var, want_var)
            assert N.same_bits(var[~valid], v0[~valid]) and not np.isnan(mean[valid]).any()
    ctx.close()


def test_refusals(gpu):
    key = "builtin0"
    w, h, depth, spps = SCENES[key]
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    P = lambda k, mode, **kw: gpu.make_params(w, h, 1, depth, SEED0 + k, accumulate=mode, **kw)  # noqa: E731
    go = lambda **kw: ctx.denoise(guided=True, **kw)  # noqa: E731
    _refused(gpu, go, "no live accumulation")
    for k in range(2):
        ctx.render(sc, sc.camera, P(k, True))
    _refused(gpu, go, "carries no Q")
    ctx.render(sc, sc.camera, P(0, "error"))
    _refused(gpu, go, "needs two")
    ctx.render(sc, sc.camera, P(1, "error"))
    _refused(gpu, go, "no G-buffer")
    ctx.gbuffer(sc, sc.camera, w, h)
    for levels in (0, 7):
        _refused(gpu, lambda: go(levels=levels), "levels")
    for k in (0.0, float("nan"), 2048.0):
        _refused(gpu, lambda: go(k=k), "must be finite, > 0 and <= 1024")
    for z in (0.0, -1.0, float("nan"), float("inf"), 2048.0):
        _refused(gpu, lambda: go(sigma_z=z), "sigma_z")
    _refused(gpu, lambda: go(normal_pow2=9), "normal_pow2 9 must be 0 to 8")
    _refused(gpu, lambda: go(demodulate=2), "demodulate 2 must be 0 or 1")
    guide = gpu.FrDenoiseGuide(0.5, 2, 0, 1)
    assert gpu.lib().fr_ctx_denoise_guided(ctx._h, 4, C.c_float(4.0), C.byref(guide)) == gpu.FR_EARG
    assert "pad 1 must be 0" in gpu.lib().fr_last_error().decode()
    _refused(gpu, lambda: ctx.download_denoised(w, h), "no denoised image")  # the refused calls enqueued nothing
    ctx.denoise()  # an unguided image to keep
    before = ctx.download_denoised(w, h)
    # a G-buffer of another camera, size or scene upload than the live accumulation's
    cam2 = gpu.FrCamera.from_buffer_copy(sc.camera)
    cam2.position[0] += 0.5
    ctx.gbuffer(sc, cam2, w, h)
    _refused(gpu, go, "another camera")
    ctx.gbuffer(sc, sc.camera, w - 1, h)
    _refused(gpu, go, f"width {w - 1} differs")
    ctx.gbuffer(sc, sc.camera, w, h + 1)
    _refused(gpu, go, f"height {h + 1} differs")
    sc2 = _product_scene(gpu, key, w, h)
    ctx.gbuffer(sc2, sc.camera, w, h)
    _refused(gpu, go, "another scene upload")
    after = ctx.download_denoised(w, h)
    assert _same_bits(before[0], after[0]) and np.array_equal(before[1], after[1])  # the previous image is still there
    ctx.gbuffer(sc, sc.camera, w, h)
    go(levels=1, k=1024.0, sigma_z=1024.0, normal_pow2=8, demodulate=False)  # the ends of the ranges are in
    go(levels=6, k=2.0 ** -20, sigma_z=2.0 ** -100, normal_pow2=0)
    gpu.check(gpu.lib().fr_ctx_denoise_guided(ctx._h, 4, C.c_float(4.0), None))  # NULL: the defaults
    _check_denoised(ctx, _guided(key, 1), w, h)
    ctx.accum_reset()
    _refused(gpu, go, "no live accumulation")
    for k in range(2):  # a shard of an image
        ctx.render(sc, sc.camera, P(4 + k, "error", shard_index=1, shard_count=2))
    _refused(gpu, go, "shard_count 2")
    ctx.close()
    assert gpu.lib().fr_ctx_denoise_guided(None, 4, C.c_float(4.0), None) == gpu.FR_EARG


def test_update_shows_the_guided_picture(gpu):
    w, h = 32, 24
    m = gpu.create_model(w, h)
    ocam = O.camera_new(w, h)
    d = (C.c_float * 3)()
    comp = R.ErrorComposite()
    for frame in range(3):
        pix = gpu.update(m, 0, 0.1, accumulate="error", denoise="guided").copy()
        gpu.check(gpu.lib().fr_update_delta(0, 0.1, d))
        O.camera_orbit(ocam, list(d))
        seed = m.seed ^ (0x9E3779B97F4A7C15 * (frame + 1) & 0xFFFFFFFFFFFFFFFF)
        omean, _, _, _ = O.render(S.BUILTIN[0](), ocam, w, h, 1, 50, seed=seed)
        mean = comp.add(_frame_sum(omean, 1), 1)
        if frame == 0:
            g = G.gbuffer(S.BUILTIN[0](), ocam, w, h)  # the view of the accumulation's first frame
            assert np.array_equal(pix.reshape(h, w, 3), _to_u8(mean))
            assert G.same(m.ctx.download_gbuffer(w, h), g) == []
        else:
            _, want_u8, _ = DG.denoise(comp.a, comp.q, comp.n, comp.frames, g)
            assert np.array_equal(pix.reshape(h, w, 3), want_u8), frame
            assert not np.array_equal(want_u8, D.denoise(comp.a, comp.q, comp.n, comp.frames)[1])
        assert m.ctx.accum_info() == (frame + 1, frame + 1)
    pix = gpu.update(m, 0b001000, 0.1, accumulate="error", denoise="guided")  # a key press: a new view
    gpu.check(gpu.lib().fr_update_delta(0b001000, 0.1, d))
    O.camera_orbit(ocam, list(d))
    assert m.ctx.accum_info() == (1, 1)
    assert G.same(m.ctx.download_gbuffer(w, h), G.gbuffer(S.BUILTIN[0](), ocam, w, h)) == []
    m.close()
