"""The error estimate of progressive accumulation (FR_FLAG_ACCUM_ERROR) on the GPU against the
oracle, bit for bit.

The contract (include/forma_rt.h): a frame with the flag also does Q = S^2 / spp or
Q = Q + S^2 / spp per channel in its resolve; fr_ctx_accum_error turns A and Q into a relative
standard error per pixel, counts the pixels at or under a threshold and takes the maximum.

The exact reference is tests/test_accumulate.py's: for spp a power of two S = mean * spp exactly,
so A, Q, rel, the count and the maximum are rebuilt in numpy f32 from the oracle's frames
(tests/accum_error_ref.py, which tests/test_accum_error_host.py holds against the bits of the
header the kernels compile). After every frame from the second on: the mean's bits and the u8
image (the FR_FLAG_ACCUMULATE composite: the flag never changes the picture), the error map's
bits, pixels, converged, max_rel's bits, frames and samples.

Images are 33x17 or 32x24 as in test_accumulate.py: several sum and error workgroups, the last
one partly filled, and at 33x17 partial tiles and a partial strip."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import accum_error_ref as R
from tests.test_accumulate import _frame_sum, _oracle_frame, _product_scene, _same_bits, _to_u8

pytestmark = pytest.mark.gpu
F = np.float32
SEED0 = 0xE220
T = 2.0 ** -4  # the threshold the cases are summarised at


@functools.lru_cache(maxsize=None)
def _composites(key, w, h, depth, spps):
    """The expected state after every frame of an accumulation whose frame k has seed
    SEED0 + k: a list of (mean, u8, rel, A-and-Q composite snapshot), computed once."""
    comp = R.ErrorComposite()
    out = []
    for k, spp in enumerate(spps):
        omean, _, _, _ = _oracle_frame(key, w, h, spp, depth, SEED0 + k)
        mean = comp.add(_frame_sum(omean, spp), spp)
        rel = comp.rel() if comp.frames >= 2 else None
        out.append({"mean": mean, "u8": _to_u8(mean), "rel": rel, "n": comp.n, "frames": comp.frames,
                    "a": comp.a.copy(), "q": comp.q.copy()})
    return out


def _want_summary(state, threshold, rows=None):
    rel = state["rel"] if rows is None else state["rel"][rows]
    return {"frames": state["frames"], "samples": state["n"], "pixels": int(rel.size),
            "converged": int(np.count_nonzero(rel <= F(threshold))), "max_rel": F(rel.max())}


def _check_summary(got, want, threshold):
    assert got["frames"] == want["frames"] and got["samples"] == want["samples"]
    assert got["pixels"] == want["pixels"]
    assert got["converged"] == want["converged"]
    assert _same_bits(F(got["max_rel"]), want["max_rel"]), (got["max_rel"], want["max_rel"])
    assert got["threshold"] == F(threshold)


def _check_frame(ctx, state, w, h, threshold=T):
    """Everything a frame from the second on is held to."""
    ctx.sync()
    mean, u8 = ctx.download(w, h)
    assert _same_bits(mean, state["mean"]), float(np.max(np.abs(mean - state["mean"])))
    assert np.array_equal(u8, state["u8"])
    assert ctx.accum_info() == (state["frames"], state["n"])
    got, rel = ctx.accum_error(threshold, want_map=True)
    assert rel.shape == (h, w) and not np.isnan(rel).any()
    assert _same_bits(rel, state["rel"]), int(np.count_nonzero(rel.view(np.uint32) != state["rel"].view(np.uint32)))
    want = _want_summary(state, threshold)
    assert want["pixels"] == w * h
    _check_summary(got, want, threshold)


def _refused(gpu, call, text):
    with pytest.raises(gpu.ForMaError) as e:
        call()
    assert e.value.code == gpu.FR_EARG and text in str(e.value), str(e.value)


def _accumulate(gpu, key, w, h, depth, spps, scene_jit=False, ctx=None, threshold=T):
    """len(spps) frames with the flag on one context, checked after every frame from the second
    on; accum_error is refused after the first. Returns the expected states."""
    states = _composites(key, w, h, depth, tuple(spps))
    sc = _product_scene(gpu, key, w, h)
    own = ctx is None
    ctx = gpu.RenderContext(0) if own else ctx
    for k, spp in enumerate(spps):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error", scene_jit=scene_jit))
        if k == 0:
            _refused(gpu, lambda: ctx.accum_error(T), "needs two")
            ctx.sync()
            mean, u8 = ctx.download(w, h)
            assert _same_bits(mean, states[0]["mean"]) and np.array_equal(u8, states[0]["u8"])
        else:
            _check_frame(ctx, states[k], w, h, threshold)
    if scene_jit:
        assert ctx.jit_state() == gpu.FR_JIT_USED
    if own:
        ctx.close()
    # not vacuous: at the last frame some pixels are under the threshold and some are not
    done = _want_summary(states[-1], threshold)["converged"]
    assert 0 < done < w * h, done
    return states


# every resolve instantiation that fills Q, at the smallest shapes that reach it
def test_short_frames_sum_kernel_8_byte_records(gpu):  # spp < 16: sum_kernel<2>
    _accumulate(gpu, "scene_08", 33, 17, 8, [4] * 5)


@pytest.mark.parametrize("spps,jit", [((16,) * 4, False), ((32,) * 3, False), ((16,) * 4, "wait")])
def test_full_blocks_sum_nib_kernel(gpu, spps, jit):
    _accumulate(gpu, "scene_08", 33, 17, 8, spps, scene_jit=jit)


def test_deferred_12_byte_records(gpu):  # sum_kernel<3>, deferred records
    states = _accumulate(gpu, "scene_01", 33, 17, 8, [2] * 4)
    assert np.count_nonzero(states[-1]["rel"] == 0) >= 1  # pixels every sample of which agreed


def test_colour_records_at_update_shape(gpu):  # depth 50: sum_kernel<3> adds colours
    states = _accumulate(gpu, "builtin0", 32, 24, 50, [1] * 6)
    last = states[-1]
    m, _ = R.variance(last["a"], last["q"], last["n"], last["frames"])
    with np.errstate(all="ignore"):
        raw = ((last["q"] - (last["a"] * m).astype(F)).astype(F) / F(last["frames"] - 1)).astype(F)
    assert np.count_nonzero(raw < 0) >= 1  # a channel whose Q - A^2 / n is negative: clamped to 0
    msum = ((m[..., 0] + m[..., 1]).astype(F) + m[..., 2]).astype(F)
    assert np.count_nonzero(msum <= R.FLOOR) >= 1  # a pixel at the 2^-7 floor of the denominator


def test_bvh_class_records(gpu):  # sum_nib_kernel reads the attenuation-class table
    _accumulate(gpu, "cubes100", 33, 17, 8, [16] * 3)


def test_frames_of_different_spp(gpu):  # the resolve kernel, and spp in S^2 / spp, change from frame to frame
    states = _accumulate(gpu, "scene_08", 33, 17, 8, [1, 4, 16, 2])
    assert states[-1]["n"] == 23


def test_threshold_sweep(gpu):
    key, w, h, depth, spps = "cubes100", 33, 17, 8, (16,) * 3  # has pixels whose estimate is exactly 0
    states = _composites(key, w, h, depth, spps)
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k, spp in enumerate(spps):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
    rel = states[-1]["rel"]
    assert 0 < np.count_nonzero(rel == 0) < np.count_nonzero(rel <= F(2.0 ** -5))
    counts = []
    for thr in (0.0, 2.0 ** -5, 2.0 ** -4, 2.0 ** -3, float("inf")):
        got = ctx.accum_error(thr)
        _check_summary(got, _want_summary(states[-1], thr), thr)
        counts.append(got["converged"])
    assert counts[0] == int(np.count_nonzero(rel == 0))  # 0 counts the pixels whose estimate is exactly 0
    assert counts[-1] == w * h  # +inf counts all of them
    assert counts == sorted(set(counts))  # five different counts
    ctx.close()


def test_multi_pass_frames(gpu, monkeypatch):
    """FR_PIPELINE=3: `running` carries S between a frame's passes, only the last pass's resolve
    touches A and Q."""
    monkeypatch.setenv("FR_PIPELINE", "3")
    ctx = gpu.RenderContext(0)
    # (192 samples bring every pixel under 2^-4; 2^-5 still divides them)
    _accumulate(gpu, "scene_08", 33, 17, 8, [64] * 3, ctx=ctx, threshold=2.0 ** -5)
    assert ctx.sync()["trace_launches"] >= 2
    ctx.close()


@pytest.mark.parametrize("pipe", [None, "2"])
def test_streamed_frames(gpu, pipe, monkeypatch):
    """Six frames enqueued with no sync, then accum_error: the sum stream alone orders Q's
    read-modify-writes and the error kernel behind them."""
    if pipe is None:
        monkeypatch.delenv("FR_FRAME_PIPE", raising=False)
    else:
        monkeypatch.setenv("FR_FRAME_PIPE", pipe)
    key, w, h, spp, depth = "scene_08", 33, 17, 16, 8
    states = _composites(key, w, h, depth, (spp,) * 6)
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k in range(6):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
    got, rel = ctx.accum_error(T, want_map=True)  # no sync before it
    assert _same_bits(rel, states[-1]["rel"])
    _check_summary(got, _want_summary(states[-1], T), T)
    _check_frame(ctx, states[-1], w, h)  # the pending render, its picture and the state are as they were
    ctx.close()


def test_restarts(gpu):
    """Toggling the flag, a camera orbit, a scene edit and accum_reset each start a new
    accumulation: accum_info == (1, spp), and accum_error is refused until the second frame."""
    w, h, spp, depth = 32, 24, 2, 8
    sc = _product_scene(gpu, "builtin0", w, h)
    cam = sc.camera
    ctx = gpu.RenderContext(0)
    seed = [SEED0]

    def frame(accumulate="error"):
        seed[0] += 1
        ctx.render(sc, cam, gpu.make_params(w, h, spp, depth, seed[0], accumulate=accumulate))
        ctx.sync()

    _refused(gpu, lambda: ctx.accum_error(T), "no live accumulation")
    frame()
    frame()
    assert ctx.accum_error(T)["frames"] == 2
    causes = [("flag_off", lambda: None, True), ("flag_on", lambda: None, "error"),
              ("orbit", lambda: gpu.camera_orbit(cam, (0.3, 0.1, 0.0)), "error"),
              ("scene_translate", lambda: sc.translate(0, (-1.0, 0.0, 0.0)), "error"),
              ("accum_reset", ctx.accum_reset, "error")]
    for name, cause, acc in causes:
        cause()
        frame(acc)
        assert ctx.accum_info() == (1, spp), name
        if acc == "error":
            _refused(gpu, lambda: ctx.accum_error(T), "needs two")
            frame(acc)
            got = ctx.accum_error(T)
            assert (got["frames"], got["samples"], got["pixels"]) == (2, 2 * spp, w * h), name
        else:
            frame(acc)
            assert ctx.accum_info() == (2, 2 * spp)
            _refused(gpu, lambda: ctx.accum_error(T), "carries no Q")
    ctx.close()


def test_plain_render_in_between_leaves_q_alone(gpu):
    key, w, h, spp, depth = "scene_08", 33, 17, 4, 8
    states = _composites(key, w, h, depth, (spp,) * 3)
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k in range(3):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
        ctx.sync()
        if k == 1:  # a plain frame of another seed, spp and shard between two frames of the accumulation
            ctx.render(sc, sc.camera, gpu.make_params(w, h, 16, depth, 77, shard_index=1, shard_count=2))
            ctx.sync()
            assert ctx.accum_info() == (2, 2 * spp)
            got, rel = ctx.accum_error(T, want_map=True)  # still the accumulation's own shape and state
            assert _same_bits(rel, states[1]["rel"])
            _check_summary(got, _want_summary(states[1], T), T)
    _check_frame(ctx, states[2], w, h)
    ctx.close()


def test_prepare_of_a_larger_frame_keeps_q(gpu):
    key, w, h, spp, depth = "scene_08", 33, 17, 4, 8
    states = _composites(key, w, h, depth, (spp,) * 3)
    sc = _product_scene(gpu, key, w, h)
    big = _product_scene(gpu, key, 64, 40)
    ctx = gpu.RenderContext(0)
    for k in range(3):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
        if k == 1:  # grows A and Q (and replaces the output buffers); what A and Q hold goes on
            ctx.sync()
            ctx.prepare(big, big.camera, gpu.make_params(64, 40, spp, depth, accumulate="error"))
            assert ctx.accum_info() == (2, 2 * spp)
            got, rel = ctx.accum_error(T, want_map=True)
            assert _same_bits(rel, states[1]["rel"])
            _check_summary(got, _want_summary(states[1], T), T)
    _check_frame(ctx, states[2], w, h)
    ctx.close()


def test_a_shard_writes_only_its_rows(gpu):
    key, w, h, spp, depth = "scene_08", 33, 17, 4, 8  # three strips: shard 1 of 2 owns rows 8..15
    states = _composites(key, w, h, depth, (spp,) * 3)
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    for k in range(3):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, shard_index=1, shard_count=2,
                                                  accumulate="error"))
    got = ctx.accum_error(T)
    rows = slice(8, 16)
    _check_summary(got, _want_summary(states[-1], T, rows), T)
    assert got["pixels"] == 8 * w
    rel = np.full((h, w), np.nan, F)
    gpu.check(gpu.lib().fr_ctx_download_error(ctx._h, rel.ctypes.data_as(C.POINTER(C.c_float))))
    assert _same_bits(rel[rows], states[-1]["rel"][rows])
    assert np.isnan(rel[:8]).all() and np.isnan(rel[16:]).all()
    ctx.close()


def test_multi_context_equals_one_context(gpu):
    key, w, h, spp, depth = "scene_08", 33, 17, 4, 8  # shard 0 has two strips, shard 1 one
    states = _composites(key, w, h, depth, (spp,) * 3)
    sc = _product_scene(gpu, key, w, h)
    m = gpu.MultiContext([0, 0])
    for k in range(3):
        m.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, SEED0 + k, accumulate="error"))
        m.sync()
        mean, u8 = m.frame()
        assert _same_bits(mean, states[k]["mean"]) and np.array_equal(u8, states[k]["u8"]), k
        if k == 0:
            _refused(gpu, lambda: m.accum_error(T), "needs two")
            continue
        got, rel = m.accum_error(T, want_map=True)
        assert _same_bits(rel, states[k]["rel"]), k  # the stitched map is the single context's
        _check_summary(got, _want_summary(states[k], T), T)
        parts = [m.context(i).accum_error(T) for i in range(2)]
        assert got["pixels"] == sum(p["pixels"] for p in parts) == w * h
        assert got["converged"] == sum(p["converged"] for p in parts)
        assert got["max_rel"] == max(p["max_rel"] for p in parts)
        assert [p["pixels"] for p in parts] == [9 * w, 8 * w]
    m.close()


def test_errors(gpu):
    w, h = 32, 24
    sc = _product_scene(gpu, "builtin0", w, h)
    ctx = gpu.RenderContext(0)
    p = gpu.make_params(w, h, 2, 8, accumulate="error")
    p.flags &= ~gpu.FR_FLAG_ACCUMULATE
    _refused(gpu, lambda: ctx.render(sc, sc.camera, p), "FR_FLAG_ACCUM_ERROR without FR_FLAG_ACCUMULATE")
    _refused(gpu, lambda: ctx.render(sc, sc.camera, gpu.make_params(w, h, 0, 8, accumulate="error")),
             "FR_FLAG_ACCUM_ERROR with spp 0")
    _refused(gpu, lambda: ctx.render(sc, sc.camera, gpu.make_params(w, h, 2, 50, accumulate="error", mt_bands=True)),
             "FR_FLAG_MT_BANDS")
    assert ctx.accum_info() == (0, 0)
    _refused(gpu, lambda: ctx.accum_error(T), "no live accumulation")
    _refused(gpu, lambda: ctx.download_error(np.zeros((h, w), F)), "no error map")
    for k in range(2):
        ctx.render(sc, sc.camera, gpu.make_params(w, h, 2, 8, 5 + k, accumulate=True))
    _refused(gpu, lambda: ctx.accum_error(T), "carries no Q")
    ctx.render(sc, sc.camera, gpu.make_params(w, h, 2, 8, 7, accumulate="error"))
    _refused(gpu, lambda: ctx.accum_error(T), "needs two")
    ctx.render(sc, sc.camera, gpu.make_params(w, h, 2, 8, 8, accumulate="error"))
    _refused(gpu, lambda: ctx.accum_error(float("nan")), "threshold")
    _refused(gpu, lambda: ctx.accum_error(-0.5), "threshold")
    assert ctx.accum_error(float("inf"))["converged"] == w * h
    ctx.accum_reset()
    _refused(gpu, lambda: ctx.accum_error(T), "no live accumulation")
    ctx.close()
    # the one-shot calls refuse the flag through FR_FLAG_ACCUMULATE
    p = gpu.make_params(w, h, 2, 8, accumulate="error")
    mean = np.zeros((h, w, 3), F)
    rc = gpu.lib().fr_render_hip(sc._h, C.byref(sc.camera), C.byref(p), 0, mean.ctypes.data_as(C.POINTER(C.c_float)),
                                 None, None)
    assert rc == gpu.FR_EARG and b"FR_FLAG_ACCUMULATE" in gpu.lib().fr_last_error()


def test_update_carries_the_estimate(gpu):
    w, h = 32, 24
    m = gpu.create_model(w, h)
    plain = gpu.create_model(w, h)
    for frame in range(3):
        pix = gpu.update(m, 0, 0.1, accumulate="error").copy()
        ref = gpu.update(plain, 0, 0.1, accumulate=True)
        assert np.array_equal(pix, ref), frame  # the same picture as accumulate=True
    got = m.ctx.accum_error(T)
    assert (got["frames"], got["samples"], got["pixels"]) == (3, 3, w * h)
    m.close()
    plain.close()


def test_render_converged_stops_where_the_composite_says(gpu):
    key, w, h, spp, depth, max_frames = "scene_08", 33, 17, 16, 8, 8
    target, fraction = 2.0 ** -3, 0.99
    states = _composites(key, w, h, depth, (spp,) * max_frames)
    stop = next(k + 1 for k in range(1, max_frames)
                if _want_summary(states[k], target)["converged"] >= fraction * w * h)
    assert 2 < stop < max_frames, stop  # the loop is seen to go on past frame 2 and to stop by itself
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    # frame k = 1, 2, ... has seed `seed + k`: the composite's frames
    mean, u8, summary = gpu.render_converged(ctx, sc, sc.camera, w, h, spp, depth, SEED0 - 1, target, fraction=fraction,
                                             max_frames=max_frames)
    assert ctx.accum_info() == (stop, stop * spp)
    assert _same_bits(mean, states[stop - 1]["mean"]) and np.array_equal(u8, states[stop - 1]["u8"])
    _check_summary(summary, _want_summary(states[stop - 1], target), target)
    # checked every third frame only, it stops at the first multiple of 3 at or past that frame
    mean, u8, summary = gpu.render_converged(ctx, sc, sc.camera, w, h, spp, depth, SEED0 - 1, target, fraction=fraction,
                                             max_frames=max_frames, check_every=3)
    stop3 = next(k for k in range(3, max_frames + 1, 3)
                 if _want_summary(states[k - 1], target)["converged"] >= fraction * w * h)
    assert ctx.accum_info() == (stop3, stop3 * spp) and summary["frames"] == stop3
    assert _same_bits(mean, states[stop3 - 1]["mean"])
    ctx.close()
