"""Adaptive sampling (FR_FLAG_ADAPTIVE) on the GPU against the oracle, bit for bit.

The contract (include/forma_rt.h): fr_ctx_adapt turns the live accumulation's error estimate
into a list of active 8x8 tiles; a frame with the flag traces and resolves those tiles only,
with the tile's own counts (A += S, Q += S^2 / spp, n_t += spp, K_t += 1, mean = A / n_t), and
leaves every other pixel's A, Q, counts and outputs as they are. A pixel's random streams depend
on (seed, pixel index, block) alone, so S on an active tile is the plain frame's S: everything is
rebuilt in numpy f32 from whole oracle frames (tests/adaptive_ref.py).

The flow is F F A F F A F A (F: a frame with seed 0xADA0 + k, A: an adapt call). After every
frame: the bits of the mean, the u8 image, accum_info and the frame's stats.samples. After every
adapt: every field of the info, the bits of the error map, and both count maps. Each case's
threshold is a condition the host test holds on the oracle: at the first adapt some tiles are
active and some are not. Images are 33x17 or 32x24 as in test_accumulate.py."""
import ctypes as C

import numpy as np
import pytest

from tests import adaptive_ref as AR
from tests.test_accumulate import _product_scene, _same_bits, _to_u8

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")


def _refused(gpu, call, text):
    with pytest.raises(gpu.ForMaError) as e:
        call()
    assert e.value.code == gpu.FR_EARG and text in str(e.value), str(e.value)


def _check_info(got, want):
    for name in ("frames", "samples", "tiles", "active_tiles", "pixels", "active_pixels", "converged", "min_samples"):
        assert got[name] == want[name], (name, got[name], want[name])
    assert _same_bits(F(got["max_rel"]), want["max_rel"]), (got["max_rel"], want["max_rel"])
    assert _same_bits(F(got["threshold"]), want["threshold"])


def _check_adapt(ctx, step, threshold, min_samples):
    got = ctx.adapt(threshold, min_samples)
    _check_info(got, step["summary"])
    rel = ctx.download_error()
    assert _same_bits(rel, step["rel"]), int(np.count_nonzero(rel.view(np.uint32) != step["rel"].view(np.uint32)))
    n, k = ctx.download_counts()
    assert np.array_equal(n, step["n"]) and np.array_equal(k, step["k"])
    return got


def _check_frame(ctx, step, w, h, spp):
    st = ctx.sync()
    mean, u8 = ctx.download(w, h)
    assert _same_bits(mean, step["mean"]), float(np.max(np.abs(mean - step["mean"])))
    assert np.array_equal(u8, _to_u8(step["mean"]))
    assert ctx.accum_info() == (step["frames"], step["samples"])
    assert st["samples"] == step["traced"] * spp
    if step["traced"] == 0:
        assert st["segments"] == 0 and st["hits"] == 0 and st["trace_launches"] == 0
    else:
        assert step["traced"] * spp <= st["segments"] and st["prim_tests"] >= st["segments"]
    return st


def _flow(gpu, case, scene_jit=False, ctx=None, sync=True, flow=AR.FLOW, uniform_from=None, threshold=None,
          min_samples=None):
    """Walks `flow` on one context against the reference. sync=False: frames are enqueued without
    a sync and only the last frame before each adapt, and the adapts, are checked."""
    key, w, h, depth, spp, thr, mins = AR.CASES[case]
    thr = thr if threshold is None else threshold
    mins = mins if min_samples is None else min_samples
    steps = AR.reference_flow(key, w, h, depth, spp, thr, mins, flow, uniform_from)
    sc = _product_scene(gpu, key, w, h)
    own = ctx is None
    ctx = gpu.RenderContext(0) if own else ctx
    for i, step in enumerate(steps):
        if step["op"] == "F":
            ctx.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, step["seed"], accumulate=step["mode"],
                                                      scene_jit=scene_jit))
            if sync:
                _check_frame(ctx, step, w, h, spp)
        else:
            _check_adapt(ctx, step, thr, mins)  # no sync before it
            if not sync:
                _check_frame(ctx, steps[i - 1], w, h, spp)  # the pending render and its picture are as they were
    if scene_jit:
        assert ctx.jit_state() == gpu.FR_JIT_USED
    if own:
        ctx.close()
    return steps


def _active(steps):
    return [int(s["summary"]["active_tiles"]) for s in steps if s["op"] == "A"]


@pytest.mark.parametrize("case,jit", [("scene08_16", False), ("scene08_16", "wait"), ("scene08_4", False),
                                      ("scene01_2", False), ("builtin0_4", False), ("scene08_32", False)])
def test_flow_against_the_reference(gpu, case, jit):
    steps = _flow(gpu, case, scene_jit=jit)
    first = _active(steps)[0]
    assert 0 < first < steps[2]["summary"]["tiles"]


def test_bvh_family_and_the_empty_list(gpu):
    steps = _flow(gpu, "cubes100_16")
    assert _active(steps)[-2] > 0 and _active(steps)[-1] == 0
    # one more adaptive frame on the empty list: nothing traced, nothing moves
    key, w, h, depth, spp, thr, mins = AR.CASES["cubes100_16"]
    steps = _flow(gpu, "cubes100_16", flow=AR.FLOW + "FA")
    assert steps[-2]["traced"] == 0 and steps[-2]["frames"] == steps[-4]["frames"]
    assert _same_bits(steps[-2]["mean"], steps[-4]["mean"])


def test_one_workgroup_claims_every_batch(gpu, monkeypatch):
    monkeypatch.setenv("FR_MAX_WGS", "1")
    _flow(gpu, "scene08_32")


def test_multi_pass_frames(gpu, monkeypatch):
    """FR_PIPELINE=2 at 64 spp: `running` carries S between the passes under the indirection."""
    monkeypatch.setenv("FR_PIPELINE", "2")
    ctx = gpu.RenderContext(0)
    steps = _flow(gpu, "scene08_64", ctx=ctx)
    assert 0 < _active(steps)[0] < 15 and steps[-2]["traced"] > 0
    assert ctx.sync()["trace_launches"] >= 2
    ctx.close()


@pytest.mark.parametrize("pipe", ["1", "2"])
def test_streamed_frames(gpu, pipe, monkeypatch):
    """Frames enqueued with no sync between them, an adapt between streamed frames."""
    monkeypatch.setenv("FR_FRAME_PIPE", pipe)
    _flow(gpu, "scene08_16", sync=False)


def test_a_plain_accumulating_frame_in_a_tiled_accumulation(gpu):
    """Frames 4 and 5 lack the flag: every tile advances, each with its own divisor."""
    steps = _flow(gpu, "scene08_16", flow="FFAFFAFFA", uniform_from=4)
    last = steps[-1]
    assert len(np.unique(last["n"])) >= 2 and int(last["n"].min()) >= 64  # every tile got the two uniform frames
    assert steps[-2]["mode"] == "error" and steps[-2]["traced"] == 33 * 17


def test_min_samples_alone(gpu):
    """threshold = +inf: every tile is active until its n_t reaches 48, then none."""
    steps = _flow(gpu, "scene08_16", threshold=INF, min_samples=48)
    assert _active(steps) == [15, 0, 0]
    assert steps[-2]["traced"] == 0 and steps[-2]["samples"] == 64


def test_threshold_zero(gpu):
    steps = _flow(gpu, "cubes100_zero", flow="FFA")
    a = steps[-1]
    with_noise = {(y // 8, x // 8) for y, x in zip(*np.nonzero(a["rel"] > 0))}
    assert {(int(s), int(c)) for s, c in zip(*np.nonzero(a["mask"]))} == with_noise


def test_refusals_enqueue_nothing(gpu):
    key, w, h, depth, spp, thr, _ = AR.CASES["scene08_16"]
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    P = lambda k, mode: gpu.make_params(w, h, spp, depth, AR.SEED0 + k, accumulate=mode)  # noqa: E731
    _refused(gpu, lambda: ctx.adapt(thr), "no live accumulation")
    _refused(gpu, lambda: ctx.download_counts(np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)),
             "no live accumulation")
    _refused(gpu, lambda: ctx.render(sc, sc.camera, P(0, "adaptive")), "would start a new accumulation")
    assert ctx.accum_info() == (0, 0)
    ctx.render(sc, sc.camera, P(0, "error"))
    _refused(gpu, lambda: ctx.adapt(thr), "needs two")
    n, k = ctx.download_counts()
    assert (n == spp).all() and (k == 1).all()  # untiled: the uniform values
    ctx.render(sc, sc.camera, P(1, "error"))
    _refused(gpu, lambda: ctx.render(sc, sc.camera, P(2, "adaptive")), "no tile list")
    for bad in (-1.0, float("nan")):
        _refused(gpu, lambda: ctx.adapt(bad), "threshold")
    # the flag without either of the other two
    p = P(2, "adaptive")
    for drop in (gpu.FR_FLAG_ACCUM_ERROR, gpu.FR_FLAG_ACCUMULATE | gpu.FR_FLAG_ACCUM_ERROR):
        q = P(2, "adaptive")
        q.flags = p.flags & ~drop
        _refused(gpu, lambda: ctx.render(sc, sc.camera, q), "FR_FLAG_ADAPTIVE needs")
    assert ctx.accum_info() == (2, 2 * spp)
    ctx.adapt(thr)
    ctx.prepare(sc, sc.camera, P(2, "adaptive"))  # allocates, changes no state
    assert ctx.accum_info() == (2, 2 * spp)
    # an accumulation without Q has no selection
    ctx.render(sc, sc.camera, P(3, True))
    ctx.render(sc, sc.camera, P(4, True))
    _refused(gpu, lambda: ctx.adapt(thr), "carries no Q")
    ctx.close()
    mean = np.zeros((h, w, 3), F)
    p = P(0, "adaptive")
    for n_arg, call in ((0, gpu.lib().fr_render_hip), (1, gpu.lib().fr_render_hip_multi)):
        rc = call(sc._h, C.byref(sc.camera), C.byref(p), n_arg, mean.ctypes.data_as(C.POINTER(C.c_float)), None, None)
        assert rc == gpu.FR_EARG


def test_a_restart_drops_the_list(gpu):
    key, w, h, depth, spp, thr, _ = AR.CASES["scene08_16"]
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    P = lambda k, mode: gpu.make_params(w, h, spp, depth, AR.SEED0 + k, accumulate=mode)  # noqa: E731
    for k in range(2):
        ctx.render(sc, sc.camera, P(k, "error"))
    assert 0 < ctx.adapt(thr)["active_tiles"] < 15
    ctx.render(sc, sc.camera, P(2, "adaptive"))
    assert ctx.accum_info() == (3, 3 * spp)
    moved = gpu.camera_orbit(sc.camera, (0.1, 0.0))
    _refused(gpu, lambda: ctx.render(sc, moved, P(3, "adaptive")), "would start a new accumulation")
    assert ctx.accum_info() == (3, 3 * spp)
    ctx.render(sc, moved, P(3, "error"))  # the camera moved: a new, uniform accumulation
    assert ctx.accum_info() == (1, spp)
    ctx.render(sc, moved, P(4, "error"))
    _refused(gpu, lambda: ctx.render(sc, moved, P(5, "adaptive")), "no tile list")
    n, k = ctx.download_counts()
    assert (n == 2 * spp).all() and (k == 2).all()
    ctx.accum_reset()
    _refused(gpu, lambda: ctx.render(sc, moved, P(5, "adaptive")), "would start a new accumulation")
    ctx.close()


def test_two_shards_stitch_to_the_single_context(gpu):
    key, w, h, depth, spp, thr, mins = AR.CASES["scene08_16"]
    steps = AR.reference_flow(key, w, h, depth, spp, thr, mins)
    sc = _product_scene(gpu, key, w, h)
    m = gpu.MultiContext([0, 0])
    rows = [np.array([y for y in range(h) if (y // 8) % 2 == i]) for i in range(2)]
    for step in steps:
        if step["op"] == "F":
            m.render(sc, sc.camera, gpu.make_params(w, h, spp, depth, step["seed"], accumulate=step["mode"]))
            st = m.sync()
            mean, u8 = m.frame()
            assert _same_bits(mean, step["mean"]) and np.array_equal(u8, _to_u8(step["mean"]))
            assert st["samples"] == step["traced"] * spp
        else:
            got = m.adapt(thr, mins)
            want = dict(step["summary"])
            # (a shard whose list was empty does not advance: the sums hold, the totals are the largest)
            _check_info(got, want)
            n = np.zeros((h, w), np.uint32)
            k = np.zeros((h, w), np.uint32)
            rel = np.full((h, w), np.nan, F)
            for i in range(2):
                c = m.context(i)
                c.download_counts(n, k)
                c.download_error(rel)
            assert np.array_equal(n, step["n"]) and np.array_equal(k, step["k"])
            assert _same_bits(rel, step["rel"])
            for i in range(2):  # and a shard's own selection counts its rows alone (the same list: same bits)
                comp_rows = rows[i]
                one = m.context(i).adapt(thr, mins)
                assert one["tiles"] == len(np.unique(comp_rows // 8)) * 5
                assert one["active_tiles"] == int(step["mask"][np.unique(comp_rows // 8)].sum())
                assert one["pixels"] == len(comp_rows) * w
    m.close()


def test_render_converged_adaptive(gpu):
    key, w, h, depth, spp, thr, _ = AR.CASES["scene08_16"]
    sc = _product_scene(gpu, key, w, h)
    ctx = gpu.RenderContext(0)
    _, _, uni = gpu.render_converged(ctx, sc, sc.camera, w, h, spp, depth, AR.SEED0, thr, max_frames=32)
    assert uni["converged"] == uni["pixels"]
    mean, u8, ada = gpu.render_converged(ctx, sc, sc.camera, w, h, spp, depth, AR.SEED0, thr, max_frames=32,
                                         adaptive=True, min_samples=32)
    assert ada["active_tiles"] == 0 or ada["converged"] == ada["pixels"]
    print(f"uniform: {uni['frames']} frames, {uni['pixels'] * uni['samples']} samples; "
          f"adaptive: {ada['frames']} frames, {ada['traced']} samples")
    assert ada["traced"] < uni["pixels"] * uni["samples"]
    n, _ = ctx.download_counts()
    assert int(n.astype(np.uint64).sum()) == ada["traced"] and int(n.min()) >= 32
    assert np.array_equal(u8, _to_u8(mean))
    ctx.close()
