"""Temporal reuse of a progressive accumulation (fr_ctx_temporal) on the GPU against the oracle,
bit for bit.

The contract (include/forma_rt.h): on the first call of a new accumulation the previous view's
totals are reprojected through the G-buffers of both views into a per-pixel prior; every call adds
the prior to the live accumulation, keeps the totals as the view's history and shows them through
0 to 6 levels of fr_ctx_denoise's or fr_ctx_denoise_guided's filter.

Expected values: the oracle's frames and first hits of the views of tests/temporal_fixtures.py,
passed through tests/temporal_ref.py, which tests/test_temporal_host.py holds against the bits of
the header the kernels compile. Priors, totals, source, reason, mean, u8 and variance are compared
exactly (a NaN for a NaN of any payload)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import accum_error_ref as R
from tests import adaptive_ref as AR
from tests import gbuffer_ref as G
from tests import nonfinite_fixtures as N
from tests import temporal_fixtures as X
from tests import temporal_ref as T
from tests.test_accum_error import _refused
from tests.test_accumulate import _same_bits
from tests.test_denoise_guided_host import OTHER

pytestmark = pytest.mark.gpu
F = np.float32
# (levels, guide): levels 0, 1 and 4, unguided and guided, with and without demodulation
VARIANTS = ((0, None), (1, None), (4, None), (0, {}), (1, {}), (4, {}), (0, OTHER), (4, OTHER))


def _check(ctx, want, w, h, tag):
    got = ctx.download_temporal(w, h)
    for f in T.FIELDS:
        if f in ("source", "reason"):
            assert np.array_equal(got[f], want[f]), (tag, f, int(np.count_nonzero(got[f] != want[f])))
        else:
            assert N.same_bits_nan(got[f], want[f]), (tag, f, int(np.count_nonzero(N.bits(got[f]) != N.bits(want[f]))))
    mean, u8, var = ctx.download_denoised(w, h, want_var=True)
    assert N.same_bits_nan(mean, want["mean"]), (tag, "mean", int(np.count_nonzero(N.bits(mean) != N.bits(want["mean"]))))
    assert np.array_equal(u8, want["u8"]), (tag, "u8")
    assert N.same_bits(var, want["var"]), (tag, "var")
    return got


class _Driver:
    """A context fed the steps of tests/temporal_fixtures.run: ("frame", view), ("restart",),
    ("reset",); the G-buffer is enqueued with the first frame of every accumulation."""

    def __init__(self, gpu, name):
        self.gpu, self.name = gpu, name
        _, self.sc, self.w, self.h = X.scene(gpu, name)
        self.cams = X.product_views(gpu, name, self.sc)
        for cam, ocam in zip(self.cams, X.oracle_views(name)):
            assert np.array_equal(cam.to_array().view(np.uint32), O.camera_to_array(ocam).view(np.uint32))
        self.ctx = gpu.RenderContext(0)
        self.frames, self.cur, self.fresh = 0, None, True

    def step(self, op, accumulate="error"):
        if op[0] == "frame":
            v = op[1]
            self.ctx.render(self.sc, self.cams[v], self.gpu.make_params(self.w, self.h, X.SPP, X.DEPTH, X.SEED0 + self.frames,
                                                                        accumulate=accumulate))
            self.frames += 1
            if self.fresh or v != self.cur:
                self.ctx.gbuffer(self.sc, self.cams[v], self.w, self.h)
            self.cur, self.fresh = v, False
        elif op[0] == "restart":
            self.ctx.accum_reset()
            self.fresh = True
        elif op[0] == "reset":
            self.ctx.temporal_reset()

    def call(self, levels, guide, opt=None):
        self.ctx.temporal(levels, 4.0, guide, **dict(T.OPT, **dict(X.CASES[self.name][4], **(opt or {}))))


@pytest.mark.parametrize("name", ["spheres", "boxes", "spheres_33x17", "metal"])
def test_sequence(gpu, name):
    """V0 -> V1 -> V2, two calls per view: at every call each variant of the levels runs on the
    same prior (a still view's later call keeps the prior's bits)."""
    want = [X.run(name, X.SEQUENCE, levels, 4.0, guide) for levels, guide in VARIANTS]
    d = _Driver(gpu, name)
    calls, prior = 0, None
    for op in X.SEQUENCE:
        if op[0] != "call":
            d.step(op)
            continue
        for i, (levels, guide) in enumerate(VARIANTS):
            d.call(levels, guide)
            got = _check(d.ctx, want[i][calls], d.w, d.h, (name, calls, levels, guide))
        if calls % 2:
            for f in ("prior_a", "prior_q", "prior_n", "prior_k", "source", "reason"):
                assert np.array_equal(N.bits(got[f]) if got[f].dtype == F else got[f],
                                      N.bits(prior[f]) if got[f].dtype == F else prior[f]), f
        prior = got
        assert want[0][calls]["action"] == ("keep" if calls % 2 else "empty" if calls == 0 else "reproject")
        calls += 1
    assert (want[0][2]["reason"] == T.REUSED).any() and d.ctx.accum_info() == (3, 12)
    d.ctx.close()


def test_every_reason_code(gpu):
    """The pair that reaches every code, NaN totals included (tests/test_temporal_fixtures.py)."""
    name = "codes"
    script = (("frame", 0), ("frame", 0), ("call",), ("frame", 1), ("call",))
    d = _Driver(gpu, name)
    calls = 0
    variants = ((0, None), (4, {}))
    want = [X.run(name, script, levels, 4.0, guide) for levels, guide in variants]
    for op in script:
        if op[0] != "call":
            d.step(op)
            continue
        for (levels, guide), wnt in zip(variants, want):
            d.call(levels, guide)
            _check(d.ctx, wnt[calls], d.w, d.h, (name, calls, levels))
        calls += 1
    assert set(np.unique(want[0][1]["reason"])) == set(range(8)) - {T.NO_HISTORY}
    d.ctx.close()


def test_streamed(gpu):
    """Frames, G-buffers and temporal calls enqueued back to back without a sync: the last call's
    results are the sequence's."""
    name = "boxes"
    want = X.run(name, X.SEQUENCE, 4, 4.0, {})
    d = _Driver(gpu, name)
    for op in X.SEQUENCE:
        if op[0] == "call":
            d.call(4, {})
        else:
            d.step(op)
    _check(d.ctx, want[-1], d.w, d.h, name)
    d.ctx.sync()
    d.ctx.close()


def test_tiled_accumulation(gpu):
    """V0 uniform; V1 made tiled by adapt with adaptive frames in between: the totals take each
    tile's own n_t and K_t."""
    name = "boxes"
    thr, mins = 0.6, 0  # (six of the fifteen tiles stay active)
    _, _, w, h = X.scene(None, name)
    tp = T.Temporal()
    comp0 = R.ErrorComposite()
    for k in range(2):
        comp0.add(X.frame_sum(name, 0, X.SEED0 + k), X.SPP)
    cams, cls = X.oracle_views(name), X.classes(name)
    r0 = tp.call(1, X.key_of(name), comp0.a, comp0.q, comp0.n, comp0.frames, X.features(name, 0), cams[0], cls, 0)
    assert (r0["reason"] == T.NO_HISTORY).all()
    comp, mask = AR.AdaptiveComposite(w, h), None
    for k in range(4):
        if k == 2:
            mask, summary = comp.select(thr, mins)
        comp.add(X.frame_sum(name, 1, X.SEED0 + 2 + k), X.SPP, mask)
    assert 0 < int(mask.sum()) < mask.size and len(np.unique(comp.n)) == 2
    want = [tp.call(2, X.key_of(name), comp.a, comp.q, comp.pixels(comp.n), comp.pixels(comp.k), X.features(name, 1),
                    cams[1], cls, levels, 4.0, guide) for levels, guide in ((0, None), (4, {}))]
    assert len(np.unique(want[0]["total_n"])) > 2
    d = _Driver(gpu, name)
    for op in (("frame", 0), ("frame", 0)):
        d.step(op)
    d.call(0, None)
    for k in range(4):
        if k == 2:
            assert d.ctx.adapt(thr, mins)["active_tiles"] == summary["active_tiles"]
        d.step(("frame", 1), accumulate="adaptive" if k >= 2 else "error")
    for (levels, guide), wnt in zip(((0, None), (4, {})), want):
        d.call(levels, guide)
        _check(d.ctx, wnt, w, h, ("tiled", levels))
    d.ctx.close()


@pytest.mark.parametrize("name", ["spheres", "boxes"])
def test_first_view_equals_denoise(gpu, name):
    """K >= 2 and no history: the totals are the accumulation's, so temporal(levels, k) is
    denoise(levels, k) bit for bit, and the guided form denoise(guided=True)."""
    d = _Driver(gpu, name)
    for op in (("frame", 0), ("frame", 0), ("frame", 0)):
        d.step(op)
    for levels, k in ((1, 4.0), (4, 4.0), (6, 0.5)):
        for guide in (None, {}, OTHER):
            if guide is None:
                d.ctx.denoise(levels, k)
            else:
                d.ctx.denoise(levels, k, guided=True, **guide)
            want = d.ctx.download_denoised(d.w, d.h, want_var=True)
            d.ctx.temporal(levels, k, guide)
            got = d.ctx.download_denoised(d.w, d.h, want_var=True)
            assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and _same_bits(got[2], want[2])
    t = d.ctx.download_temporal(d.w, d.h)
    assert (t["reason"] == T.NO_HISTORY).all() and (t["total_n"] == 12).all() and (t["total_k"] == 3).all()
    d.ctx.close()


def test_no_history_after_edit_reset_and_resize(gpu):
    name = "spheres"
    d = _Driver(gpu, name)
    w, h = d.w, d.h

    def view(v, sc=None, size=None):
        ww, hh = size or (w, h)
        cam = d.cams[v]
        for k in range(2):
            d.ctx.render(sc or d.sc, cam, gpu.make_params(ww, hh, X.SPP, X.DEPTH, X.SEED0 + k, accumulate="error"))
        d.ctx.gbuffer(sc or d.sc, cam, ww, hh)
        d.ctx.temporal(0)
        return d.ctx.download_temporal(ww, hh)

    assert (view(0)["reason"] == T.NO_HISTORY).all()
    assert (view(1)["reason"] == T.REUSED).any()
    d.ctx.temporal_reset()
    d.ctx.accum_reset()
    r = view(0)
    assert (r["reason"] == T.NO_HISTORY).all() and (r["source"] == T.NONE).all() and not r["prior_n"].any()
    assert (view(1)["reason"] == T.REUSED).any()
    d.sc.translate(0, (-1.0, 0.0, 0.0))  # a scene edit (the plane, at its own place): a new upload
    assert (view(0)["reason"] == T.NO_HISTORY).all()
    assert (view(1)["reason"] == T.REUSED).any()
    assert (view(0, size=(w + 8, h))["reason"] == T.NO_HISTORY).all()  # (the camera's aspect is the old one's: any view will do)
    assert (view(1, size=(w + 8, h))["reason"] == T.REUSED).any()
    # the same camera after accum_reset reuses the view's own history: every accepted pixel maps to itself
    d.ctx.accum_reset()
    r = view(1, size=(w + 8, h))
    ok = r["reason"] == T.REUSED
    assert ok.any() and np.array_equal(r["source"][ok], np.arange((w + 8) * h, dtype=np.uint32).reshape(h, w + 8)[ok])
    d.ctx.close()


def test_refusals(gpu):
    name = "spheres"
    d = _Driver(gpu, name)
    ctx, sc, w, h, cam = d.ctx, d.sc, d.w, d.h, d.cams[0]
    P = lambda k, mode, **kw: gpu.make_params(w, h, 1, X.DEPTH, X.SEED0 + k, accumulate=mode, **kw)  # noqa: E731
    go = ctx.temporal
    _refused(gpu, go, "no live accumulation")
    ctx.render(sc, cam, P(0, True))
    _refused(gpu, go, "carries no Q")
    ctx.render(sc, cam, P(0, "error"))
    _refused(gpu, go, "no G-buffer")
    ctx.gbuffer(sc, cam, w, h)
    go()  # one frame is accepted
    before, state = ctx.download_denoised(w, h, want_var=True), ctx.download_temporal(w, h)
    _refused(gpu, lambda: go(levels=7), "levels 7 must be 0 to 6")
    for k in (0.0, float("nan"), 2048.0):
        _refused(gpu, lambda: go(k=k), "must be finite, > 0 and <= 1024")
    for bad in (dict(n_max=0.0), dict(n_max=float("nan")), dict(n_max=2.0 ** 25), dict(n_max_specular=-1.0),
                dict(n_max_specular=float("inf")), dict(sigma_z=0.0), dict(sigma_z=2048.0), dict(normal_min=1.5),
                dict(normal_min=float("nan"))):
        _refused(gpu, lambda: go(**bad), next(iter(bad)))
    _refused(gpu, lambda: go(guide=dict(sigma_z=0.0)), "sigma_z")
    _refused(gpu, lambda: go(guide=dict(normal_pow2=9)), "normal_pow2 9 must be 0 to 8")
    _refused(gpu, lambda: go(guide=dict(demodulate=2)), "demodulate 2 must be 0 or 1")
    opt = gpu.FrTemporal(32.0, 8.0, 0.5, 0.9)
    opt.pad[2] = 1
    assert gpu.lib().fr_ctx_temporal(ctx._h, 4, C.c_float(4.0), None, C.byref(opt)) == gpu.FR_EARG
    assert "pad 1 must be 0" in gpu.lib().fr_last_error().decode()
    cam2 = gpu.FrCamera.from_buffer_copy(cam)
    cam2.position[0] += 0.5
    ctx.gbuffer(sc, cam2, w, h)
    _refused(gpu, go, "another camera")
    ctx.gbuffer(sc, cam, w - 1, h)
    _refused(gpu, go, f"width {w - 1} differs")
    ctx.gbuffer(sc, cam, w, h + 1)
    _refused(gpu, go, f"height {h + 1} differs")
    sc2 = X.scene(gpu, name)[1]
    ctx.gbuffer(sc2, cam, w, h)
    _refused(gpu, go, "another scene upload")
    # nothing was enqueued and no state moved: the outputs, the history and the accumulation stand
    after, state2 = ctx.download_denoised(w, h, want_var=True), ctx.download_temporal(w, h)
    assert all(_same_bits(a, b) if a.dtype == F else np.array_equal(a, b) for a, b in zip(before, after))
    assert all(np.array_equal(N.bits(state[f]) if state[f].dtype == F else state[f],
                              N.bits(state2[f]) if state[f].dtype == F else state2[f]) for f in T.FIELDS)
    assert ctx.accum_info() == (1, 1)
    ctx.gbuffer(sc, cam, w, h)
    go(levels=0, k=1024.0, n_max=2.0 ** 24, n_max_specular=0.0, sigma_z=1024.0, normal_min=-1.0)  # the ends of the ranges
    go(levels=6, k=2.0 ** -20, n_max=2.0 ** -100, n_max_specular=2.0 ** 24, sigma_z=2.0 ** -100, normal_min=1.0)
    gpu.check(gpu.lib().fr_ctx_temporal(ctx._h, 4, C.c_float(4.0), None, None))  # NULL: unguided, the defaults
    ctx.accum_reset()
    _refused(gpu, go, "no live accumulation")
    ctx.render(sc, cam, P(4, "error", shard_index=1, shard_count=2))
    _refused(gpu, go, "shard_count 2")
    ctx.close()
    assert gpu.lib().fr_ctx_temporal(None, 4, C.c_float(4.0), None, None) == gpu.FR_EARG
    assert gpu.lib().fr_ctx_download_temporal(*([None] * 11)) == gpu.FR_EARG


@pytest.mark.parametrize("mode", ["temporal", "temporal-guided"])
def test_update_shows_the_temporal_picture(gpu, mode):
    """update() over still, orbit, orbit, still: every frame's model.pixels is the restatement's u8,
    the moved camera's first frames included."""
    w, h, depth = 32, 24, 8
    m = gpu.create_model(w, h)
    ocam = O.camera_new(w, h)
    prims, cls = S.BUILTIN[0](), T.scatter_classes(S.BUILTIN[0]())
    d = (C.c_float * 3)()
    tp, comp, gen, g, prev, reused = T.Temporal(), None, 0, None, None, []
    for frame, keys in enumerate((0, 0b001000, 0b001000, 0)):
        pix = gpu.update(m, keys, 0.1, max_depth=depth, accumulate="error", denoise=mode).copy()
        gpu.check(gpu.lib().fr_update_delta(keys, 0.1, d))
        O.camera_orbit(ocam, list(d))  # (update() orbits on every frame; a zero delta after the first keeps the camera)
        if O.camera_to_array(ocam).tobytes() != prev:
            comp, gen, g = R.ErrorComposite(), gen + 1, G.gbuffer(prims, ocam, w, h)
        prev = O.camera_to_array(ocam).tobytes()
        seed = m.seed ^ (0x9E3779B97F4A7C15 * (frame + 1) & 0xFFFFFFFFFFFFFFFF)
        omean, _, _, _ = O.render(prims, ocam, w, h, 1, depth, seed=seed)
        comp.add(N.frame_sum(omean, 1), 1)
        r = tp.call(gen, (0, w, h, depth), comp.a, comp.q, comp.n, comp.frames, g, O.OrCamera.from_buffer_copy(ocam), cls,
                    guide={} if mode == "temporal-guided" else None)
        assert np.array_equal(pix.reshape(h, w, 3), r["u8"]), frame
        reused.append(int((r["reason"] == T.REUSED).sum()))
    assert reused[0] == 0 and min(reused[1:3]) > 0
    assert m.ctx.accum_info() == (2, 2)
    m.close()


def test_stage_events(gpu):
    """fr_ctx_trace_log_read(which = 4): three HIP-event durations per temporal() call made while
    the log is on (the prior, totals and prep, the picture), none before it was."""
    d = _Driver(gpu, "spheres")
    d.step(("frame", 0))
    d.call(0, None)
    d.ctx.trace_log(True)
    assert d.ctx.trace_log_read(temporal=True) == []
    d.step(("frame", 1))
    for levels, guide in ((0, None), (4, None), (4, {})):
        d.call(levels, guide)
    ms = d.ctx.trace_log_read(temporal=True)
    assert len(ms) == 9 and all(0.0 <= t < 1000.0 for t in ms) and all(t > 0.0 for t in ms[1::3] + ms[2::3])
    assert d.ctx.trace_log_read() != [] and len(d.ctx.trace_log_read(frames=True)) == 1  # the other logs are as they were
    d.ctx.trace_log(False)
    d.call(0, None)
    assert len(d.ctx.trace_log_read(temporal=True)) == 9
    _check(d.ctx, X.run("spheres", (("frame", 0), ("call",), ("frame", 1), ("call",)), 0)[1], d.w, d.h, "events")
    d.ctx.close()
