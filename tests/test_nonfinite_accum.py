"""Non-finite and out-of-range pixels through accumulate, error, adapt and denoise on the GPU,
against the oracle bit for bit.

The contract (include/forma_rt.h, accum_error.h, denoise.h): a NaN variance reads 0, the
relative error of a pixel whose summed mean is NaN or infinite is +0 and never NaN or negative
(so the reductions and fr_ctx_adapt order its bits as uint32), a pixel over the denoise's caps
or not finite is invalid, is tapped by nobody and comes out of every level as prep left it. The
host tests hold the numpy references to the headers' host build; every other GPU test of the
chain renders scenes whose pixels are all ordinary. Here the frames of
tests/nonfinite_fixtures.py (colours of inf, -inf, NaN, 2^17, 2^-18 and a negative one on the
lattices, 32 x 32, mostly one sample per pixel) go through the device build of the same chain:
the resolve kernels add inf to inf and inf to NaN in A and Q, fmax_num meets NaN operands, the
finiteness test and dn_prep's comparisons meet NaN, and S, S^2 / spp, A / n and var are denormal
or underflow. tests/test_nonfinite_fixtures.py holds, without a GPU, that every case reaches the
classes of pixels it is named for.

The mean and what is copied from it are compared NaN-aware (NaN equals NaN of any sign and
payload, everything else bit for bit); rel, max_rel and the denoise's variance strictly bit for
bit and free of NaN; the u8 images and every count exactly.

What each check would catch (the faults applied to the numpy references in a scratch run,
nothing is broken on the device):
  - the finiteness test folded away ((msum - msum) == 0 taken for true): a NaN channel leaves
    the floor as denominator and the other channels' noise as the error; rel's bits differ on
    521 pixels of the nan case, 231 of the -inf and 115 of the inf case, and max_rel with them;
  - fmax_num returning its NaN operand: rel is NaN on the 414 pixels of the 2^17 case whose A is
    finite and whose Q has overflowed (the map's comparison, its isnan assertion, and max_rel: a
    maximum over bits, where a NaN's are above every number's); in dn_prep var would be NaN, which
    the strict comparison of the variance map and its isnan assertion hold;
  - an invalid pixel tapped: every valid pixel of the 2^17 case is an exact 0 among invalid
    neighbours of 2^41 and more, and 135 valid pixels of the inf, -inf and nan cases have an
    invalid pixel among their step-1 taps; the mean and the variance differ at 1, 4 and 6 levels;
  - the invalid bit dropped after a level: the pixel is filtered and tapped from the next level
    on; mean and variance differ at 4 and 6 levels, and the invalid pixels are no longer prep's;
  - a flushed denormal: 441 channels of the 2^-18 case's S are denormal and 773 pixels have an
    S^2 that underflows. A flush of S changes the mean's bits in 44 to 80 pixels per frame, one
    in Q's terms rel's bits in 19 (every pixel of that case sits on the 2^-7 floor); one of
    prep's mean or variance, or of a level's output, shows in the denoise at one level (38
    denormal means and 5 denormal variances after frame 2; four levels average them away);
  - inf - inf in the resolve: the -inf case's accumulator meets +inf and -inf in one channel
    (NaN from then on) and keeps -inf in 12 pixels, whose u8 is 0.

51 tests of a few 1024-pixel frames each: 3 s on an MI355X (the magnitude file: 47 s)."""
import numpy as np
import pytest

from tests import denoise_ref as D
from tests import magnitude_fixtures as M
from tests import nonfinite_fixtures as N
from tests.test_accumulate import _to_u8
from tests.test_adaptive import _check_info

pytestmark = pytest.mark.gpu
F = np.float32
W, H, T = N.W, N.H, N.T


def _scene(gpu, case):
    prims = N.prims(case)
    if case.size == "big":
        assert M.bvh_cost(prims) >= 48 and len(prims) >= 48  # the BVH family
    return gpu.Scene.from_prims(prims), N.cameras(gpu)[0]


def _params(gpu, case, k, mode, jit=False):
    return gpu.make_params(W, H, case.spps[k], case.depth, N.seed_of(case, k), accumulate=mode, scene_jit=jit)


def _check_picture(ctx, st):
    mean, u8 = ctx.download(W, H)
    assert N.same_bits_nan(mean, st["mean"]), int(np.count_nonzero(N.bits(mean) != N.bits(st["mean"])))
    assert np.array_equal(u8, st["u8"])
    assert ctx.accum_info() == (st["frames"], st["n"])


def _check_counters(stats, st, spp):
    cnt = st["counters"]
    assert (stats["segments"], stats["hits"], stats["scatters"]) == (cnt["segments"], cnt["hits"], cnt["scatters"])
    assert stats["samples"] == W * H * spp


def _check_summary(got, st, threshold):
    want = N.summary(st, threshold)
    assert (got["frames"], got["samples"], got["pixels"]) == (want["frames"], want["samples"], W * H)
    assert got["converged"] == want["converged"], (threshold, got["converged"], want["converged"])
    assert N.same_bits(F(got["max_rel"]), want["max_rel"]), (got["max_rel"], want["max_rel"])
    assert not np.isnan(got["max_rel"]) and got["threshold"] == F(threshold)


def _check_error(ctx, st, threshold=T):
    got, rel = ctx.accum_error(threshold, want_map=True)
    assert rel.shape == (H, W) and not np.isnan(rel).any() and not np.signbit(rel).any()
    assert N.same_bits(rel, st["rel"]), int(np.count_nonzero(N.bits(rel) != N.bits(st["rel"])))
    _check_summary(got, st, threshold)


def _accumulate(gpu, case, mode, jit=False, stream=False):
    """The case's frames on one context. Checked after every frame (stream: after the last one
    alone, the frames enqueued with no sync between them): the picture, the frame's counters
    and, for mode "error" from the second frame on, the estimate."""
    states = N.states(case)
    sc, cam = _scene(gpu, case)
    ctx = gpu.RenderContext(0)
    for k, spp in enumerate(case.spps):
        ctx.render(sc, cam, _params(gpu, case, k, mode, jit))
        if stream and k + 1 < len(case.spps):
            continue
        _check_counters(ctx.sync(), states[k], spp)
        _check_picture(ctx, states[k])
        if mode == "error" and k >= 1:
            _check_error(ctx, states[k])
            _check_picture(ctx, states[k])  # the estimate moved nothing
    if jit:
        assert ctx.jit_state() == gpu.FR_JIT_USED
    ctx.close()


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_accumulation(gpu, case):
    _accumulate(gpu, case, True)


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_accumulation_with_the_error_estimate(gpu, case):
    _accumulate(gpu, case, "error")


def test_deferred_12_byte_records(gpu, monkeypatch):
    monkeypatch.setenv("FR_DEFER", "1")
    _accumulate(gpu, N.SMALL["inf"], "error")


def test_scene_kernel(gpu):
    _accumulate(gpu, N.SMALL["nan"], "error", jit="wait")


def test_streamed_frames(gpu):
    _accumulate(gpu, N.SMALL["-inf"], "error", stream=True)


@pytest.mark.parametrize("colour", ["inf", "2^17"])
def test_threshold_sweep(gpu, colour):
    case = N.SMALL[colour]
    st = N.states(case)[-1]
    sc, cam = _scene(gpu, case)
    ctx = gpu.RenderContext(0)
    for k in range(len(case.spps)):
        ctx.render(sc, cam, _params(gpu, case, k, "error"))
    counts = []
    for thr in N.SWEEP:
        got = ctx.accum_error(thr)
        _check_summary(got, st, thr)
        counts.append(got["converged"])
    assert counts[0] == int(np.count_nonzero(st["rel"] == 0))  # with every non-finite pixel among them
    assert counts[-1] == W * H and counts == sorted(counts) and counts[0] < counts[2] < W * H
    ctx.close()


def _check_adapt(ctx, step, threshold, min_samples):
    _check_info(ctx.adapt(threshold, min_samples), step["summary"])
    rel = ctx.download_error()
    assert not np.isnan(rel).any() and N.same_bits(rel, step["rel"])
    n, k = ctx.download_counts()
    assert np.array_equal(n, step["n"]) and np.array_equal(k, step["k"])  # each tile's n and K


@pytest.mark.parametrize("case,min_samples", [(c, 0) for c in N.ADAPT] + [(N.SMALL["inf"], 3)],
                         ids=lambda x: N.case_id(x) if isinstance(x, tuple) else f"min{x}")
def test_adaptive_flow(gpu, case, min_samples):
    """F F A F F A: the selection over an estimate with non-finite pixels, and adaptive frames
    that leave the inactive tiles' non-finite pixels as they are. min_samples 3 is above the
    n = 2 of the first adapt: every tile is active whatever its estimate."""
    steps = N.flow(case, T, min_samples)
    sc, cam = _scene(gpu, case)
    ctx = gpu.RenderContext(0)
    frame = 0
    for step in steps:
        if step["op"] == "A":
            _check_adapt(ctx, step, T, min_samples)
            continue
        before = ctx.download(W, H)[0] if frame else None
        ctx.render(sc, cam, _params(gpu, case, frame, step["mode"]))
        stats = ctx.sync()
        mean, u8 = ctx.download(W, H)
        assert N.same_bits_nan(mean, step["mean"]), frame
        assert np.array_equal(u8, _to_u8(step["mean"]))
        assert ctx.accum_info() == (step["frames"], step["samples"])
        assert stats["samples"] == step["traced"] * step["spp"]
        if step["mode"] == "adaptive":  # the device's own pixels outside the list did not move
            idle = ~np.repeat(np.repeat(step["mask"], 8, 0), 8, 1)
            assert idle.any() or min_samples
            assert N.same_bits_nan(mean[idle], before[idle])
        frame += 1
    ctx.close()


def _check_denoised(ctx, den):
    mean, u8, var = ctx.download_denoised(W, H, want_var=True)
    assert N.same_bits_nan(mean, den.mean), int(np.count_nonzero(N.bits(mean) != N.bits(den.mean)))
    assert np.array_equal(u8, den.u8)
    assert not np.isnan(var).any() and not np.signbit(var).any()
    assert N.same_bits(var, den.var), int(np.count_nonzero(N.bits(var) != N.bits(den.var)))
    inv = ~den.valid  # as prep left them, the sign bit off
    assert N.same_bits_nan(mean[inv], den.prep_mean[inv]) and N.same_bits(var[inv], den.prep_var[inv])
    assert not np.isnan(mean[den.valid]).any()


@pytest.mark.parametrize("case", N.DENOISE, ids=N.case_id)
def test_denoise(gpu, case):
    states = N.states(case)
    sc, cam = _scene(gpu, case)
    ctx = gpu.RenderContext(0)
    for k in range(4):
        ctx.render(sc, cam, _params(gpu, case, k, "error"))
        if k in (1, 3):
            for levels in N.LEVELS:
                ctx.denoise(levels)
                _check_denoised(ctx, N.denoised(case, k, levels))
            ctx.sync()  # the frames' own outputs, the counts and the estimate are as they were
            _check_picture(ctx, states[k])
            _check_error(ctx, states[k])
            _check_denoised(ctx, N.denoised(case, k, N.LEVELS[-1]))  # and the denoised image is still there
    ctx.close()


def test_denoise_of_a_tiled_accumulation(gpu):
    """Two uniform frames, adapt, two adaptive frames, denoise: prep reads each tile's n and K
    over NaN pixels, some in tiles that stayed behind."""
    case = N.SMALL["nan"]
    steps = N.flow(case)
    last = steps[-1]
    with np.errstate(all="ignore"):
        want = D.denoise(last["a"], last["q"], last["n"], last["k"])
        pm, pv, valid = D.prep(last["a"], last["q"], last["n"], last["k"])
        uniform = D.denoise(last["a"], last["q"], int(last["n"].max()), int(last["k"].max()))
    assert len(np.unique(last["n"])) == 2 and not N.same_bits_nan(want[0], uniform[0])  # the tiles' own counts show
    sc, cam = _scene(gpu, case)
    ctx = gpu.RenderContext(0)
    frame = 0
    for step in steps[:-1]:
        if step["op"] == "A":
            assert ctx.adapt(T)["active_tiles"] == step["summary"]["active_tiles"]
        else:
            ctx.render(sc, cam, _params(gpu, case, frame, step["mode"]))
            frame += 1
    ctx.denoise()
    _check_denoised(ctx, N.Denoised(want[0], want[1], want[2], valid, pm, pv))
    n, k = ctx.download_counts()
    assert np.array_equal(n, last["n"]) and np.array_equal(k, last["k"])
    ctx.close()


def test_two_shards_equal_one_context(gpu):
    case = N.SMALL["inf"]
    states = N.states(case)
    sc, cam = _scene(gpu, case)
    m = gpu.MultiContext([0, 0])
    for k, spp in enumerate(case.spps):
        m.render(sc, cam, _params(gpu, case, k, "error"))
        _check_counters(m.sync(), states[k], spp)
        mean, u8 = m.frame()
        assert N.same_bits_nan(mean, states[k]["mean"]) and np.array_equal(u8, states[k]["u8"]), k
        if k == 0:
            continue
        got, rel = m.accum_error(T, want_map=True)
        assert not np.isnan(rel).any() and N.same_bits(rel, states[k]["rel"]), k  # the stitched map
        _check_summary(got, states[k], T)
        parts = [m.context(i).accum_error(T) for i in range(2)]
        assert [p["pixels"] for p in parts] == [W * H // 2] * 2
        assert got["converged"] == sum(p["converged"] for p in parts)
    mask, info = N.select(states[-1])
    _check_info(m.adapt(T, 0), info)
    rel = np.full((H, W), np.nan, F)
    for i in range(2):
        m.context(i).download_error(rel)
    assert N.same_bits(rel, states[-1]["rel"])
    strips = [np.arange(i, H // 8, 2) for i in range(2)]  # a shard's strips: every second one
    assert [m.context(i).adapt(T, 0)["active_tiles"] for i in range(2)] == [int(mask[s].sum()) for s in strips]
    m.close()


def test_a_restart_forgets_non_finite_accumulators(gpu):
    """accum_reset over A and Q that hold NaN and inf: the next accumulation starts from S alone
    (A = S, Q = S^2 / spp, no 0 * old or old - old), so its first frame is the plain render and
    its second frame's estimate is the fresh accumulation's."""
    case = N.SMALL["-inf"]
    states = N.states(case)
    sc, cam = _scene(gpu, case)
    ctx = gpu.RenderContext(0)
    for k in (2, 3):  # other frames of the same view first: NaN, +inf and -inf where frames 0 and 1 have none
        ctx.render(sc, cam, _params(gpu, case, k, "error"))
    ctx.sync()
    dirty = ~np.isfinite(ctx.download(W, H)[0]).all(-1)
    assert np.array_equal(dirty, N.restart_dirty(case)) and (dirty & np.isfinite(states[1]["mean"]).all(-1)).any()
    ctx.accum_reset()
    assert ctx.accum_info() == (0, 0)
    for k in (0, 1):
        ctx.render(sc, cam, _params(gpu, case, k, "error"))
        _check_counters(ctx.sync(), states[k], case.spps[k])
        _check_picture(ctx, states[k])
        if k == 0:
            plain, plain_u8, _ = gpu.render(sc, cam, W, H, case.spps[0], case.depth, seed=N.seed_of(case, 0))
            mean, u8 = ctx.download(W, H)
            assert N.same_bits_nan(mean, plain) and np.array_equal(u8, plain_u8)
    _check_error(ctx, states[1])
    ctx.close()
