"""The cases of tests/nonfinite_fixtures.py reach the classes of pixels they are named for.

Checked on the oracle's frames and the numpy references alone (no GPU): after the last frame
of a case its accumulators hold the infinities, NaNs, over-the-cap, negative or denormal values
the case exists for, next to ordinary pixels; the error estimate is 0 on every non-finite pixel
and divides the image at the case's threshold; fr_ctx_adapt's selection leaves tiles with
non-finite pixels inactive; the denoise has valid pixels whose taps meet invalid ones. These
are conditions, not measurements: tests/test_nonfinite_accum.py compares the device with the
same states, and a case that did not reach its class would compare nothing."""
import numpy as np
import pytest

from tests import accum_error_ref as R
from tests import denoise_ref as D
from tests import nonfinite_fixtures as N

F = np.float32
DENORMAL = F(2.0 ** -126)  # the least normal f32


def _px(mask):
    """Pixels with the property in any channel."""
    return int(np.count_nonzero(mask.any(-1) if mask.ndim == 3 else mask))


def _msum(st):
    """The summed channel mean the estimate's finiteness test and floor look at."""
    with np.errstate(all="ignore"):
        m, _ = R.variance(st["a"], st["q"], st["n"], st["frames"])
        return ((m[..., 0] + m[..., 1]).astype(F) + m[..., 2]).astype(F)


def _tiles(pixels):
    return {(int(y) // 8, int(x) // 8) for y, x in zip(*np.nonzero(pixels))}


def test_the_case_lists():
    assert len(set(N.CASES)) == len(N.CASES)
    assert set(N.SMALL) == {"2^-18", "2^17", "negative", "inf", "nan", "-inf"}
    assert all(c in N.CASES for c in N.DENOISE + N.ADAPT)
    assert all(len(c.spps) == 4 and set(c.spps) == {1} for c in N.DENOISE + N.ADAPT)
    assert {c.spps[0] for c in N.CASES} == {1, 4, 16}
    assert all(c.spps == (1,) * 4 for c in N.CASES if c.colour == "2^-18")  # denormal samples need spp 1
    assert "-inf" not in dict(N.M.M6_COLOURS) and len(N.M.M6_COLOURS) == 6  # M6's own list is as it was


def test_comparison_helpers():
    nan, other = F(np.nan), np.array([0xFFC00001], np.uint32).view(F)[0]  # a NaN of another sign and payload
    a = np.array([1.0, 0.0, nan, np.inf], F)
    assert N.same_bits_nan(a, np.array([1.0, 0.0, other, np.inf], F))
    assert not N.same_bits(a, np.array([1.0, 0.0, other, np.inf], F))
    assert not N.same_bits_nan(a, np.array([1.0, -0.0, nan, np.inf], F))  # the sign of a zero counts
    assert not N.same_bits_nan(a, np.array([1.0, 0.0, nan, nan], F))  # inf is not NaN
    assert not N.same_bits_nan(a, np.array([1.0, 0.0, 0.0, np.inf], F))
    tiny = np.array([2.0 ** -140], F)
    assert not N.same_bits(tiny, np.zeros(1, F)) and not N.same_bits_nan(tiny, np.zeros(1, F))  # a flushed denormal


def test_frame_sum_is_nan_aware_and_strict():
    mean = np.array([[[np.nan, np.inf, -np.inf], [2.0 ** -140, 0.5, -0.0]]], F)
    s = N.frame_sum(mean, 1)
    assert N.same_bits_nan(s, mean) and N.same_bits(s[0, 1], mean[0, 1])
    big = np.array([[[np.nan, np.inf, 3.0]]], F)
    assert N.same_bits_nan(N.frame_sum(big, 16), np.array([[[np.nan, np.inf, 48.0]]], F))
    with pytest.raises(AssertionError):
        N.frame_sum(mean, 4)  # a mean near the subnormals at spp > 1
    with pytest.raises(AssertionError):
        N.frame_sum(np.array([[[1.0, 2.0, 3.0]]], F), 3)


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_case_reaches_its_classes(fr, case):
    states = N.states(case)
    st = states[-1]
    a, q = st["a"], st["q"]
    assert st["frames"] == len(case.spps) >= 3 and st["n"] == sum(case.spps)
    fin_a = np.isfinite(a).all(-1)
    den = N.denoised(case, len(case.spps) - 1)
    if case.colour in ("inf", "-inf"):
        assert _px(np.isinf(a)) >= 16
        if case.kind == "mixed":
            assert _px(np.isnan(a)) >= 16  # inf met 0 or an inf of the other sign
        if case.colour == "-inf":
            assert _px(a == -np.inf) >= 1 and _px(a == np.inf) >= 1
    if case.colour == "nan":
        assert _px(np.isnan(a)) >= 16 and int(fin_a.sum()) >= 16
        assert _px(np.isinf(a)) == 0  # NaN is the only non-finite value of these frames
    if case.colour == "2^17":
        assert int((fin_a & np.isinf(q).any(-1)).sum()) >= 16  # A finite, Q overflowed
        assert _px(a == np.inf) >= 16
        assert int(den.valid.sum()) >= 16
        if case.spps[0] == 1:  # (at spp 16 almost every finite pixel is ordinary or has overflowed: 4 such)
            assert int((fin_a & np.isfinite(q).all(-1) & ~den.valid).sum()) >= 16  # finite, over a cap of the denoise
    if case.colour == "negative":
        assert _px(st["mean"] < 0) >= 16
        if case.kind == "mixed":
            msum = _msum(st)
            assert int((np.isfinite(msum) & (msum < R.FLOOR)).sum()) >= 1  # the floor decides rel
    if case.colour == "2^-18":
        s = [x["s"] for x in states]
        assert sum(_px((np.abs(x) > 0) & (np.abs(x) < DENORMAL)) for x in s) >= 1  # a nonzero denormal channel of S
        with np.errstate(all="ignore"):
            assert sum(_px((x != 0) & ((x * x).astype(F) < DENORMAL)) for x in s) >= 1  # S * S underflows
        assert not _px(~np.isfinite(a)) and den.valid.all()
        one = N.denoised(case, 1, 1)  # one level keeps denormals in both outputs (four average them away)
        assert _px((np.abs(one.mean) > 0) & (np.abs(one.mean) < DENORMAL)) >= 1
        assert _px((one.var > 0) & (one.var < DENORMAL)) >= 1
        assert _px((one.prep_var > 0) & (one.prep_var < DENORMAL)) >= 1
    if case.colour in N.NONFINITE:
        assert _px(~np.isfinite(a)) >= 16
    else:
        assert np.isfinite(a).all() and np.isfinite(q).all()


@pytest.mark.parametrize("case", [c for c in N.CASES if c.colour in N.NONFINITE], ids=N.case_id)
def test_non_finite_pixels_divide_every_stage(fr, case):
    """What the estimate, the selection and the denoise must make of a case with non-finite pixels."""
    for k, st in enumerate(N.states(case)):
        if k == 0:
            continue
        rel = st["rel"]
        assert not np.isnan(rel).any() and (rel >= 0).all() and not np.signbit(rel).any()
        nonfinite = ~np.isfinite(_msum(st))
        assert nonfinite.any() and (N.bits(rel[nonfinite]) == 0).all()  # exactly +0
        # (a non-finite channel of A makes the summed mean non-finite: inf, or NaN where inf meets -inf)
        assert np.array_equal(nonfinite | ~np.isfinite(st["a"]).all(-1), nonfinite)
    st = N.states(case)[-1]
    nonfinite = ~np.isfinite(_msum(st))
    assert 0 < N.summary(st, N.T)["converged"] < N.W * N.H
    assert N.summary(st, 0.0)["converged"] == int(np.count_nonzero(st["rel"] == 0)) >= int(nonfinite.sum())
    assert N.summary(st, float("inf"))["converged"] == N.W * N.H
    mask, info = N.select(st)
    assert 0 < int(mask.sum()) < mask.size and info["active_tiles"] == int(mask.sum())
    assert info["converged"] == N.summary(st, N.T)["converged"]
    if case.size == "small":  # (at depth 8 every tile of the big lattice that holds a non-finite pixel is active)
        assert any(not mask[t] for t in _tiles(nonfinite))
    if case == N.SPP16:
        return  # not denoised: 37 valid pixels
    den = N.denoised(case, len(case.spps) - 1)
    assert den.valid.any() and (~den.valid).any()
    assert not (den.valid & nonfinite).any()
    assert int(N.invalid_tap(den.valid).sum()) >= 32
    assert not np.isnan(den.mean[den.valid]).any() and not np.isnan(den.var).any()
    assert not np.signbit(den.var).any()


@pytest.mark.parametrize("case", N.DENOISE, ids=N.case_id)
def test_denoise_keeps_invalid_pixels_at_every_level_count(fr, case):
    for frame in (1, 3):
        for levels in N.LEVELS:
            den = N.denoised(case, frame, levels)
            inv = ~den.valid
            assert N.same_bits_nan(den.mean[inv], den.prep_mean[inv]) and N.same_bits(den.var[inv], den.prep_var[inv])
            assert not np.isnan(den.mean[den.valid]).any() and not np.isnan(den.var).any()
            assert np.array_equal(den.valid, D.valid_mask(N.states(case)[frame]["a"], N.states(case)[frame]["q"],
                                                          N.states(case)[frame]["n"], N.states(case)[frame]["frames"]))
        # the filter moved valid pixels, and differently per level count (every valid pixel of the
        # 2^17 frames is an exact 0 among invalid ones: there any tap of a neighbour would show)
        if case.colour in ("inf", "nan", "-inf"):
            moved = [N.denoised(case, frame, lv).mean[den.valid].tobytes() for lv in N.LEVELS]
            assert len(set(moved)) == len(moved)


@pytest.mark.parametrize("case", N.ADAPT, ids=N.case_id)
def test_adaptive_flow_leaves_non_finite_tiles_alone(fr, case):
    steps = N.flow(case)
    first, second = [s for s in steps if s["op"] == "A"]
    for a in (first, second):
        assert 0 < a["summary"]["active_tiles"] < a["summary"]["tiles"] == 16
    nonfinite = ~np.isfinite(first["a"]).all(-1)
    idle = [t for t in _tiles(nonfinite) if not first["mask"][t]]
    assert idle  # a tile with non-finite pixels that the adaptive frames must not touch
    frames = [s for s in steps if s["op"] == "F"]
    assert [f["mode"] for f in frames] == ["error", "error", "adaptive", "adaptive"]
    assert 0 < frames[2]["traced"] < N.W * N.H
    for t in idle:
        rows, cols = slice(8 * t[0], 8 * t[0] + 8), slice(8 * t[1], 8 * t[1] + 8)
        assert N.same_bits_nan(frames[3]["mean"][rows, cols], frames[1]["mean"][rows, cols])
    assert len(np.unique(second["tile_n"])) == 2 and len(np.unique(second["tile_k"])) == 2
    # min_samples above n: every tile is active whatever its estimate
    forced = N.flow(case, N.T, 3)
    assert [s["summary"]["active_tiles"] for s in forced if s["op"] == "A"][0] == 16


def test_the_restart_case_has_pixels_to_forget(fr):
    """Frames 2 and 3 of the -inf case leave non-finite values where the accumulation of frames
    0 and 1 is finite: a restart that cleared the old A or Q by arithmetic (0 * old, old - old)
    would show there. One such pixel decides; a handful is asked for."""
    case = N.SMALL["-inf"]
    dirty = N.restart_dirty(case)
    fresh = np.isfinite(N.states(case)[1]["mean"]).all(-1)
    assert int((dirty & fresh).sum()) >= 8 and int((dirty & np.isfinite(N.states(case)[0]["mean"]).all(-1)).sum()) >= 8
