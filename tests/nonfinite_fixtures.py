"""Fixtures for the non-finite and out-of-range pixels of a progressive accumulation
(tests/test_nonfinite_accum.py): frames whose pixels are inf, -inf, NaN, negative, huge or
denormal, accumulated, estimated, selected and denoised.

tests/test_magnitude.py holds a single plain frame of the M6 family (colours of 2^-18, 2^17,
negative, inf and NaN on the lattices of tests/magnitude_fixtures.py, 32 x 32 pixels of one
sample) to the oracle bit for bit in every trace-kernel family. Here the same scenes and camera
are accumulated: frame k of a case has seed SEED0 + k (seed_of), and what the resolve, the
error estimate, fr_ctx_adapt and fr_ctx_denoise must make of such frames is rebuilt from the
oracle's frames with the numpy restatements of the headers (tests/accum_error_ref.py, tests/adaptive_ref.py,
tests/denoise_ref.py, which the host tests hold against the headers' own bits).

A case is (kind, size, colour, depth, spps). Most have one sample per pixel: the oracle's mean
then is the frame's sum S itself, a denormal sample survives, and nothing has to be argued
about S = mean * spp. The few cases of spp 4 and 16 exist for the other resolve kernels
(sum_kernel<2>, sum_nib_kernel, the BVH family's attenuation-class table).

tests/test_nonfinite_fixtures.py checks, on the oracle and the references alone, that every
case reaches the classes of pixels it is named for. Not a test module."""
import functools
from collections import namedtuple

import numpy as np

from oracle import oracle_py as O
from tests import accum_error_ref as R
from tests import adaptive_ref as AR
from tests import denoise_ref as D
from tests import magnitude_fixtures as M
from tests.test_accumulate import _to_u8

F = np.float32
SEED0 = 0xE220
W = H = 32
T = 2.0 ** -3  # the threshold the cases are summarised and selected at
FLT_MAX = float(np.finfo(F).max)
SWEEP = (0.0, 2.0 ** -5, 2.0 ** -3, FLT_MAX, float("inf"))
LEVELS = (1, 4, 6)

# M6's colours (without -0.0, which is an ordinary pixel after the trace) and one of this
# module's own: a green component of -inf, so that +inf and -inf meet in one accumulator
COLOURS = {name: kw for name, kw in M.M6_COLOURS if name != "neg0"}
COLOURS["-inf"] = dict(one=-np.inf)
NONFINITE = ("inf", "-inf", "nan", "2^17")  # the colours that leave non-finite pixels

Case = namedtuple("Case", "kind size colour depth spps")


def _case(kind, size, colour, depth=8, spps=(1, 1, 1, 1)):
    return Case(kind, size, colour, depth, tuple(spps))


SMALL = {c: _case("mixed", "small", c) for c in COLOURS}  # every colour, four frames of one sample
# A pixel's mean stays negative only while the few samples that met the negative colour an odd
# number of times outweigh the others: on the mixed lattice 39 pixels after one frame and 6 after
# four at SEED0 and depth 8. Depth 12 with these seeds keeps 17 (the condition asks for 16); the
# box lattice, whose first lambertian box fills half the frame, keeps 498.
SMALL["negative"] = _case("mixed", "small", "negative", 12)
SEEDS = {SMALL["negative"][:4]: 0xE2C4}  # (kind, size, colour, depth): the first frame's seed where it is not SEED0
NEGATIVE_BOX = _case("box", "small", "negative")
BOX = {c: _case("box", "small", c, 12) for c in ("inf", "nan", "2^17")}  # u32 stack
BIG = {c: _case("mixed", "big", c) for c in ("inf", "nan", "2^17")}  # the BVH family
SPP4 = _case("mixed", "small", "inf", spps=(4,) * 3)  # sum_kernel<2>
SPP16 = _case("mixed", "small", "2^17", spps=(16,) * 3)  # sum_nib_kernel
SPP16_BIG = _case("mixed", "big", "nan", spps=(16,) * 3)  # sum_nib_kernel over the class table
CASES = list(SMALL.values()) + list(BOX.values()) + list(BIG.values()) + [SPP4, SPP16, SPP16_BIG, NEGATIVE_BOX]
# the cases fr_ctx_denoise runs on (2^17 at spp 16 keeps too few valid pixels to say much)
DENOISE = [SMALL[c] for c in ("inf", "nan", "-inf", "2^17", "2^-18", "negative")] + [BIG["nan"]]
ADAPT = [SMALL[c] for c in ("inf", "nan", "2^17")]


def case_id(case):
    return f"{case.kind}-{case.size}-{case.colour}-d{case.depth}-spp{case.spps[0]}x{len(case.spps)}"


def prims(case):
    return M.coloured(M.lattice(case.kind, case.size), **COLOURS[case.colour])


def cameras(fr):
    """(FrCamera, OrCamera): M6's camera at 32 x 32."""
    return M.edge_camera(fr, w=W, h=H, **M.M6_CAM)


# ---- comparisons ----------------------------------------------------------------------

def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same_bits(a, b):
    """Strictly bit for bit: for what the contract says is never NaN."""
    return np.array_equal(bits(a), bits(b))


def same_bits_nan(a, b):
    """NaN equal to NaN of any payload and sign (the device's default NaN and numpy's differ in
    sign), everything else bit for bit: tests/test_gpu_parity._same_bits."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b))))


# ---- oracle frames and expected states ------------------------------------------------

def frame_sum(mean, spp):
    """S = mean * spp in f32 from the oracle's mean of a frame. S / spp must give the mean back
    bit for bit (NaN for NaN); for spp > 1 no finite nonzero |mean| may be under 2^-100, where
    the oracle's own division could have lost bits of S to a denormal."""
    assert spp & (spp - 1) == 0
    with np.errstate(all="ignore"):
        s = (mean * F(spp)).astype(F)
        back = (s / F(spp)).astype(F)
    nan = np.isnan(mean)
    assert np.array_equal(np.isnan(back), nan) and np.array_equal(bits(back)[~nan], bits(mean)[~nan])
    if spp > 1:
        small = np.abs(mean[np.isfinite(mean) & (mean != 0)])
        assert small.size == 0 or float(small.min()) >= 2.0 ** -100
    return s


@functools.lru_cache(maxsize=None)
def oracle_frame(kind, size, colour, depth, spp, seed):
    """(mean, u8, counters) of one oracle frame, computed once and shared read-only."""
    import forma_rt
    case = Case(kind, size, colour, depth, ())
    mean, u8, cnt, rows = O.render(prims(case), cameras(forma_rt)[1], W, H, spp, depth, seed=seed)
    assert rows == H
    mean.setflags(write=False)
    u8.setflags(write=False)
    return mean, u8, cnt


def seed_of(case, k):
    return SEEDS.get(case[:4], SEED0) + k


def frame_of(case, k):
    return oracle_frame(case.kind, case.size, case.colour, case.depth, case.spps[k], seed_of(case, k))


@functools.lru_cache(maxsize=None)
def states(case):
    """The expected state after every frame of a case: a list of dicts of a, q, n, frames, mean,
    u8, s (the frame's own sum), counters (the frame's own, the oracle's) and, from the second
    frame on, rel. Computed once; the arrays are read-only."""
    comp = R.ErrorComposite()
    out = []
    for k, spp in enumerate(case.spps):
        omean, _, cnt = frame_of(case, k)
        s = frame_sum(omean, spp)
        with np.errstate(all="ignore"):
            mean = comp.add(s, spp)
            st = {"a": comp.a.copy(), "q": comp.q.copy(), "n": comp.n, "frames": comp.frames, "mean": mean,
                  "u8": _to_u8(mean), "s": s, "counters": cnt, "rel": comp.rel() if comp.frames >= 2 else None}
        for x in st.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        out.append(st)
    return out


def restart_dirty(case):
    """[H, W] bool: the pixels that an accumulation of frames 2 and 3 alone leaves non-finite
    (what the restart test fills the accumulators with before accum_reset)."""
    st = states(case)
    with np.errstate(all="ignore"):
        return ~np.isfinite((st[2]["s"] + st[3]["s"]).astype(F)).all(-1)


def summary(state, threshold):
    """What fr_ctx_accum_error reports for a state."""
    rel = state["rel"]
    return {"frames": state["frames"], "samples": state["n"], "pixels": int(rel.size),
            "converged": int(np.count_nonzero(rel <= F(threshold))), "max_rel": F(rel.max())}


def composite(state):
    """The state as an untiled AdaptiveComposite: every tile with the uniform n and K."""
    comp = AR.AdaptiveComposite(W, H)
    comp.a, comp.q, comp.mean = state["a"].copy(), state["q"].copy(), state["mean"].copy()
    comp.n[:], comp.k[:] = state["n"], state["frames"]
    comp.frames, comp.samples = state["frames"], state["n"]
    return comp


def select(state, threshold=T, min_samples=0):
    """(tile mask, summary) of fr_ctx_adapt on a state."""
    with np.errstate(all="ignore"):
        return composite(state).select(threshold, min_samples)


Denoised = namedtuple("Denoised", "mean u8 var valid prep_mean prep_var")


@functools.lru_cache(maxsize=None)
def denoised(case, frame, levels=D.LEVELS):
    """fr_ctx_denoise after frame index `frame` of a case, with prep's own mean, variance and
    validity beside it. Computed once; read-only."""
    st = states(case)[frame]
    with np.errstate(all="ignore"):
        pm, pv, valid = D.prep(st["a"], st["q"], st["n"], st["frames"])
        mean, u8, var = D.denoise(st["a"], st["q"], st["n"], st["frames"], levels)
    out = Denoised(mean, u8, var, valid, pm, pv)
    for x in out:
        x.setflags(write=False)
    return out


def invalid_tap(valid, step=1):
    """[H, W] bool: the valid pixels with an invalid pixel among their 5 x 5 taps at `step`."""
    seen = np.zeros(valid.shape, bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            seen |= D._shifted(~valid, step * dx, step * dy, False)
    return valid & seen


@functools.lru_cache(maxsize=None)
def flow(case, threshold=T, min_samples=0, steps="FFAFFA"):
    """tests/adaptive_ref.reference_flow over a case's frames: the expected state after every
    step (F: frame k with seed seed_of(case, k), uniform before the first A and adaptive after it;
    A: an adapt call). An A also carries the accumulators and the per-tile counts."""
    comp = AR.AdaptiveComposite(W, H)
    mask, out, k = None, [], 0
    for op in steps:
        with np.errstate(all="ignore"):
            if op == "F":
                spp = case.spps[k]
                mean = comp.add(frame_sum(frame_of(case, k)[0], spp), spp, mask)
                traced = W * H if mask is None else int(comp.pixels(mask).sum())
                out.append({"op": "F", "seed": seed_of(case, k), "spp": spp, "mode": "error" if mask is None else "adaptive",
                            "mask": np.ones(comp.shape, bool) if mask is None else mask.copy(), "mean": mean.copy(),
                            "frames": comp.frames, "samples": comp.samples, "traced": traced})
                k += 1
            else:
                mask, info = comp.select(threshold, min_samples)
                out.append({"op": "A", "mask": mask.copy(), "summary": info, "rel": comp.rel(),
                            "n": comp.pixels(comp.n).copy(), "k": comp.pixels(comp.k).copy(),
                            "a": comp.a.copy(), "q": comp.q.copy(), "tile_n": comp.n.copy(), "tile_k": comp.k.copy()})
    return out
