"""Adaptive sampling (FR_FLAG_ADAPTIVE, include/forma_rt.h) restated in numpy f32 on top of
tests/accum_error_ref.py: per-tile counts n and K, frames that update masked tiles only, rel per
distinct (n, K), and fr_ctx_adapt's selection and summary. Also the cases the GPU tests run and
the flow they share, so the host test can hold every case's condition on the oracle alone.
Shared by tests/test_adaptive.py and tests/test_adaptive_host.py; not a test module.

Tiles are the image's 8x8 tiles, [strip, column]: a shard's tiles are its strips' rows of this
array, so the whole-image arrays describe one context and a stitched MultiContext alike."""
import functools

import numpy as np

from tests import accum_error_ref as R

F = np.float32
SEED0 = 0xADA0
FLOW = "FFAFFAFA"  # F: a frame (seed SEED0 + k for the k-th frame), A: an adapt call


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


class AdaptiveComposite:
    """The expected A, Q, per-tile n and K, mean, and what fr_ctx_adapt reports."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.shape = ((h + 7) // 8, (w + 7) // 8)
        self.a = self.q = self.mean = None
        self.n = np.zeros(self.shape, np.uint32)
        self.k = np.zeros(self.shape, np.uint32)
        self.frames = self.samples = 0  # the host's totals

    def pixels(self, tiles):
        """A per-tile array spread over the tiles' image pixels: [H, W]."""
        return np.repeat(np.repeat(tiles, 8, 0), 8, 1)[:self.h, :self.w]

    def add(self, s, spp, mask=None):
        """A frame of per-pixel sum s [H, W, 3] over the tiles of `mask` (None: every tile).
        Returns the mean image: A / n_t in masked tiles, as it was elsewhere."""
        mask = np.ones(self.shape, bool) if mask is None else np.asarray(mask, bool)
        if not mask.any():
            return self.mean  # an empty list: nothing moves, the totals included
        t = R.sq_term(s, spp)
        if self.a is None:
            assert mask.all()
            self.a, self.q = s.astype(F).copy(), t
            self.mean = np.zeros_like(self.a)
        else:
            pm = self.pixels(mask)
            self.a = np.where(pm[..., None], (self.a + s).astype(F), self.a)
            self.q = np.where(pm[..., None], (self.q + t).astype(F), self.q)
        self.n = np.where(mask, self.n + np.uint32(spp), self.n).astype(np.uint32)
        self.k = np.where(mask, self.k + np.uint32(1), self.k).astype(np.uint32)
        self.frames += 1
        self.samples += spp
        pm = self.pixels(mask)
        with np.errstate(all="ignore"):
            mean = (self.a / self.pixels(self.n).astype(F)[..., None]).astype(F)
        self.mean = np.where(pm[..., None], mean, self.mean)
        return self.mean

    def rel(self):
        """rel [H, W], each pixel with its tile's (n, K): evaluated once per distinct pair."""
        out = np.zeros((self.h, self.w), F)
        pn, pk = self.pixels(self.n), self.pixels(self.k)
        for n, k in sorted({(int(n), int(k)) for n, k in zip(self.n.ravel(), self.k.ravel())}):
            sel = (pn == n) & (pk == k)
            out[sel] = R.rel_error(self.a, self.q, n, k)[sel]
        return out

    def select(self, threshold, min_samples=0, rows=None):
        """(tile mask, summary) of fr_ctx_adapt: a tile is active iff the maximum of rel over its
        image pixels is > threshold as uint32 bits, or its n < min_samples. rows: the image rows
        of one shard (the summary then counts that shard alone; the mask stays whole)."""
        rel = self.rel()
        tmax = np.zeros(self.shape, np.uint32)
        for s in range(self.shape[0]):
            for c in range(self.shape[1]):
                tmax[s, c] = _bits(rel[8 * s:8 * s + 8, 8 * c:8 * c + 8]).max()
        mask = (tmax > _bits(F(threshold))) | (self.n < np.uint32(min_samples))
        pm = self.pixels(mask)
        strips = np.arange(self.shape[0]) if rows is None else np.unique(np.asarray(rows) // 8)
        rr = slice(None) if rows is None else rows
        summary = {"frames": self.frames, "samples": self.samples,
                   "tiles": int(len(strips) * self.shape[1]), "active_tiles": int(mask[strips].sum()),
                   "pixels": int(rel[rr].size), "active_pixels": int(pm[rr].sum()),
                   "converged": int(np.count_nonzero(rel[rr] <= F(threshold))), "max_rel": F(rel[rr].max()),
                   "threshold": F(threshold), "min_samples": int(min_samples)}
        return mask, summary


# ---- the cases of tests/test_adaptive.py ------------------------------------------------------
# name: (scene key, w, h, depth, spp, threshold, min_samples). A threshold is a condition, not a
# measurement: at the first adapt of FLOW the reference gives 0 < active_tiles < tiles
# (tests/test_adaptive_host.py holds that for every case on the oracle).
INF = float("inf")
CASES = {
    "scene08_16": ("scene_08", 33, 17, 8, 16, 2.0 ** -3, 0),  # nibble list kernel, sum_nib_kernel
    "scene08_4": ("scene_08", 33, 17, 8, 4, 2.0 ** -3, 0),    # sum_kernel<2>
    "scene01_2": ("scene_01", 33, 17, 8, 2, 0.75, 0),         # planes, 12-B records, sum_kernel<3>
    "builtin0_4": ("builtin0", 32, 24, 50, 4, 2.0 ** -2, 0),  # colour records, MAXD = 0
    "cubes100_16": ("cubes100", 33, 17, 8, 16, 2.0 ** -3, 0),  # BVH family; ends on the empty list
    "scene08_32": ("scene_08", 33, 17, 8, 32, 2.0 ** -4, 0),  # two blocks, sub-block items over a compact P
    "scene08_64": ("scene_08", 33, 17, 8, 64, 2.0 ** -5, 0),  # FR_PIPELINE=2: multi-pass
    "cubes100_zero": ("cubes100", 33, 17, 8, 16, 0.0, 0),     # exactly the tiles with a pixel of rel > 0
}


@functools.lru_cache(maxsize=None)
def reference_flow(key, w, h, depth, spp, threshold, min_samples, flow=FLOW, uniform_from=None):
    """The expected state after every step of `flow`: a list of dicts, for an F {"op": "F",
    "seed", "mode" ("error" or "adaptive"), "mask" (the tiles traced), "mean", "frames",
    "samples", "traced" (image pixels traced)}, for an A {"op": "A", "mask", "summary", "rel",
    "n", "k" (per-pixel count maps)}. Frames before the first A are plain accumulating frames;
    after it adaptive ones, except from frame index `uniform_from` on (plain accumulating frames
    in the tiled accumulation)."""
    from tests.test_accumulate import _frame_sum, _oracle_frame
    comp = AdaptiveComposite(w, h)
    mask, out, k = None, [], 0
    for op in flow:
        if op == "F":
            uniform = mask is None or (uniform_from is not None and k >= uniform_from)
            m = None if uniform else mask
            omean, _, _, _ = _oracle_frame(key, w, h, spp, depth, SEED0 + k)
            mean = comp.add(_frame_sum(omean, spp), spp, m)
            traced = w * h if m is None else int(comp.pixels(m).sum())
            out.append({"op": "F", "seed": SEED0 + k, "mode": "error" if uniform else "adaptive",
                        "mask": np.ones(comp.shape, bool) if m is None else m.copy(), "mean": mean.copy(),
                        "frames": comp.frames, "samples": comp.samples, "traced": traced})
            k += 1
        else:
            mask, summary = comp.select(threshold, min_samples)
            out.append({"op": "A", "mask": mask.copy(), "summary": summary, "rel": comp.rel(),
                        "n": comp.pixels(comp.n).copy(), "k": comp.pixels(comp.k).copy()})
    return out
