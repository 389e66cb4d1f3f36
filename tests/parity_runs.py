"""Renders of one fixture through the trace-kernel families, compared with the oracle bit for
bit: the helper tests/test_ray_edges.py and tests/test_magnitude.py share."""
import numpy as np

from tests.test_gpu_parity import _same_bits, assert_parity
from tests.test_scene_jit import _ctx_render

ENV = ("FR_DEFER", "FR_MAT", "FR_BVH")


class Runs:
    """Renders of one fixture; every mismatch is collected, so one failing case shows every
    kernel family that deviates. `reference(variant, depth)` gives the oracle's (prims, mean,
    u8, counters); `frame` is (width, height, spp, seed)."""

    def __init__(self, gpu, monkeypatch, key, cam, reference, frame):
        self.gpu, self.mp, self.key, self.errors = gpu, monkeypatch, key, []
        self.cam, self.reference, self.frame = cam, reference, frame

    def render(self, prims, depth, env=None, jit=False):
        for e in ENV:
            self.mp.delenv(e, raising=False)
        if env:
            self.mp.setenv(*env)
        w, h, spp, seed = self.frame
        sc = self.gpu.Scene.from_prims(prims)  # a fresh scene: FR_BVH acts when the scene is uploaded
        if jit:
            mean, u8, st, info = _ctx_render(self.gpu, sc, self.cam, w, h, spp, depth, seed=seed)
            if not info["used"]:
                self.errors.append(f"scene kernel not used: {info}")
            return mean, u8, st
        return self.gpu.render(sc, self.cam, w, h, spp, depth, seed=seed)

    def check(self, tag, got, want):
        mean, u8, st = got
        omean, ou8, ocnt = want
        try:
            if np.isfinite(omean).all():  # (the distance of two infinities is NaN: the bits below decide)
                assert_parity(mean, u8, st, omean, ou8, ocnt)
            assert _same_bits(mean, omean), f"mean bits differ in {int((mean.view(np.uint32) != omean.view(np.uint32)).any(axis=2).sum())} pixels"
            assert np.array_equal(u8, ou8), "u8 differs"
            for k in ("segments", "hits", "scatters"):
                assert st[k] == ocnt[k], f"{k}: {st[k]} != {ocnt[k]}"
        except AssertionError as e:
            self.errors.append(f"{tag}: {str(e).splitlines()[0] if str(e) else 'assertion failed'}")

    def against_oracle(self, variant, depth, env=None, jit=False):
        prims, omean, ou8, ocnt = self.reference(variant, depth)
        got = self.render(prims, depth, env, jit)
        self.check(f"{variant} depth {depth} {env or ''}{' scene kernel' if jit else ''}", got, (omean, ou8, ocnt))
        return got

    def done(self):
        assert not self.errors, f"{self.key}:\n  " + "\n  ".join(self.errors)
