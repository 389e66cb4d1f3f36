"""Edge-ray parity: exactly axis-parallel rays, origins exactly on a surface and zero
directions through every trace-kernel family, against the oracle bit for bit.

The frames of test_gpu_parity.py come from camera_new / camera_look with jittered pixels
and random bounces, which never produce a direction component that is exactly +0 or -0,
an origin exactly in a box's face plane, on a sphere or on a triangle's edge, or d = 0.
The branches only such rays reach (the box reciprocal's fallback and its +-2^100 clamp, the
NaN-ignoring min / max of the oriented box where 0 inf occurs, the near / far root at
t == 0, sign(0) in the box normal, the scene kernel's compile-time-zero slab coordinate,
the BVH cull on clamped slabs, det == 0 / u == 0 / u + v == 1 in the triangle, the plane's
strict rim) are reached here on purpose, with the cameras and lattice scenes of
tests/ray_edge_fixtures.py. tests/test_ray_edge_fixtures.py checks, without a GPU, that
each fixture reaches its edge in the oracle.

Per (scene, size, family) every kernel family the scene can reach is rendered (names as in
plan.h select_kernel):
  list kernels   8-B records (<= 15 primitives), 12-B records (16..47, or FR_DEFER=1), the
                 unwinding kernel (FR_DEFER=0); box-only, sphere-only and general; with and
                 without a plane; depth 8 (u16 stack) and 12; the general and the diffuse-only
                 shading step (FR_MAT=0 on a diffuse scene gives the same bits)
  BVH kernels    u16 stack (depth 8), u32 stack (12, 50), attenuation-class records,
                 FR_BVH=1 forced on the small lattice; each also equal to its FR_BVH=0 render
  scene kernel   scene_jit="wait" for every list-loop scene (jit_info()["used"])
  mt_bands       the save_image_mt instantiations, against the oracle's render_mt
Each render must equal the oracle's in the mean's bits (NaN equal to NaN), the u8 image
and the segment, hit and scatter counters."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import ray_edge_fixtures as X
from tests.test_gpu_parity import _same_bits, assert_parity
from tests.test_scene_jit import _ctx_render

pytestmark = pytest.mark.gpu
ENV = ("FR_DEFER", "FR_MAT", "FR_BVH")


class _Runs:
    """Renders of one fixture; every mismatch is collected, so one failing case shows every
    kernel family that deviates."""

    def __init__(self, gpu, monkeypatch, kind, size, name):
        self.gpu, self.mp, self.key, self.errors = gpu, monkeypatch, (kind, size, name), []
        self.cam = X.cameras(gpu, X.fixture(kind, name))[0]

    def render(self, prims, depth, env=None, jit=False):
        for e in ENV:
            self.mp.delenv(e, raising=False)
        if env:
            self.mp.setenv(*env)
        sc = self.gpu.Scene.from_prims(prims)  # a fresh scene: FR_BVH acts when the scene is uploaded
        if jit:
            mean, u8, st, info = _ctx_render(self.gpu, sc, self.cam, X.W, X.H, X.SPP, depth, seed=X.SEED)
            if not info["used"]:
                self.errors.append(f"scene kernel not used: {info}")
            return mean, u8, st
        return self.gpu.render(sc, self.cam, X.W, X.H, X.SPP, depth, seed=X.SEED)

    def check(self, tag, got, want):
        mean, u8, st = got
        omean, ou8, ocnt = want
        try:
            if not np.isnan(omean).any():
                assert_parity(mean, u8, st, omean, ou8, ocnt)
            assert _same_bits(mean, omean), f"mean bits differ in {int((mean.view(np.uint32) != omean.view(np.uint32)).any(axis=2).sum())} pixels"
            assert np.array_equal(u8, ou8), "u8 differs"
            for k in ("segments", "hits", "scatters"):
                assert st[k] == ocnt[k], f"{k}: {st[k]} != {ocnt[k]}"
        except AssertionError as e:
            self.errors.append(f"{tag}: {str(e).splitlines()[0] if str(e) else 'assertion failed'}")

    def against_oracle(self, variant, depth, env=None, jit=False):
        kind, size, name = self.key
        prims, omean, ou8, ocnt = X.reference(self.gpu, kind, size, variant, name, depth)
        got = self.render(prims, depth, env, jit)
        self.check(f"{variant} depth {depth} {env or ''}{' scene kernel' if jit else ''}", got, (omean, ou8, ocnt))
        return got

    def done(self):
        assert not self.errors, f"{self.key}:\n  " + "\n  ".join(self.errors)


@pytest.mark.parametrize("kind,size,name", X.cases())
def test_edge_rays_match_the_oracle(gpu, kind, size, name, monkeypatch):
    r = _Runs(gpu, monkeypatch, kind, size, name)
    if size == "big":
        prims = X.lattice(kind, size, X.fixture(kind, name).shift)
        assert X.bvh_cost(prims) >= 48 and len(prims) >= 48  # so the product takes the BVH path
        for depth in (8, 12) + ((50,) if name == "R1_face" else ()):  # u16 stack; u32 stack
            r.against_oracle("full", depth)
            r.against_oracle("full", depth, ("FR_BVH", "0"))  # the in-order loop: the same bits
        r.against_oracle("diffuse", 8)
        for env in (None, ("FR_DEFER", "0"), ("FR_BVH", "0")):  # class records; the unwinding BVH kernel; the loop
            r.against_oracle("classes", 8, env)
    else:
        for depth in (8, 12):
            r.against_oracle("full", depth)
        r.against_oracle("full", 8, ("FR_DEFER", "1"))  # 12-B records
        r.against_oracle("full", 8, ("FR_DEFER", "0"))  # the unwind in the trace kernel
        r.against_oracle("full", 8, jit="wait")
        r.against_oracle("diffuse", 8)
        r.against_oracle("diffuse", 8, ("FR_MAT", "0"))  # the general shading step: the same bits
        r.against_oracle("diffuse", 12)
        if size == "small":  # the BVH kernels on a lattice of ten primitives
            r.against_oracle("full", 8, ("FR_BVH", "1"))
            r.against_oracle("full", 12, ("FR_BVH", "1"))
            r.against_oracle("classes", 8, ("FR_BVH", "1"))
    r.done()


@pytest.mark.parametrize("kind,size", [("box", "small"), ("box", "mid_plane"), ("mixed", "big")])
def test_edge_rays_through_save_image_mt(gpu, kind, size):
    """The MT kernels are their own instantiations (in-order loop, no deferred unwind): the R1
    face-plane fan through the four row bands, against the oracle's render_mt."""
    fx = X.fixture(kind, "R1_face")
    cam, ocam = X.cameras(gpu, fx)
    prims = X.lattice(kind, size, fx.shift)
    for depth in (8, 12):
        acc, u8, st = gpu.render(gpu.Scene.from_prims(prims), cam, X.W, X.H, X.SPP, depth, seed=X.SEED, mt_bands=True)
        oacc, ou8, ocnt = O.render_mt(prims, ocam, X.W, X.H, X.SPP, depth, X.SEED)
        assert ocnt["hits"] * 2 >= ocnt["segments"] or kind != "box"
        assert np.array_equal(acc.view(np.uint32), oacc.view(np.uint32)) and np.array_equal(u8, ou8)
        assert (st["segments"], st["hits"], st["scatters"]) == (ocnt["segments"], ocnt["hits"], ocnt["scatters"])
