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
from tests.parity_runs import Runs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,size,name", X.cases())
def test_edge_rays_match_the_oracle(gpu, kind, size, name, monkeypatch):
    r = Runs(gpu, monkeypatch, (kind, size, name), X.cameras(gpu, X.fixture(kind, name))[0],
             lambda variant, depth: X.reference(gpu, kind, size, variant, name, depth), (X.W, X.H, X.SPP, X.SEED))
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
