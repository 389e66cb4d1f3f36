"""Magnitude-edge parity: tiny, huge and denormal ray directions, scaled scenes, far cameras
and extreme attenuations through every trace-kernel family, against the oracle bit for bit.

The hot path's cheaper sequences (recip_nr, div_rn, sqrt_core, the clamped box reciprocal,
the padded BVH cull, the deferred sum's skipped unwind) hold only inside range guards, and
every frame elsewhere in the suite stays inside all of them: directions of order 1, scenes of
order 1..100, colours in [0.1, 1]. The fixtures of tests/magnitude_fixtures.py leave each
guard with every lane of a wave and with some lanes of a wave, in the kernels that ship (the
compiled specialisations, the scene kernel built at run time, the BVH walk), not in the
self-test instantiation. tests/test_magnitude_fixtures.py checks, without a GPU, that each
fixture leaves the guard it names in the oracle.

The kernel families per (scene, size, fixture) are those of tests/test_ray_edges.py. Each render
must equal the oracle's in the mean's bits (NaN equal to NaN), the u8 image and the segment,
hit and scatter counters: there is no tolerance. 823 cases of 1024 samples each take
47 s on an MI355X with a cold scene-kernel cache, 25 s warm (the edge-ray file: 256 cases, 13 s)."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import magnitude_fixtures as M
from tests.parity_runs import Runs
from tests.test_gpu_parity import _same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,size,name", M.cases())
def test_magnitude_edges_match_the_oracle(gpu, kind, size, name, monkeypatch):
    fx = M.fixture(kind, size, name)
    r = Runs(gpu, monkeypatch, (kind, size, name), M.cameras(gpu, fx)[0],
             lambda variant, depth: M.reference(gpu, kind, size, variant, name, depth), M.frame(fx) + (M.SEED,))
    if size == "big":
        prims = M.scene(kind, size, fx)
        assert M.bvh_cost(prims) >= 48 and len(prims) >= 48  # so the product takes the BVH path (M5: up to its reach)
        for depth in (8, 12):  # u16 stack; u32 stack
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


@pytest.mark.parametrize("kind,size,name", [("box", "small", "M1_k-49"), ("mixed", "mid", "M2_cross2^-100"),
                                            ("sphere", "small", "M3_s-30"), ("box", "big", "M3_s21")])
def test_magnitude_edges_through_save_image_mt(gpu, kind, size, name):
    """The MT kernels are their own instantiations (in-order loop, no deferred unwind): one
    fixture of M1, the M2 crossing and M3 through the four row bands, against the oracle's
    render_mt."""
    fx = M.fixture(kind, size, name)
    cam, ocam = M.cameras(gpu, fx)
    prims = M.scene(kind, size, fx)
    for depth in (8, 12):
        acc, u8, st = gpu.render(gpu.Scene.from_prims(prims), cam, M.W, M.H, M.SPP, depth, seed=M.SEED, mt_bands=True)
        oacc, ou8, ocnt = O.render_mt(prims, ocam, M.W, M.H, M.SPP, depth, M.SEED)
        assert ocnt["hits"] > 0
        assert _same_bits(acc, oacc) and np.array_equal(u8, ou8)
        assert (st["segments"], st["hits"], st["scatters"]) == (ocnt["segments"], ocnt["hits"], ocnt["scatters"])
