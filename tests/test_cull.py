"""The tree's cull on the GPU where the sphere test accepts by rounding error: the fixtures of
tests/cull_fixtures.py through fr_ctx_cast, fr_ctx_gbuffer and the trace kernels, bit for bit
against the oracle.

A ray that passes a small sphere at several radii from far away, or with a direction of 2^-69, is
a hit in the oracle (the discriminant's error exceeds its value), and the product returns the
oracle's closest-hit loop. The rays here start beyond every box padded by 1e-4 (extent + 1) alone
and point away from the scene, so only bounds that hold the test's own error (bvh.h
bvh_sphere_bound) or the tiny-direction rule (kBvhTinyDir, the list) can return those hits.
tests/test_cull_fixtures.py holds the fixtures' conditions in the oracle, tests/test_cull_host.py
walks the same rays through cast.h on the CPU."""
import numpy as np
import pytest

from tests import cast_fixtures as CF
from tests import cull_fixtures as K
from tests import gbuffer_ref as G
from tests.parity_runs import Runs

pytestmark = pytest.mark.gpu
F = np.float32


def _waves(n):
    return (n + 63) // 64


@pytest.mark.parametrize("name", K.GPU_FAMILIES)
def test_cast_returns_the_false_accepts(gpu, name):
    s = K.subset(name)
    n = len(s["o"])
    sc = gpu.Scene.from_prims(s["prims"])
    ctx = gpu.RenderContext(0)
    got = ctx.cast(sc, s["o"], s["d"])
    info = ctx.cast_info()
    assert CF.same(got, s["want"]) == []
    fallback = CF.fallback_waves(s)
    assert info == {"n": n, "tree": 1, "waves_tree": _waves(n) - len(fallback), "waves_list": len(fallback)}
    if name.startswith("tiny_dir") and float(name.rsplit("_k", 1)[1]) < -60:
        assert len(fallback) == _waves(n)  # below the tiny-direction limit: the list, by rule
    else:
        assert fallback == []
    got = ctx.cast(sc, s["o"], s["d"], list_walk=True)
    assert CF.same(got, s["want"]) == []
    assert ctx.cast_info() == {"n": n, "tree": 0, "waves_tree": 0, "waves_list": _waves(n)}
    ctx.close()


def test_cast_of_device_rays(gpu):
    import torch
    s = K.subset("sparse_extreme_tilted")
    n = len(s["o"])
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 4:7] = s["o"], s["d"]
    t = torch.from_numpy(rays).to("cuda:0")
    torch.cuda.synchronize()
    ctx = gpu.RenderContext(0)
    got = ctx.cast(gpu.Scene.from_prims(s["prims"]), t)
    assert CF.same(got, s["want"]) == []
    assert ctx.cast_info() == {"n": n, "tree": 1, "waves_tree": _waves(n), "waves_list": 0}
    ctx.close()
    del t


def _view(gpu, which):
    return K.extreme_view(gpu) if which == "extreme" else K.tiny_view(gpu)


@pytest.mark.parametrize("which", ["extreme", "tiny"])
def test_gbuffer_of_the_outside_view(gpu, which):
    v = _view(gpu, which)
    assert v["false"].sum() >= 8 and (v["d"][:, 0] >= 0).all()
    sc = gpu.Scene.from_prims(v["prims"])
    ctx = gpu.RenderContext(0)
    ctx.gbuffer(sc, v["cam"], K.W, K.H)
    assert ctx.gbuffer_info() == "tree"  # the camera is within the reach
    assert G.same(ctx.download_gbuffer(K.W, K.H), v["gbuffer"]) == []
    # and the view's pixel rays through the cast
    got = ctx.cast(sc, v["o"], v["d"])
    assert G.same(CF.as_gbuffer(got, K.W, K.H), v["gbuffer"]) == []
    info = ctx.cast_info()
    assert info["tree"] == 1 and info["waves_list"] == (_waves(K.W * K.H) if which == "tiny" else 0)
    ctx.close()


@pytest.mark.parametrize("which", ["extreme", "tiny"])
def test_trace_kernels_on_the_outside_view(gpu, which, monkeypatch):
    """The same view at 16 x 16, 4 spp, depth 8 and 12 through the BVH kernels (deferred and
    unwinding) and the in-order loop. In the tiny view every primary ray's direction is below
    kBvhTinyDir in every component, so the BVH kernels' list_walk ballot sends it to the in-order
    loop by rule (cull_fixtures.tiny_view and tests/test_cull_fixtures.py hold that on the rays)."""
    v = _view(gpu, which)
    for depth in (8, 12):
        assert (v["frames"][depth][4] & v["false"]).sum() >= 8  # the oracle's frame counts hits in those pixels
        assert v["frames"][depth][3]["hits"] >= 8
    r = Runs(gpu, monkeypatch, ("cull", which), v["cam"], lambda variant, depth: v["frames"][depth][:4], (K.W, K.H, K.SPP, K.SEED))
    for depth in (8, 12):
        for env in (None, ("FR_BVH", "0"), ("FR_DEFER", "0")):
            r.against_oracle("full", depth, env)
    r.done()
