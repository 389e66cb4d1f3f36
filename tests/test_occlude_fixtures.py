"""The per-ray ranges of the occlusion tests (tests/occlude_fixtures.py) reach the classes they
are chosen for, checked on the oracle-based reference alone, without a device and without the
product's kernels."""
import numpy as np
import pytest

from tests import cast_fixtures as CF
from tests import occlude_fixtures as OF
from tests import ray_edge_fixtures as X

F = np.float32


def _mode(n, name):
    return np.arange(n) % len(OF.MODES) == OF.MODES.index(name)


@pytest.mark.parametrize("kind", X.KINDS)
def test_a_batch_holds_both_answers_at_the_boundary(fr, kind):
    b, t_max, ref = OF.lattice(fr, kind)
    want = CF.expected(fr, kind)
    n = len(t_max)
    hit = want["prim"] != CF.MISS
    occ = ref["occluded"]
    assert occ.any() and (~occ).any()
    # every mode is present, with the values it names
    assert all(_mode(n, m).sum() >= n // 12 for m in OF.MODES)
    assert np.isnan(t_max[_mode(n, "nan")]).all() and np.isinf(t_max[_mode(n, "inf")]).all()
    assert np.array_equal(t_max[_mode(n, "t") & hit].view(np.uint32), want["t"][_mode(n, "t") & hit].view(np.uint32))
    up, down = _mode(n, "t_up") & hit, _mode(n, "t_down") & hit
    assert (t_max[up] > want["t"][up]).all() and (np.nextafter(t_max[up], F(-np.inf)) == want["t"][up]).all() and up.any()
    assert (t_max[down] < want["t"][down]).all() and (np.nextafter(t_max[down], F(np.inf)) == want["t"][down]).all() and down.any()
    # the boundary pair: one ulp above the root a ray is occluded, at or below it rays are not
    pair = _mode(n, "t") | _mode(n, "t_up") | _mode(n, "t_down")
    assert (occ & pair).any() and (~occ & pair & hit).any()
    assert occ[up].any() and (~occ[_mode(n, "t") & hit]).any() and (~occ[down]).any()
    if kind != "plane" and kind != "mixed":  # (a plane is gated on its denominator, not on its root)
        assert occ[up].all() and not occ[_mode(n, "t") & hit].any() and not occ[down].any()
    # a range that ends at or below t_min, and a NaN, occlude nothing; a miss stays a miss
    for m in ("t_min", "zero", "minus_one", "nan"):
        assert not occ[_mode(n, m)].any(), m
    assert np.array_equal(occ[_mode(n, "flt_max")], hit[_mode(n, "flt_max")])
    assert np.array_equal(occ, ref["prim"] != CF.MISS)


@pytest.mark.parametrize("kind", ["plane", "mixed"])
def test_the_plane_gate_decides_some_rays(fr, kind):
    """A ray whose ranged winner is not its unbounded winner cut at t_max: a plane that wins at
    FLT_MAX fails a short ray's gate on the denominator, or passes it with a root beyond t_max."""
    _, t_max, ref = OF.lattice(fr, kind)
    cut = OF.truncated(CF.expected(fr, kind), t_max)
    assert (cut != ref["prim"]).any()


@pytest.mark.parametrize("kind", X.KINDS)
def test_a_batch_has_tree_waves_and_fallback_waves(fr, kind):
    b, t_max, _ = OF.lattice(fr, kind)
    waves = CF.fallback_waves(b)
    assert 0 < len(waves) < (len(t_max) + 63) // 64


def test_the_sphere_batch(fr):
    prims, o, d, t_max, ref = OF.spheres(fr, 2000)
    assert len(o) > 24 * 16 and len(o) >= 100 + 321 and ref["occluded"].any() and not ref["occluded"].all()
    assert not CF.falls_back(prims, o, d).any()
    sel = slice(100, 100 + 321)  # the tails the GPU test cuts: both answers in each
    assert ref["occluded"][sel].any() and not ref["occluded"][sel].all()
