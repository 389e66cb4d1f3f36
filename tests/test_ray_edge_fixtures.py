"""The edge-ray fixtures (tests/ray_edge_fixtures.py) reach the edges they are built for.

A fixture that silently misses its target proves nothing about the kernels, so every
fixture's declared condition is checked here against the oracle alone (no GPU): the
hit-mostly fans hit, the must-miss ones miss, the two zero signs of R2 change the frame,
a zero direction gives NaN in the sky and scatters inside a box, and the images vary.
tests/test_ray_edges.py then compares the trace kernels with the same oracle frames."""
import numpy as np
import pytest

from oracle import scene_ref as S
from tests import ray_edge_fixtures as X


def _distinct(mean):
    return len({tuple(p) for p in mean.reshape(-1, 3).view(np.uint32).tolist()})


def test_edge_camera_keeps_the_sign_of_zero(fr):
    cam, ocam = X.edge_camera(fr, **X.fixture("box", "R2_neg0").cam)
    a = cam.to_array()
    assert np.signbit(a[3]) and np.signbit(a[6]) and np.signbit(a[9]) and not np.signbit(a[0])  # ll, hor, ver; pos
    assert a[3] == 0 and a[6] == 0 and a[9] == 0
    pos, _ = X.edge_camera(fr, **X.fixture("box", "R2_pos0").cam)
    assert not np.signbit(pos.to_array()[[0, 3, 6, 9]]).any()


@pytest.mark.parametrize("kind", X.KINDS)
def test_scene_sizes_select_the_intended_kernels(kind):
    """<= 15 primitives (8-B records), 16..47 (12-B records; one with a plane), >= 49 cells
    with a BVH cost of at least 48; the diffuse copies hold no metal or glass, the class
    copy at most 15 colours; every material and, in the mixed scene, every kind occurs."""
    for shift in (0, -1):
        assert len(X.lattice(kind, "small", shift)) <= 15
        assert 16 <= len(X.lattice(kind, "mid", shift)) <= 47
        mp = X.lattice(kind, "mid_plane", shift)
        assert 16 <= len(mp) <= 47 and any(p["kind"] == S.PLANE for p in mp)
        big = X.lattice(kind, "big", shift)
        assert len(X.cells(kind, "big", shift)) >= 49 and len(big) >= 49 and X.bvh_cost(big) >= 48
    for size in X.SIZES:
        full = X.lattice(kind, size)
        assert {p["material"] for p in full} == {0, 1, 2, 3}
        assert all(p["fuzz"] == 0 for p in full)
        for variant in ("diffuse", "classes"):
            assert {p["material"] for p in X.lattice(kind, size, 0, variant)} <= {S.LAMBERTIAN, S.LIGHT}
        assert len({tuple(p["color"]) for p in X.lattice(kind, size, 0, "classes")}) <= 15
    assert len({tuple(p["color"]) for p in X.lattice(kind, "big", 0, "diffuse")}) > 16
    if kind == "mixed":
        assert {p["kind"] for p in X.lattice(kind, "small")} == {S.SPHERE, S.PLANE, S.AABB, S.OBB, S.STUB, S.TRIANGLE}
    if kind in ("box", "sphere"):  # one kind only: the single-kind kernels
        assert len({p["kind"] for p in X.lattice(kind, "big")}) == 1
    # faces of the shifted lattice lie in x = 0
    if kind == "box":
        assert any(p["g"][0] == 0 or p["g"][3] == 0 for p in X.lattice(kind, "small", -1))


@pytest.mark.parametrize("kind,size,name", X.cases())
def test_fixture_reaches_its_edge(fr, kind, size, name):
    fx = X.fixture(kind, name)
    if fx.expect == "must_miss" and size == "mid_plane":
        size = "mid"  # the same cells without the backdrop plane, which every missing ray would hit
    _, mean, _, cnt = X.reference(fr, kind, size, "full", name, 8)
    nan = int(np.isnan(mean).any(axis=2).sum())
    if fx.expect == "nan_all":
        assert nan == X.W * X.H and cnt["hits"] == 0
        return
    assert nan == 0
    if fx.expect == "hit_mostly":
        assert 2 * cnt["hits"] >= cnt["segments"], cnt
    elif fx.expect == "must_miss":
        assert cnt["hits"] <= (1 if kind == "sphere" else 0), cnt
    elif fx.expect == "scatters":
        assert cnt["scatters"] > 0 and cnt["hits"] >= X.W * X.H * X.SPP, cnt  # every primary ray hits its own box
    elif fx.expect == "absorbed":
        assert cnt["hits"] == cnt["segments"] == X.W * X.H * X.SPP and cnt["scatters"] == 0 and not mean.any()
    if fx.varied:
        assert 2 * _distinct(mean) >= X.W * X.H, _distinct(mean)


@pytest.mark.parametrize("kind", ["box", "mixed"])
@pytest.mark.parametrize("size", X.SIZES)
def test_the_sign_of_a_zero_changes_the_frame(fr, kind, size):
    """R2: position.x = +0 with lower_left.x = horizontal.x = vertical.x = -0 or +0, box
    faces in x = 0. With -0 the sign of d.x follows the (zero) lens offset's sign, and a
    grazing ray hits only for +0, so the twins' frames differ."""
    neg = X.reference(fr, kind, size, "full", "R2_neg0", 8)[3]
    pos = X.reference(fr, kind, size, "full", "R2_pos0", 8)[3]
    assert neg["segments"] != pos["segments"], (neg, pos)
