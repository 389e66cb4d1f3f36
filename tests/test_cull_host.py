"""The tree's cull against the list loop on the cull fixtures, without a device.

tests/c/cast_check.cpp (built as tests/test_cast_host.py builds it, with its sanitizer flags) walks
cast.h's definition of the tree walk and of the list loop over the tables the library packs:
- every family of tests/cull_fixtures.py: no ray that passes the fallback test differs between the
  two (rays whose sphere test accepts a root by rounding error, from outside every box padded by
  1e-4 (extent + 1) alone, are the ones a cull without the sphere bound of bvh.h loses), and
  every sphere winner of such a ray lies within bvh_sphere_bound in double;
- the fallback count is the Python restatement's (cast_fixtures.fallback_terms);
- on the GPU subsets and the views' pixel rays, the list loop's rows are cast_fixtures.hits' bits;
- the box, triangle and oriented-box searches keep their zero."""
import numpy as np
import pytest

from tests import cast_fixtures as CF
from tests import cull_fixtures as K
from tests import ray_edge_fixtures as X
from tests.test_cast_host import check, run_check  # noqa: F401 (check: the fixture that builds the program)

F = np.float32


def _cam(fr):
    return X.edge_camera(fr, w=4, h=4, **X.fixture("box", "R0_control").cam)[1]


def _walk(check, tmp_path, fr, name, prims, o, d, ocam=None, w=4, h=4):
    info, got, fb = run_check(check, tmp_path, name, prims, ocam or _cam(fr), w, h, o, d)
    assert info["tree"] == 1 and info["mismatch"] == 0 and info["bound"] == 0 and info["pixel_ray"] == 0 and info["rr"] == 0
    reach = float(np.array([info["reach"]], np.uint32).view(F)[0])
    lo, hi = CF.reach_bounds(prims)
    assert lo * (1.0 - 2.0 ** -22) <= reach <= hi * (1.0 + 2.0 ** -22)  # (the library's reach is rounded to f32)
    terms = CF.fallback_terms(o, d, reach, reach)
    want = terms["far_origin"][0] | terms["tiny_direction"][0] | terms["overflow_oinv"][0]
    assert np.array_equal(fb, want) and info["fallback"] == int(want.sum())
    return info, got, fb


@pytest.mark.parametrize("name", K.SPHERE_FAMILIES)
def test_tree_equals_list_on_the_sphere_families(check, tmp_path, fr, name):
    f = K.family(name)
    info, got, fb = _walk(check, tmp_path, fr, name, f["prims"], f["o"], f["d"])
    assert np.array_equal(fb, CF.falls_back(f["prims"], f["o"], f["d"]))
    if name.startswith("tiny_dir") and float(name.rsplit("_k", 1)[1]) < -60:
        assert fb.all()  # below the tiny-direction limit: the list, by rule
    else:
        assert not fb.any() and info["steps"] > len(f["o"])
    assert CF.same(got, K.hits(name)) == []


@pytest.mark.parametrize("name", K.GPU_FAMILIES)
def test_list_rows_equal_the_oracle_on_the_gpu_subsets(check, tmp_path, fr, name):
    s = K.subset(name)
    _, got, _ = _walk(check, tmp_path, fr, name, s["prims"], s["o"], s["d"])
    assert CF.same(got, s["want"]) == []


@pytest.mark.parametrize("which", ["extreme", "tiny"])
def test_tree_equals_list_on_the_views(check, tmp_path, fr, which):
    v = K.extreme_view(fr) if which == "extreme" else K.tiny_view(fr)
    _, got, fb = _walk(check, tmp_path, fr, which, v["prims"], v["o"], v["d"], v["ocam"], K.W, K.H)
    assert fb.all() == (which == "tiny")
    gb = CF.as_gbuffer(got, K.W, K.H)
    for a, b in (("prim", "prim"), ("depth", "depth"), ("normal", "normal"), ("position", "position"), ("albedo", "albedo")):
        assert np.array_equal(np.ascontiguousarray(gb[a]).view(np.uint32), np.ascontiguousarray(v["gbuffer"][b]).view(np.uint32)), a


@pytest.mark.parametrize("name", K.OTHER_FAMILIES)
def test_other_kinds_keep_their_zero(check, tmp_path, fr, name):
    f = K.family(name)
    info, got, fb = _walk(check, tmp_path, fr, name, f["prims"], f["o"], f["d"])
    assert not fb.any() and info["steps"] > len(f["o"])
    assert (got["prim"] != CF.MISS).sum() >= len(f["o"]) // 100  # aimed rays do hit (from the shell f32 directions resolve 0.03 units: few)
