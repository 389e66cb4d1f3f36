"""The cull fixtures (tests/cull_fixtures.py) meet their conditions in the oracle alone: nothing
here depends on how the tree is built.

- Each sphere family (sparse_extreme, sparse_random, tiny_dir) holds at least 100 rays whose oracle
  winner is a sphere the ray passes outside in float64 (p > r), and so does each member that is
  built to: both sparse_extreme ray sets, sparse_random, and every tiny_dir scene from k = -69.2
  down. tiny_dir at k >= -67 holds none: controls.
- In sparse_extreme and tiny_dir such a winner is sphere 0, the scene's extreme on +x, and every
  ray has o.x beyond that sphere's face padded by 1e-4 (extent + 1) and d.x >= 0: it touches no
  box padded that way, so a tree with such boxes cannot return the hit.
- Every false accept of a ray the walk admits (cast_fixtures.falls_back is false) lies under the
  bound of bvh.h, p^2 <= r^2 + 20 * 2^-24 |o - c|^2 + 2^-28, in float64; the tiny_dir rays below the
  tiny-direction limit, which exceed it, all fall back.
- The GPU subsets put the false accepts first and are no multiple of 64 long; the views hold
  their false-accept pixels."""
import numpy as np
import pytest

from tests import cast_fixtures as CF
from tests import cull_fixtures as K


def _k(name):
    return float(name.rsplit("_k", 1)[1])


@pytest.mark.parametrize("name", K.SPHERE_FAMILIES)
def test_false_accepts_of_a_member(name):
    fa = K.false_accepts(name)
    h = K.hits(name)
    n = int(fa.sum())
    if name.startswith("tiny_dir"):
        if _k(name) >= -67:
            assert n == 0
        elif _k(name) <= -69.2:
            assert n >= 100
    else:
        assert n >= 100
    if name != "sparse_random":
        assert (h["prim"][fa] == 0).all()
        assert K.outside_old_boxes(name).all()
    assert (h["prim"] != CF.MISS).sum() >= n and len(fa) >= 4096


@pytest.mark.parametrize("family", ["sparse_extreme", "sparse_random", "tiny_dir_r1.0", "tiny_dir_r0.125"])
def test_false_accepts_of_a_family(family):
    members = [m for m in K.SPHERE_FAMILIES if m.startswith(family) and not (m.startswith("tiny") and _k(m) >= -67)]
    assert sum(int(K.false_accepts(m).sum()) for m in members) >= 100


@pytest.mark.parametrize("name", K.SPHERE_FAMILIES)
def test_admitted_false_accepts_lie_under_the_bound(name):
    f, h, fa = K.family(name), K.hits(name), K.false_accepts(name)
    fb = CF.falls_back(f["prims"], f["o"], f["d"])
    if name.startswith("tiny_dir"):
        assert fb.all() == (_k(name) < -60) and fb.any() == (_k(name) < -60)
    else:
        assert not fb.any()
    p, r, dist = K.passing_distance(f["prims"], f["o"], f["d"], h["prim"])
    sel = fa & ~fb
    excess = p[sel] ** 2 - r[sel] ** 2
    assert (excess <= K.DISC_ERR * dist[sel] ** 2 + K.DISC_ABS).all()
    # and the ball the builder uses, taken at the largest |o - c| of the reach, holds them all
    reach = CF.reach_bounds(f["prims"])[0]
    c = np.array([q["g"][:3] for q in f["prims"]], np.float64)[h["prim"][sel]]
    lmax2 = ((reach + np.abs(c)) ** 2).sum(axis=1)
    assert (dist[sel] ** 2 <= lmax2).all() and (p[sel] ** 2 <= r[sel] ** 2 + K.DISC_ERR * lmax2 + K.DISC_ABS).all()


@pytest.mark.parametrize("name", K.GPU_FAMILIES)
def test_gpu_subsets(name):
    s = K.subset(name)
    n, nf = len(s["o"]), int(s["false"].sum())
    assert 64 < n <= 4096 and n % 64 != 0
    assert s["false"][:nf].all() and not s["false"][nf:].any() and n - nf >= min(nf, 64)
    assert nf == min(int(K.false_accepts(name, K.POOL.get(name)).sum()), 2048) and nf >= (100 if name.startswith("sparse") else 0)
    assert CF.same(CF.hits(s["prims"], s["o"], s["d"]), s["want"]) == []


def test_other_kinds_hit_their_targets():
    for name in K.OTHER_FAMILIES:
        f = K.family(name)
        assert len(f["prims"]) == 2000 and len(f["o"]) == 20000 and np.isfinite(f["d"]).all()
    # (their hits are counted by tests/test_cull_host.py, which walks them)


@pytest.mark.parametrize("which", ["extreme", "tiny"])
def test_views(fr, which):
    v = K.extreme_view(fr) if which == "extreme" else K.tiny_view(fr)
    assert v["false"].sum() >= 8 and (v["gbuffer"]["prim"][v["false"]] == 0).all() and (v["d"][:, 0] == 0).all()
    for depth in (8, 12):
        assert (v["frames"][depth][4] & v["false"]).sum() >= 8
    # the camera is on the outside plane of sphere 0, beyond the old padding, and within the reach
    g0 = v["prims"][0]["g"]
    assert float(v["o"][0, 0]) > float(g0[0]) + float(g0[3]) + K.pad_of(v["prims"])
    assert np.abs(v["o"][0]).max() <= CF.reach_bounds(v["prims"])[0]
    tiny = CF.fallback_terms(v["o"], v["d"], *CF.reach_bounds(v["prims"]))["tiny_direction"]
    if which == "tiny":  # every pixel ray is below the tiny-direction limit, and above the former one
        assert tiny[0].all() and (np.abs(v["d"]).max(axis=1) >= 2.0 ** -70).all()
        assert all(float(x) == 0.0 for x in v["ocam"].position)
    else:
        assert tiny[1].all()
