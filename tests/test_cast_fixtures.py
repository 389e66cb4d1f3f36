"""The ray batches of the ray-query tests (tests/cast_fixtures.py) reach what they are named for,
checked on the oracle alone, without a device and without the product's kernels."""
import numpy as np
import pytest

from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import gbuffer_ref as G
from tests import ray_edge_fixtures as X

F = np.float32


@pytest.mark.parametrize("kind", X.KINDS)
def test_a_batch_holds_its_parts(fr, kind):
    b, want = CF.batch(fr, kind), CF.expected(fr, kind)
    n = len(b["o"])
    assert n % 64 != 0 and b["o"].shape == b["d"].shape == (n, 3) and len(b["label"]) == n
    lab = b["label"]
    assert (lab == "primary").sum() == 256 and (lab == "bounce").sum() > 0
    for fx in X.families(kind):
        assert (lab == "family:" + fx.name).sum() == 64, fx.name
    names = CF.specials(b["prims"])[0]
    assert [str(lab[i]) for i in b["special"][-len(names):]] == ["special:" + nm for nm in names]  # the tail
    assert b["special"][-1] >= n - 2 and len(b["special"]) == len(names) + 4
    hit = want["prim"] != CF.MISS
    assert hit.any() and (~hit).any()  # hits and misses
    assert (want["prim"][hit] < len(b["prims"])).all()
    # bounce rays start on a surface: the oracle's point of a primary hit, bit for bit
    first = CF.hits(b["prims"], b["o"][lab == "primary"], b["d"][lab == "primary"])
    pts = first["position"][first["prim"] != CF.MISS]
    assert np.array_equal(b["o"][lab == "bounce"].view(np.uint32), pts.view(np.uint32)) and len(pts) > 0
    assert len(b["prims"]) >= 49 and X.bvh_cost(b["prims"]) >= 48  # a tree scene, unless its planes forbid it


def test_the_box_batch_has_an_exact_tie(fr):
    """Two boxes that share a face are entered and left at one t: a ray whose winner's root is
    also the root of another primitive, bit for bit (the list loop keeps the first)."""
    b, want = CF.batch(fr, "box"), CF.expected(fr, "box")
    prims = b["prims"]
    ties = 0
    for i in np.nonzero(want["prim"] != CF.MISS)[0][:600]:
        best = int(want["prim"][i])
        rest = prims[best + 1:]
        if not rest:
            continue
        # the list without the winner and everything before it: a tie shows as the same root
        other = CF.hits(rest, b["o"][i:i + 1], b["d"][i:i + 1])
        if other["prim"][0] != CF.MISS and other["t"][0].view(np.uint32) == want["t"][i].view(np.uint32):
            ties += 1
    assert ties >= 1


def test_the_mixed_batch_has_stale_records(fr):
    want = CF.expected(fr, "mixed")
    assert want["stale"].any() and not want["stale"].all()
    assert CF.expected(fr, "plane")["stale"].any()


@pytest.mark.parametrize("kind", X.KINDS)
def test_every_fallback_condition_is_true_for_some_ray_and_false_for_others(fr, kind):
    b = CF.batch(fr, kind)
    terms = CF.fallback_terms(b["o"], b["d"], *CF.reach_bounds(b["prims"]))
    for name, (yes, no) in terms.items():
        assert (yes ^ no).all(), name  # decided whatever the scene's reach is within its bounds
        assert yes.any() and no.any(), name
    lab = b["label"]
    assert terms["far_origin"][0][lab == "special:far_origin"].all() and terms["far_origin"][0][lab == "special:nan_origin"].all()
    assert terms["tiny_direction"][0][lab == "special:tiny_direction"].all()
    assert terms["tiny_direction"][0][lab == "special:zero_direction"].all()
    assert terms["overflow_oinv"][0][lab == "special:overflow_oinv"].all()
    fb = CF.falls_back(b["prims"], b["o"], b["d"])
    assert fb[b["special"]].all() and not fb[lab == "primary"].any() and not fb[lab == "bounce"].any()
    waves = CF.fallback_waves(b)
    n_waves = (len(fb) + 63) // 64
    assert {0, 1, n_waves - 1} <= set(waves) and len(waves) < n_waves  # tree waves and list waves share the batch


def test_the_specials_are_what_they_say(fr):
    prims = CF.lattice_prims("mixed")
    names, o, d = CF.specials(prims)
    row = dict(zip(names, zip(o, d)))
    assert (row["zero_direction"][1] == 0).all()
    assert np.isnan(row["nan_origin"][0]).sum() == 1
    assert np.abs(row["far_origin"][0]).max() >= 1000.0 * CF.reach_bounds(prims)[1]
    assert (np.abs(row["tiny_direction"][1]) == F(2.0 ** -80)).all()
    assert row["overflow_oinv"][0][1] == F(2.0 ** 30) and row["overflow_oinv"][1][1] == 0  # 2^30 2^100 overflows


def test_the_generator_batches(fr):
    for count in (200, 2000):
        prims, o, d, want = CF.gen_batch(fr, count, 24, 16)
        assert len(prims) >= count and all(p["kind"] == S.SPHERE for p in prims if p["kind"] != S.PLANE)
        hit = want["prim"] != CF.MISS
        assert hit[:24 * 16].any() and (~hit[:24 * 16]).any() and len(o) > 24 * 16
        assert not CF.falls_back(prims, o, d).any()


def test_hits_of_pixel_rays_are_the_gbuffer_reference(fr):
    """cast_fixtures.hits on a view's pinhole rays is gbuffer_ref.gbuffer of that view."""
    for name in ("lattice_mixed", "spheres200"):
        prims, _, ocam, w, h, _ = G.case(fr, name)
        o, d = CF.camera_rays(ocam, w, h)
        assert G.same(CF.as_gbuffer(CF.hits(prims, o, d), w, h), G.expected(fr, name)) == []
