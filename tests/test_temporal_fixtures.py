"""The views of tests/temporal_fixtures.py reach what they are chosen for, on the oracle and the
restatement alone (tests/temporal_ref.py): every reason code of the reprojection, a small orbit
that keeps at least half of the hit pixels, and the identity map of a view onto itself.

"no history yet" is not a reason a pair can reach: it is what every pixel reads when the context
holds no history at all, so it is checked on the first view of every case and
is off the pairs' list."""
import numpy as np
import pytest

from tests import temporal_fixtures as X
from tests import temporal_ref as T

F = np.float32
PAIR = (("frame", 0), ("frame", 0), ("call",), ("frame", 1), ("call",))


@pytest.mark.parametrize("name", list(X.CASES))
def test_first_view_has_no_history(name):
    r = X.run(name, PAIR[:3], 0)[0]
    assert (r["reason"] == T.NO_HISTORY).all() and (r["source"] == T.NONE).all()
    assert not r["prior_a"].any() and not r["prior_q"].any() and not r["prior_n"].any() and not r["prior_k"].any()


def test_the_codes_pair_reaches_every_reason():
    r = X.run("codes", PAIR, 0)[1]
    counts = np.bincount(r["reason"].ravel(), minlength=8)
    print(dict(zip(T.REASONS, counts.tolist())))
    assert counts[T.NO_HISTORY] == 0 and all(counts[c] >= 1 for c in range(8) if c != T.NO_HISTORY)
    g = X.features("codes", 1)
    assert np.array_equal(r["reason"] == T.MISS, g["prim"] == T.NONE)
    assert np.array_equal(r["source"] == T.NONE, np.isin(r["reason"], (T.MISS, T.OFFSCREEN)))
    # the "history" pixels' sources really carry non-finite totals
    first = X.run("codes", PAIR[:3], 0)[0]
    src = r["source"][r["reason"] == T.HISTORY]
    assert not np.isfinite(first["total_a"].reshape(-1, 3)[src]).all(-1).any()


@pytest.mark.parametrize("name", ["spheres", "spheres_33x17", "boxes", "metal", "scene_01", "spheres_down", "metal_near"])
def test_small_moves_keep_at_least_half_of_the_hit_pixels(name):
    r = X.run(name, PAIR, 0)[1]
    counts = np.bincount(r["reason"].ravel(), minlength=8)
    assert counts[T.NO_HISTORY] == 0 and counts[T.REUSED]
    hits = int((r["reason"] != T.MISS).sum())
    assert 2 * counts[T.REUSED] >= hits, (counts, hits)  # the small move keeps at least half of the hit pixels


def test_tight_options_reach_plane_distance_on_spheres():
    r = X.run("spheres_tight", PAIR, 0)[1]
    assert (r["reason"] == T.PLANE).any() and (r["reason"] == T.REUSED).any()


@pytest.mark.parametrize("name", ["spheres", "boxes", "metal_near"])
def test_identity(name):
    """The same camera after accum_reset: every hit pixel with finite history maps to itself, and
    n' = min(n_T, cap) up to the scaling's one rounding."""
    script = (("frame", 0),) * 3 + (("call",), ("restart",), ("frame", 0), ("call",))
    opt = dict(T.OPT, n_max=8.0, n_max_specular=8.0)
    first, r = X.run(name, script, 0, opt=opt)
    assert first["action"] == "empty" and r["action"] == "reproject"
    g = X.features(name, 0)
    h, w = g["prim"].shape
    hit = g["prim"] != T.NONE
    finite = np.isfinite(first["total_a"]).all(-1) & np.isfinite(first["total_q"]).all(-1)
    assert np.array_equal(r["reason"] == T.REUSED, hit & finite) and (hit & finite).any()
    own = np.arange(w * h, dtype=np.uint32).reshape(h, w)
    assert np.array_equal(r["source"][hit], own[hit])
    assert (first["total_n"] == 12).all()
    ok = r["reason"] == T.REUSED
    f = F(F(8) / F(12))
    assert np.array_equal(r["prior_n"][ok], np.full(int(ok.sum()), F(12) * f, F))
    assert np.allclose(r["prior_n"][ok], 8.0, rtol=2.0 ** -23, atol=0)
    assert np.allclose(r["prior_k"][ok], 1 + 2 * 8 / 12, rtol=2.0 ** -22, atol=0)
    assert (r["total_n"][ok] == r["prior_n"][ok] + 4).all()
