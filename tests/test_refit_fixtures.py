"""The move sets of tests/refit_fixtures.py, checked on the CPU with the oracle and
tests/c/refit_check.cpp so that the GPU tests of tests/test_refit.py cannot pass vacuously:
the moves change what the rays see, the rays walk the tree, a tree that is not refitted gives
wrong hits, and the sets sit in the trees where the fixtures say they do."""
import numpy as np
import pytest

from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import refit_fixtures as R
from tests.test_plan import ROOT


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return R.build_check(ROOT, str(tmp_path_factory.mktemp("refit_fx") / "refit_check"))


@pytest.mark.parametrize("kind", R.KINDS)
def test_move_sets_matter(check, tmp_path, fr, kind):
    b = CF.batch(fr, kind)
    prims = b["prims"]
    idx, new = R.move_set(kind)
    before, after = CF.expected(fr, kind), CF.hits(R.moved_prims(kind), b["o"], b["d"])
    # (a) at least a quarter of the rays change their primitive or their t
    changed = (before["prim"] != after["prim"]) | (before["t"].view(np.uint32) != after["t"].view(np.uint32))
    print(kind, "rays changed:", int(changed.sum()), "of", len(changed))
    assert changed.sum() * 4 >= len(changed)
    # (b) no ordinary ray falls back to the list, before or after
    special = np.isin(np.arange(len(changed)), b["special"])
    still = (b["d"] == 0).all(axis=1)  # the R5 families' d = 0 rays are fallback rays by construction
    for pl in (prims, R.moved_prims(kind)):
        assert not (CF.falls_back(pl, b["o"], b["d"]) & ~special & ~still).any()
    # every move is by more than the cell pitch and stays inside the extent
    for (i, d), p in zip(R.MOVES[kind], new):
        assert np.linalg.norm(d) > 2.0
        assert p["kind"] == prims[i]["kind"] and p["material"] == prims[i]["material"]
        if p["kind"] not in (S.STUB, S.PLANE):
            assert R.own_extent([p]) <= R.EXTENT[kind]
    assert R.own_extent(prims) == R.EXTENT[kind]
    # (c) the stale-tree control, and where the set sits in the tree
    info, topo, got, _ = R.run_check(check, tmp_path, kind, prims, idx, new, b["o"], b["d"])
    print(kind, "stale-tree wrong rays:", info["stale"])
    assert info["tree"] == 1 and info["patchable"] == 1 and info["stale"] >= 1
    at = {int(r[0]): r for r in topo}
    none = 0xFFFFFFFF
    a, c = R.SAME_LEAF[kind]
    assert at[a][2] == at[c][2] != none
    a, c = R.SIBLINGS[kind]
    assert at[a][3] == at[c][3] != none and at[a][2] != at[c][2]
    a, c = R.ROOT_SIDES[kind]
    assert {int(at[a][4]), int(at[c][4])} == {0, 1}
    # each moved primitive's new bounds leave its old leaf's box: the old leaf holds only cells of
    # the lattice, and the new place was empty
    if kind == "mixed":
        kinds = {prims[i]["kind"] for i in idx}
        assert S.PLANE in kinds and S.STUB in kinds


@pytest.mark.parametrize("kind", R.KINDS)
def test_fallback_edits_are_not_patchable(check, tmp_path, fr, kind):
    prims = CF.lattice_prims(kind)
    none = np.zeros((0, 3), np.float32)
    edits = dict(R.structural_edits(kind), outside=R.outside_move(kind), nonfinite=R.nonfinite_move(kind))
    for name, (idx, new) in edits.items():
        info, _, _, _ = R.run_check(check, tmp_path, f"{kind}_{name}", prims, idx, new, none, none)
        assert info["patchable"] == 0, name
    p = R.outside_move(kind)[1][0]
    assert R.own_extent([p]) > R.EXTENT[kind]


@pytest.mark.parametrize("kind", R.KINDS)
def test_successive_sets_stay_inside(fr, kind):
    cur = R.moved_prims(kind)
    for idx, new in R.successive(kind):
        cur = R.applied(cur, idx, new)
        assert R.own_extent(cur) <= R.EXTENT[kind]
