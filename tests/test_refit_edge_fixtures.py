"""The edit sets of tests/refit_edge_fixtures.py, checked on the CPU with the oracle and
tests/c/refit_check.cpp so that the GPU tests of tests/test_refit_edges.py cannot pass vacuously:
the sets sit in the trees where they claim to, they are patchable (or not) as named, they change
what the rays see, a tree that is not refitted gives wrong hits where the boxes grow, the edited
primitives are hit by the rays, and the reach family's rays lie on the side of the packed reach
they were made for."""
import numpy as np
import pytest

from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import refit_edge_fixtures as E
from tests import refit_fixtures as R
from tests.test_plan import ROOT

F = np.float32
NONE = np.zeros((0, 3), F)
NO = 0xFFFFFFFF


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return R.build_check(ROOT, str(tmp_path_factory.mktemp("refit_edge_fx") / "refit_check"))


@pytest.fixture(scope="module")
def first_tables(check, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("refit_edge_first")
    out = {}

    def get(kind):
        if kind not in out:
            out[kind] = R.run_check(check, tmp, kind, CF.lattice_prims(kind), [], [], NONE, NONE, tables=True)[3]
        return out[kind]
    return get


def _changed(before, after):
    return (before["prim"] != after["prim"]) | (before["t"].view(np.uint32) != after["t"].view(np.uint32))


def _own(kind, prims, idx):
    """The set's indices without the mirror where the mirror is of another kind than the set."""
    own = {"sphere": S.SPHERE, "box": S.AABB, "obb": S.OBB, "tri": S.TRIANGLE}.get(kind)
    return [int(i) for i in idx if own is None or prims[int(i)]["kind"] == own]


@pytest.mark.parametrize("kind,name", [(k, n) for k, g, n in E.cases() if g == "shape"])
def test_shape_edits_sit_in_the_tree_and_matter(check, first_tables, tmp_path, fr, kind, name):
    prims = CF.lattice_prims(kind)
    idx, new = E.shape_edits(kind)[name]
    assert len(set(int(i) for i in idx)) == len(idx) == len(new)
    for i, p in zip(idx, new):
        was = prims[int(i)]
        assert p["kind"] == was["kind"] and p["material"] == was["material"] and np.array_equal(p["color"], was["color"])
    o, d = E.rays_for(fr, kind, new)
    edited = R.applied(prims, idx, new)
    info, topo, _, tabs = R.run_check(check, tmp_path, f"{kind}_{name}", prims, idx, new, o, d, tables=True)
    before, after = CF.hits(prims, o, d), CF.hits(edited, o, d)
    changed = _changed(before, after)
    wins = {int(i): int((after["prim"] == i).sum()) for i in idx}
    print(kind, name, "rays", len(o), "stale", info["stale"], "changed", int(changed.sum()), "wins", wins)
    assert info["tree"] == 1 and info["patchable"] == 1, info
    # where the set sits: two primitives of one leaf, two under the children of one node, one under each child of the root
    at = {int(r[0]): r for r in topo}
    a, c = R.SAME_LEAF[kind]
    assert at[a][2] == at[c][2] != NO
    a, c = R.SIBLINGS[kind]
    assert at[a][3] == at[c][3] != NO and at[a][2] != at[c][2]
    a, c = R.ROOT_SIDES[kind]
    assert {int(at[a][4]), int(at[c][4])} == {0, 1}
    # the controls
    first = first_tables(kind)
    effect = E.EFFECT[kind][name]
    assert not np.array_equal(tabs["records"], first["records"])
    if effect == "grows":
        assert info["stale"] >= 1
        assert (before["prim"] != after["prim"])[:len(CF.batch(fr, kind)["o"])].any()
    elif effect == "shrinks":
        assert not np.array_equal(tabs["nodes"], first["nodes"]) and changed.any()
    else:
        assert np.array_equal(tabs["nodes"], first["nodes"]) and np.array_equal(tabs["slot_bounds"], first["slot_bounds"])
    assert changed.any() == ((kind, name) not in E.NO_HIT_CHANGE)
    own = _own(kind, prims, idx)
    if (kind, name) in E.UNHITTABLE:
        assert all(wins[i] == 0 for i in own), wins
    else:
        assert all(n >= 1 for i, n in wins.items() if edited[i]["kind"] != S.STUB), wins
    if kind == "mixed":
        assert {prims[int(i)]["kind"] for i in idx} == {S.AABB, S.SPHERE, S.OBB, S.TRIANGLE, S.PLANE, S.STUB}
        plane = next(int(i) for i in idx if prims[int(i)]["kind"] == S.PLANE)
        g0, g1 = np.asarray(prims[plane]["g"], F), np.asarray(edited[plane]["g"], F)
        assert not np.array_equal(g0[:3], g1[:3]) and not np.array_equal(g0[3:6], g1[3:6])


def test_the_turned_frames_are_not_exact(fr):
    """The rotate set's frames have components that are no 0 / +-1: prim_bounds' sums round."""
    idx, new = E.shape_edits("obb")["rotate"]
    for p in new:
        if p["kind"] == S.OBB:
            ax = np.abs(np.asarray(p["g"][3:12], F))
            assert ((ax > 0.0) & (ax < 1.0)).sum() >= 4
            rows = np.asarray(p["g"][3:12], np.float64).reshape(3, 3)
            assert np.abs(rows @ rows.T - np.eye(3)).max() < 4 * 2.0 ** -24  # a frame, up to float32


def test_signed_zeros_are_in_the_sets(fr):
    def neg0(p, k):
        return np.signbit(F(p["g"][k])) and F(p["g"][k]) == 0

    idx, new = E.shape_edits("sphere")["neg_zero"]
    assert sum(neg0(p, 0) and neg0(p, 1) for p in new) >= 1 and all(neg0(p, 0) or neg0(p, 1) for p in new)
    idx, new = E.shape_edits("box")["neg_zero"]
    by = {int(i): p for i, p in zip(idx, new)}
    a, c = R.SAME_LEAF["box"]
    pos0 = lambda p, k: F(p["g"][k]) == 0 and not np.signbit(F(p["g"][k]))  # noqa: E731
    assert neg0(by[a], 0) and pos0(by[c], 0) and pos0(by[a], 1) and neg0(by[c], 1)  # each order of -0.0 and +0.0 in one leaf
    assert any(neg0(p, 3) for p in new)


def test_the_leaf_union_keeps_a_zero_of_each_sign(check, tmp_path, fr):
    """The box lattice's neg_zero set reaches the compare-select's order dependence: the union of
    the node above the leaf pair has lo.x = lo.y = 0 with opposite signs (fmin would give two -0.0)."""
    prims = CF.lattice_prims("box")
    idx, new = E.shape_edits("box")["neg_zero"]
    _, topo, _, tabs = R.run_check(check, tmp_path, "zeros", prims, idx, new, NONE, NONE, tables=True)
    parent = int(next(r for r in topo if int(r[0]) == R.SAME_LEAF["box"][0])[3])
    lo = tabs["node_unions"][parent, 0:2].view(F)
    assert (lo == 0).all() and np.signbit(lo[0]) != np.signbit(lo[1]), lo


@pytest.mark.parametrize("kind", E.KINDS)
def test_extent_edits(check, first_tables, tmp_path, fr, kind):
    prims = CF.lattice_prims(kind)
    ext = F(R.EXTENT[kind])
    ed = E.extent_edits(kind)
    assert E.own_reach(ed["at_extent"][1][0]) == float(ext)
    assert E.own_reach(ed["past_extent"][1][0]) == float(np.nextafter(ext, F(np.inf)))
    assert E.own_reach(ed["inward"][1][0]) < float(ext)
    last = int(ed["inward"][0][0])
    assert last == len(prims) - 1 and E.own_reach(prims[last]) == float(ext)  # the one that defines the extent
    assert max(E.own_reach(p) for p in prims[:last] if p["kind"] not in (S.PLANE, S.STUB)) < float(ext)
    if kind == "sphere":
        g = np.asarray(ed["at_extent"][1][0]["g"], F)
        assert float(g[1]) + float(g[3]) != float(ext) and F(g[1] + g[3]) == ext  # c + r is rounded to the extent
    first = first_tables(kind)
    for name, patchable in (("at_extent", 1), ("past_extent", 0), ("inward", 1)):
        idx, new = ed[name]
        o, d = E.rays_for(fr, kind, new)
        info, _, _, tabs = R.run_check(check, tmp_path, f"{kind}_{name}", prims, idx, new, o, d, tables=True)
        before, after = CF.hits(prims, o, d), CF.hits(R.applied(prims, idx, new), o, d)
        print(kind, name, "stale", info["stale"], "changed", int(_changed(before, after).sum()))
        assert info["tree"] == 1 and info["patchable"] == patchable, (name, info)
        assert _changed(before, after).any() and (after["prim"] == int(idx[0])).any()
        if name == "inward":
            assert not np.array_equal(tabs["slot_bounds"], first["slot_bounds"])
        else:
            assert info["stale"] >= 1


def test_reach_scene(check, tmp_path, fr):
    rs = E.reach_scene()
    prims, reach = rs["prims"], rs["reach"]
    assert len(prims) == 125 and R.own_extent(prims) == 3.5
    floor = 3.5 + 1.0
    assert reach == E.origin_reach(3.5, 0.5) and floor < 5.36 < reach < 5.38 < CF.REACH_UNITS * floor
    for i in E.REACH_EDITED:  # interior: no coordinate on the lattice's faces
        assert max(abs(float(c)) for c in prims[i]["g"][:3]) <= 1.5
    for name, (idx, new) in rs["edits"].items():
        o, d = rs["rays"][name]
        tree_waves, list_waves = rs["waves"][name]
        assert len(o) == 64 * (tree_waves + list_waves) <= 1500 and tree_waves >= 1 and list_waves >= 1
        n_in = 64 * tree_waves
        terms = CF.fallback_terms(o, d, reach, reach)  # the packed reach: a radius edit does not move it
        assert all((yes ^ no).all() for yes, no in terms.values())
        assert not terms["tiny_direction"][0].any() and not terms["overflow_oinv"][0].any()
        assert terms["far_origin"][1][:n_in].all() and terms["far_origin"][0][n_in:].all()
        big = np.abs(o).max(axis=1) / F(reach)
        assert {round(float(x), 4) for x in big} == set(E.REACH_SHELLS)
        scales = np.abs(d).max(axis=1)
        assert (scales < 2.0 ** -19).any() and (scales > 2.0 ** 18).any()
        edited = R.applied(prims, idx, new)
        info, _, got, _ = R.run_check(check, tmp_path, "reach_" + name, prims, idx, new, o, d)
        # the program's own fallback verdicts, at the reach it packed: the same split
        assert not got["fallback"][:n_in].any() and got["fallback"][n_in:].all()
        before, after = CF.hits(prims, o, d), CF.hits(edited, o, d)
        wins = {int(i): int((after["prim"] == i).sum()) for i in idx}
        print("reach", name, "rays", len(o), "waves", rs["waves"][name], "stale", info["stale"], "changed",
              int(_changed(before, after).sum()), "wins", wins)
        assert info["tree"] == 1 and info["patchable"] == 1
        assert _changed(before, after).any()
        if name == "grow":
            assert info["stale"] >= 1
        # every edited sphere wins rays, the ones of radius 0 too: a ray aimed at the centre from a few
        # units away has RN(b b) > RN(a cc) by rounding alone (the slack bvh_sphere_bound is built for)
        assert all(n >= 1 for n in wins.values())
        # a fresh pack of the edited list has another reach wherever the smallest radius moved
        fresh = E.origin_reach(3.5, min(abs(float(p["g"][3])) for p in edited))
        assert (fresh != reach) == (name != "grow")


@pytest.mark.parametrize("kind", E.KINDS)
def test_sequences(check, tmp_path, fr, kind):
    prims = CF.lattice_prims(kind)
    seqs = E.sequences(kind)
    assert {"two_updates", "three_updates", "duplicate", "inverse", "before_first_use", "patch_colour_patch",
            "past_then_inside_the_new_extent"} <= set(seqs)

    def patchable(base, state, name):
        wb, ws = R.prim_words(base), R.prim_words(state)
        idx = [int(i) for i in np.nonzero((wb != ws).any(axis=1))[0]]
        return R.run_check(check, tmp_path, f"{kind}_{name}", base, idx, [state[i] for i in idx], NONE, NONE)[0]["patchable"], len(idx)

    for name, sq in seqs.items():
        cur, stamped, geometric = list(prims), set(), True
        uses = iter(sq["uses"])
        base, has_copy = list(prims), False  # the list the copy was packed from
        for st in sq["steps"]:
            if st[0] == "update":
                idx = [int(i) for i in st[1]]
                geometric = all(np.array_equal(p["color"], cur[i]["color"]) for i, p in zip(idx, st[2]))
                nxt = R.applied(cur, idx, st[2])
                if geometric:
                    stamped |= set(idx)
                else:
                    base, stamped = None, set()
                cur = nxt
            elif st[0] == "rebuild":
                base, stamped = None, set()
            else:
                want = next(uses)
                if not has_copy:
                    assert want["last_sync"] == E.PACK and want["prims_patched"] == 0
                elif want["last_sync"] == E.REFIT:
                    ok, _ = patchable(base, cur, name)
                    assert ok == 1 and want["prims_patched"] == len(stamped), (name, want, stamped)
                elif base is not None and stamped:
                    assert patchable(base, cur, name)[0] == 0, name  # a pack because the patch is refused
                if want["last_sync"] != E.REFIT:
                    base = list(cur)
                stamped, has_copy = set(), True
        assert np.array_equal(R.prim_words(cur), R.prim_words(sq["final"]))
        assert sq["restored"] == (name == "inverse") == np.array_equal(R.prim_words(cur), R.prim_words(prims))
    # the coalesced updates bring primitives the first one did not hold, and re-edit some it did
    a = set(int(i) for i in seqs["two_updates"]["steps"][1][1])
    b = set(int(i) for i in seqs["two_updates"]["steps"][2][1])
    assert a & b and b - a and seqs["two_updates"]["uses"][-1]["prims_patched"] == len(a | b)
    dup = seqs["duplicate"]["steps"][1]
    assert len(dup[1]) == 3 and dup[1][0] == dup[1][2] and seqs["duplicate"]["final"][dup[1][0]] is dup[2][2]
    assert not np.array_equal(R.prim_words([dup[2][0]]), R.prim_words([dup[2][2]]))
    # the last edit of the extent sequence is outside the first pack's extent
    far = seqs["past_then_inside_the_new_extent"]["steps"]
    assert R.own_extent(far[3][2]) > R.EXTENT[kind] and R.own_extent(far[3][2]) < R.own_extent(far[1][2])
