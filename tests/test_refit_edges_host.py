"""The edge edits of tests/refit_edge_fixtures.py through the host definition of the in-place
edit, without a device: tests/c/refit_check.cpp (built with -fsanitize=address,undefined together
with the library's packer and tree builder).

For every shape edit, extent edit and radius edit of the reach scene: the builder's nodes are
reproduced by the refit, the schedule is sound, the refitted tree's walk equals the list loop on
every ray that does not fall back, putting the primitives back restores every table, and the list
loop's hits are the oracle's. The TABLES file carries the two tables the next refit reads (the
slots' bounds and the nodes' unions), which tests/test_refit_edges.py compares with the device's."""
import numpy as np
import pytest

from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import refit_edge_fixtures as E
from tests import refit_fixtures as R
from tests.test_plan import ROOT

F = np.float32
NONE = np.zeros((0, 3), F)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return R.build_check(ROOT, str(tmp_path_factory.mktemp("refit_edges") / "refit_check"))


def _clean(info):
    assert info["refit"] == info["sched"] == info["mismatch"] == info["restore"] == 0 and info["returncode"] == 0, info


@pytest.mark.parametrize("kind,group,name", E.cases())
def test_edits_refit_to_the_oracle(check, tmp_path, fr, kind, group, name):
    prims = CF.lattice_prims(kind)
    idx, new = E.edit_of(kind, group, name)
    o, d = E.rays_for(fr, kind, new)
    info, _, got, _ = R.run_check(check, tmp_path, f"{kind}_{name}", prims, idx, new, o, d)
    print(kind, name, "rays", len(o), "stale-tree wrong rays:", info["stale"])
    _clean(info)
    assert info["tree"] == 1
    assert CF.same(got, CF.hits(R.applied(prims, idx, new), o, d)) == []


@pytest.mark.parametrize("name", list(E.REACH_RADII))
def test_radius_edits_keep_the_packed_reach(check, tmp_path, fr, name):
    """The walk at the packed reach over bounds formed at the packed reach, for radii below and
    above the packed minimum: tree = list = oracle on the grazing rays of every shell."""
    rs = E.reach_scene()
    idx, new = rs["edits"][name]
    o, d = rs["rays"][name]
    info, _, got, _ = R.run_check(check, tmp_path, "reach_" + name, rs["prims"], idx, new, o, d)
    print("reach", name, "stale-tree wrong rays:", info["stale"])
    _clean(info)
    assert info["tree"] == 1 and info["patchable"] == 1
    assert CF.same(got, CF.hits(R.applied(rs["prims"], idx, new), o, d)) == []


def test_a_turned_box_with_a_negative_half_is_bounded_by_its_magnitude(check, tmp_path, fr):
    """The builder's own bounds, in a fresh pack: the slab test hits a negative half size like its
    magnitude, so the bounds must span it (they summed the signed half, which cancelled the other
    axes' spans in a turned frame: 265 rays of this set missed the box in the tree walk)."""
    kind = "obb"
    idx, new = E.shape_edits(kind)["turned_neg_half"]
    edited = R.applied(CF.lattice_prims(kind), idx, new)
    o, d = E.rays_for(fr, kind, new)
    info, _, got, tabs = R.run_check(check, tmp_path, "fresh", edited, [], [], o, d, tables=True)
    _clean(info)
    assert CF.same(got, CF.hits(edited, o, d)) == []
    pos = [E.with_g(p, {12 + k: abs(float(p["g"][12 + k])) for k in range(3)}) if p["kind"] == S.OBB else p for p in edited]
    _, _, _, want = R.run_check(check, tmp_path, "fresh_pos", pos, [], [], NONE, NONE, tables=True)
    for n in ("nodes", "slot_bounds", "node_unions", "leaf_order"):
        assert np.array_equal(tabs[n], want[n]), n


@pytest.mark.parametrize("kind", E.KINDS)
def test_the_tables_file_carries_the_refit_tables(check, tmp_path, fr, kind):
    """Format 1: the slots' bounds and the nodes' unions follow the nodes. Each slot's row is the
    primitive's bounds, each node's union holds its children's boxes without their padding."""
    prims = CF.lattice_prims(kind)
    idx, new = R.move_set(kind)
    info, _, _, tabs = R.run_check(check, tmp_path, kind, prims, idx, new, NONE, NONE, tables=True)
    _clean(info)
    words = np.fromfile(str(tmp_path / f"{kind}.tables"), np.uint32)
    assert words[3] == 1 and len(words) == 4 + 16 * int(words[0]) + (16 + 1 + 8) * int(words[1]) + (16 + 8) * int(words[2])
    sb, un, nodes, order = tabs["slot_bounds"], tabs["node_unions"], tabs["nodes"], tabs["leaf_order"]
    assert sb.shape == (info["slots"], 8) and un.shape == (info["nodes"], 8) and nodes.shape == (info["nodes"], 16)
    moved = R.moved_prims(kind)
    for slot, row in enumerate(sb.view(F)):
        p = moved[int(order[slot, 0])]
        if p["kind"] in (S.AABB, S.TRIANGLE):  # (a sphere's bounds grow with the reach, an oriented box's are sums)
            pts = np.asarray(p["g"][:6 if p["kind"] == S.AABB else 9], F).reshape(-1, 3)
            assert np.array_equal(row[0:3], pts.min(axis=0)) and np.array_equal(row[4:7], pts.max(axis=0))
    pad = F(F(F(1e-4) * F(R.EXTENT[kind])) + F(1e-4))
    nf, uf = nodes.view(F), un.view(F)
    for q in range(len(nodes)):
        # the builder's layout (refit.h refit_node): left lo, left hi and the right child's box in a[3], b[3], c
        lo = np.minimum(nf[q, 0:3] + pad, np.array([nf[q, 3], nf[q, 8], nf[q, 9]], F) + pad)
        hi = np.maximum(nf[q, 4:7] - pad, np.array([nf[q, 7], nf[q, 10], nf[q, 11]], F) - pad)
        assert np.allclose(uf[q, 0:3], lo, rtol=0, atol=4e-6 * R.EXTENT[kind]), q
        assert np.allclose(uf[q, 4:7], hi, rtol=0, atol=4e-6 * R.EXTENT[kind]), q
