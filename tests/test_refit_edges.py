"""Edge cases of the in-place scene edit (fr_scene_update) on the GPU, bit for bit: edits of a
primitive's shape, edits at the packed extent, radius edits under a packed reach above its floor,
coalesced and interleaved updates, trace kernels and per-context reuse state after a refit.

Every test that means the device path asserts FR_SCENE_SYNC_REFIT through tests/test_refit.py's
_refit, every fallback FR_SCENE_SYNC_PACK. The edit sets, rays and sequences are those of
tests/refit_edge_fixtures.py, which tests/test_refit_edge_fixtures.py and
tests/test_refit_edges_host.py hold against the oracle and tests/c/refit_check.cpp on the CPU. The
device tables are compared with that program's, the two tables the next refit reads (the slots'
bounds and the nodes' unions) included, as uint32: a zero of the other sign is a difference."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import adaptive_ref as AR
from tests import cast_fixtures as CF
from tests import gbuffer_ref as G
from tests import nonfinite_fixtures as N
from tests import occlude_fixtures as OF
from tests import ray_edge_fixtures as X
from tests import refit_edge_fixtures as E
from tests import refit_fixtures as R
from tests import temporal_ref as T
from tests.test_accumulate import _frame_sum
from tests.test_adaptive import _refused
from tests.test_plan import ROOT
from tests.test_refit import DEPTH, H, SEED, SPP, W, _frame_case, _packed, _refit, _same_frame

pytestmark = pytest.mark.gpu
F = np.float32
NONE = np.zeros((0, 3), F)
TABLES = ("records", "leaf_records", "leaf_order", "nodes", "slot_bounds", "node_unions")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return R.build_check(ROOT, str(tmp_path_factory.mktemp("refit_edges_gpu") / "refit_check"))


def _tables(sc):
    return {n: sc.download_table(0, n) for n in TABLES}


def _same_tables(got, want, tag):
    for n in TABLES:
        assert got[n].shape == want[n].shape and np.array_equal(got[n], want[n]), (tag, n)


def _host_tables(check, tmp_path, name, base, state):
    """refit_check's tables of list `state` as an edit of the pack of `base`."""
    wb, ws = R.prim_words(base), R.prim_words(state)
    idx = [int(i) for i in np.nonzero((wb != ws).any(axis=1))[0]]
    return R.run_check(check, tmp_path, name, base, idx, [state[i] for i in idx], NONE, NONE, tables=True)[3]


@pytest.mark.parametrize("kind,name", [(k, n) for k, g, n in E.cases() if g == "shape"])
def test_queries_and_tables_after_a_shape_edit(gpu, check, tmp_path, kind, name):
    prims = CF.lattice_prims(kind)
    idx, new = E.shape_edits(kind)[name]
    back = [prims[int(i)] for i in idx]
    edited = R.applied(prims, idx, new)
    o, d = E.rays_for(gpu, kind, new)
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    ctx.cast(sc, o[:64], d[:64])
    first = _tables(sc)
    n_nodes = ctx.scene_info(sc)["n_nodes"]
    # cast
    sc.update(idx, new)
    got = ctx.cast(sc, o, d)
    info = ctx.scene_info(sc)
    _refit(info, len(idx), n_nodes)
    assert (info["packs"], info["refits"]) == (1, 1)
    assert CF.same(got, CF.hits(edited, o, d)) == []
    assert ctx.cast_info()["tree"] == 1
    # the six tables
    _same_tables(_tables(sc), R.run_check(check, tmp_path, f"{kind}_{name}", prims, idx, new, NONE, NONE, tables=True)[3], name)
    # occlusion: the first use after putting everything back and editing again
    w = h = 16
    cam, ocam = X.edge_camera(gpu, w=w, h=h, **X.fixture(kind, "R0_control").cam)
    co, cd = CF.camera_rays(ocam, w, h)
    t_max = OF.t_max_of(CF.hits(edited, co, cd)["t"])
    want = OF.ranged(edited, co, cd, t_max)["occluded"]
    sc.update(idx, back)
    sc.update(idx, new)
    occ = ctx.occluded(sc, co, cd, t_max=t_max)
    _refit(ctx.scene_info(sc), len(idx), n_nodes)
    assert np.array_equal(occ, want) and want.any() and not want.all()
    assert ctx.occluded_info()["tree"] == 1
    # the G-buffer, likewise
    sc.update(idx, back)
    sc.update(idx, new)
    ctx.gbuffer(sc, cam, w, h)
    _refit(ctx.scene_info(sc), len(idx), n_nodes)
    assert ctx.gbuffer_info() == "tree"
    assert G.same(ctx.download_gbuffer(w, h), G.gbuffer(edited, ocam, w, h)) == []
    # everything back: the first pack's tables
    sc.update(idx, back)
    ctx.cast(sc, o[:64], d[:64])
    _refit(ctx.scene_info(sc), len(idx), n_nodes)
    _same_tables(_tables(sc), first, name + " restored")
    ctx.close()
    sc.close()


@pytest.mark.parametrize("kind", E.KINDS)
def test_the_extent_is_a_closed_bound(gpu, check, tmp_path, kind):
    prims = CF.lattice_prims(kind)
    ed = E.extent_edits(kind)
    ctx = gpu.RenderContext(0)
    for name, refits in (("at_extent", True), ("past_extent", False), ("inward", True)):
        idx, new = ed[name]
        edited = R.applied(prims, idx, new)
        o, d = E.rays_for(gpu, kind, new)
        sc = gpu.Scene.from_prims(prims)
        ctx.cast(sc, o[:64], d[:64])
        first = _tables(sc)
        sc.update(idx, new)
        got = ctx.cast(sc, o, d)
        info = ctx.scene_info(sc)
        if refits:
            _refit(info, 1)
            assert (info["packs"], info["refits"]) == (1, 1), name
            _same_tables(_tables(sc), _host_tables(check, tmp_path, f"{kind}_{name}", prims, edited), name)
        else:
            _packed(info)
            assert (info["packs"], info["refits"]) == (2, 0), name
            _same_tables(_tables(sc), _host_tables(check, tmp_path, f"{kind}_{name}", edited, edited), name)
        assert CF.same(got, CF.hits(edited, o, d)) == [], name
        sc.update(idx, [prims[int(i)] for i in idx])
        ctx.cast(sc, o[:64], d[:64])
        if refits:
            _refit(ctx.scene_info(sc), 1)
            _same_tables(_tables(sc), first, name + " restored")
        else:  # inside the larger extent of the second pack
            _refit(ctx.scene_info(sc), 1)
            _same_tables(_tables(sc), _host_tables(check, tmp_path, f"{kind}_{name}_back", edited, prims), name + " back")
        sc.close()
    ctx.close()


@pytest.mark.parametrize("name", list(E.REACH_RADII))
def test_radius_edits_under_a_packed_reach_above_its_floor(gpu, check, tmp_path, name):
    rs = E.reach_scene()
    prims = rs["prims"]
    idx, new = rs["edits"][name]
    o, d = rs["rays"][name]
    tree_waves, list_waves = rs["waves"][name]
    waves = {"n": len(o), "tree": 1, "waves_tree": tree_waves, "waves_list": list_waves}
    edited = R.applied(prims, idx, new)
    sc = gpu.Scene.from_prims(prims)
    ctx, other = gpu.RenderContext(0), gpu.RenderContext(0)
    assert CF.same(ctx.cast(sc, o, d), CF.hits(prims, o, d)) == []
    assert ctx.cast_info() == waves
    first = _tables(sc)
    sc.update(idx, new)
    got = ctx.cast(sc, o, d)
    _refit(ctx.scene_info(sc), len(idx), ctx.scene_info(sc)["n_nodes"])
    assert ctx.cast_info() == waves  # the packed reach stands: the designed waves fall back, no more
    assert CF.same(got, CF.hits(edited, o, d)) == []
    _same_tables(_tables(sc), _host_tables(check, tmp_path, "reach_" + name, prims, edited), name)
    fresh = gpu.Scene.from_prims(edited)  # another reach wherever the smallest radius moved; the same hits
    assert CF.same(got, other.cast(fresh, o, d)) == []
    assert other.cast_info()["tree"] == 1
    fresh.close()
    sc.update(idx, [prims[int(i)] for i in idx])
    ctx.cast(sc, o[:64], d[:64])
    _refit(ctx.scene_info(sc), len(idx))
    _same_tables(_tables(sc), first, name + " restored")
    ctx.close()
    other.close()
    sc.close()


@pytest.mark.parametrize("kind", ["box", "sphere"])
@pytest.mark.parametrize("name", ["two_updates", "three_updates", "duplicate", "inverse", "before_first_use",
                                  "patch_colour_patch", "patch_rebuild_patch", "past_then_inside_the_new_extent"])
def test_sequences_of_updates(gpu, check, tmp_path, kind, name):
    sq = E.sequences(kind)[name]
    b = CF.batch(gpu, kind)
    prims, o, d = CF.lattice_prims(kind), b["o"], b["d"]
    sc = gpu.Scene.from_prims(prims)
    ctx, late = gpu.RenderContext(0), gpu.RenderContext(0)
    cur, base, first, got = list(prims), None, None, None
    uses = iter(sq["uses"])
    for st in sq["steps"]:
        if st[0] == "update":
            sc.update(np.asarray(st[1], np.uint32), st[2])
            cur = R.applied(cur, st[1], st[2])
        elif st[0] == "rebuild":
            sc.rebuild()
        else:
            want = next(uses)
            got = ctx.cast(sc, o, d)
            info = ctx.scene_info(sc)
            assert {k: info[k] for k in want} == want, (name, info)
            if want["last_sync"] == E.REFIT:
                _refit(info, want["prims_patched"], info["n_nodes"])
            else:
                _packed(info)
                base = list(cur)
            assert CF.same(got, CF.hits(cur, o, d)) == [], name
            first = _tables(sc) if first is None else first
    assert np.array_equal(R.prim_words(cur), R.prim_words(sq["final"]))
    have = np.array([np.frombuffer(bytes(p), np.uint32) for p in sc.prims()])
    assert np.array_equal(have, R.prim_words(cur))
    # the tables: the host's edit of the last pack's list, the coalesced updates as one
    _same_tables(_tables(sc), _host_tables(check, tmp_path, f"{kind}_{name}", base, cur), name)
    if sq["restored"]:
        _same_tables(_tables(sc), first, name + " restored")
    # a second context on the device, which uses the scene only now
    got_late = late.cast(sc, o, d)
    info, il = ctx.scene_info(sc), late.scene_info(sc)
    assert il["last_sync"] == 0 and il["prims_patched"] == 0
    assert all(il[k] == info[k] for k in ("packs", "refits", "edit_seq", "version")), (info, il)
    assert CF.same(got_late, got) == []
    ctx.close()
    late.close()
    sc.close()


def _frame_edit(kind, variant):
    """(edit name, (indices, prims)) of a rendered-frame case, on the variant's own materials."""
    prims = X.lattice(kind, "big", 0, variant)
    sets = E.shape_edits(kind)
    if kind == "sphere":  # the first two shrink, the others grow
        idx, small = sets["shrink"]
        edit = (idx, small[:2] + sets["grow"][1][2:])
    else:
        edit = sets[{"obb": "rotate", "tri": "tilt", "mixed": "all_kinds"}[kind]]
    return E.on_variant(prims, *edit)


@pytest.mark.parametrize("kind,variant", [("obb", "full"), ("tri", "full"), ("mixed", "full"), ("sphere", "classes")])
def test_rendered_frames_after_a_shape_edit(gpu, monkeypatch, kind, variant):
    """The trace kernels over a refitted tree: oriented boxes, triangles (their packed normals), the
    mixed lattice's segments with planes and stubs, the class-record kernel; and the same copy
    through the in-order loop."""
    prims, _, _, cam, ocam = _frame_case(gpu, kind, "big", variant)
    idx, new = _frame_edit(kind, variant)
    edited = R.applied(prims, idx, new)
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    p = gpu.make_params(W, H, SPP, DEPTH, seed=SEED)
    ctx.render(sc, cam, p)
    st = ctx.sync()
    before = O.render(prims, ocam, W, H, SPP, DEPTH, seed=SEED)
    _same_frame(ctx.download(W, H) + (st,), before)
    sc.update(idx, new)
    ctx.render(sc, cam, p)
    st = ctx.sync()
    info = ctx.scene_info(sc)
    _refit(info, len(idx), info["n_nodes"])
    assert info["has_tree"] == 1 and info["n_nodes"] > 0
    after = O.render(edited, ocam, W, H, SPP, DEPTH, seed=SEED)
    assert not np.array_equal(before[1], after[1])
    tree = ctx.download(W, H) + (st,)
    _same_frame(tree, after)
    monkeypatch.setenv("FR_BVH", "0")  # the in-order loop over the same copy: the same bits
    ctx.render(sc, cam, p)
    st = ctx.sync()
    info = ctx.scene_info(sc)
    assert info["last_sync"] == 0 and (info["packs"], info["refits"]) == (1, 1)
    loop = ctx.download(W, H) + (st,)
    _same_frame(loop, after)
    assert np.array_equal(loop[0].view(np.uint32), tree[0].view(np.uint32)) and np.array_equal(loop[1], tree[1])
    ctx.close()
    sc.close()


def _tile_threshold(comp):
    """A threshold between the tiles' largest relative errors: some tiles active, some not."""
    rel = comp.rel()
    tmax = np.array([[rel[8 * s:8 * s + 8, 8 * c:8 * c + 8].max() for c in range(comp.shape[1])] for s in range(comp.shape[0])])
    thr = float(np.sort(tmax.ravel())[tmax.size // 2])
    mask, summary = comp.select(thr, 0)
    assert 0 < summary["active_tiles"] < summary["tiles"]
    return thr, mask, summary


def test_adaptive_sampling_after_an_in_place_edit(gpu):
    """The tile list belongs to the accumulation, which an edit ends (the copy's uid moves). As
    documented (include/forma_rt.h, FR_FLAG_ADAPTIVE) an adaptive frame that would start a new
    accumulation is refused; the next accumulating frame traces every tile of the edited scene, and
    the list built from then on is the edited scene's."""
    kind = "sphere"
    prims, (idx, new), moved, cam, ocam = _frame_case(gpu, kind, "big", "classes")
    tiles = ((H + 7) // 8) * ((W + 7) // 8)
    P = lambda k, mode: gpu.make_params(W, H, SPP, DEPTH, seed=SEED + k, accumulate=mode)  # noqa: E731
    S_ = lambda pl, k: _frame_sum(O.render(pl, ocam, W, H, SPP, DEPTH, seed=SEED + k)[0], SPP)  # noqa: E731
    comp = AR.AdaptiveComposite(W, H)
    for k in range(2):
        comp.add(S_(prims, k), SPP)
    thr, mask, summary = _tile_threshold(comp)
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    for k in range(2):
        ctx.render(sc, cam, P(k, "error"))
    assert ctx.adapt(thr)["active_tiles"] == summary["active_tiles"]
    for k in (2, 3):  # two adaptive frames on the list
        ctx.render(sc, cam, P(k, "adaptive"))
        want = comp.add(S_(prims, k), SPP, mask)
        assert ctx.sync()["samples"] == int(comp.pixels(mask).sum()) * SPP
    assert np.array_equal(ctx.download(W, H)[0].view(np.uint32), want.view(np.uint32))
    assert ctx.accum_info() == (4, 4 * SPP)
    sc.update(idx, new)
    _refused(gpu, lambda: ctx.render(sc, cam, P(4, "adaptive")), "would start a new accumulation")
    _refit(ctx.scene_info(sc), len(idx))  # (the refused frame had caught the copy up)
    assert ctx.accum_info() == (4, 4 * SPP)
    ctx.render(sc, cam, P(4, "error"))
    st = ctx.sync()
    info = ctx.scene_info(sc)
    assert info["last_sync"] == 0 and (info["packs"], info["refits"]) == (1, 1)
    assert ctx.accum_info() == (1, SPP) and st["samples"] == W * H * SPP  # every tile
    frame = ctx.download(W, H)
    _same_frame(frame + (st,), O.render(moved, ocam, W, H, SPP, DEPTH, seed=SEED + 4))
    n, k = ctx.download_counts()
    assert (n == SPP).all() and (k == 1).all()
    _refused(gpu, lambda: ctx.render(sc, cam, P(5, "adaptive")), "no tile list")
    # a fresh context's first frame of the edited scene: the same bits
    other, fresh = gpu.RenderContext(0), gpu.Scene.from_prims(moved)
    other.render(fresh, cam, P(4, "error"))
    other.sync()
    got = other.download(W, H)
    assert np.array_equal(got[0].view(np.uint32), frame[0].view(np.uint32)) and np.array_equal(got[1], frame[1])
    # the list built next is the edited scene's
    comp2 = AR.AdaptiveComposite(W, H)
    for k in (4, 5):
        comp2.add(S_(moved, k), SPP)
    thr2, mask2, summary2 = _tile_threshold(comp2)
    for c, s in ((ctx, sc), (other, fresh)):
        c.render(s, cam, P(5, "error"))
        assert c.adapt(thr2)["active_tiles"] == summary2["active_tiles"]
        c.render(s, cam, P(6, "adaptive"))
        assert c.sync()["samples"] == int(comp2.pixels(mask2).sum()) * SPP
    want = comp2.add(S_(moved, 6), SPP, mask2)
    for c in (ctx, other):
        assert np.array_equal(c.download(W, H)[0].view(np.uint32), want.view(np.uint32))
    assert tiles == summary2["tiles"]
    ctx.close()
    other.close()
    fresh.close()
    sc.close()


def test_temporal_reuse_after_an_in_place_edit(gpu):
    """The history is keyed on the copy's uid: after an edit in place the next fr_ctx_temporal
    starts from an empty prior (every pixel FR_TP_NO_HISTORY, no source), as on a fresh context with
    the edited scene, and reprojects nothing of the picture before the edit."""
    kind = "sphere"
    prims, (idx, new), moved, cam, ocam = _frame_case(gpu, kind, "big", "classes")
    P = lambda k: gpu.make_params(W, H, SPP, DEPTH, seed=SEED + k, accumulate="error")  # noqa: E731

    def view(ctx, sc, k0, levels, guide):
        for k in range(2):
            ctx.render(sc, cam, P(k0 + k))
        ctx.gbuffer(sc, cam, W, H)
        ctx.temporal(levels, 4.0, guide)
        return ctx.download_temporal(W, H), ctx.download_denoised(W, H, want_var=True)

    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    t, _ = view(ctx, sc, 0, 0, None)
    assert (t["reason"] == T.NO_HISTORY).all()
    ctx.accum_reset()  # the control: a new accumulation of the same upload does reuse the history
    t, _ = view(ctx, sc, 2, 0, None)
    assert (t["reason"] == T.REUSED).any() and t["prior_n"].any()
    sc.update(idx, new)
    fresh, other = gpu.Scene.from_prims(moved), gpu.RenderContext(0)
    for levels, guide in ((0, None), (4, {})):
        if levels:
            ctx.accum_reset(), other.accum_reset()
            ctx.temporal_reset(), other.temporal_reset()
            sc.update(idx, [prims[int(i)] for i in idx])
            view(ctx, sc, 0, 0, None)  # a history of the unedited scene again
            sc.update(idx, new)
        got, pic = view(ctx, sc, 4, levels, guide)
        want, wpic = view(other, fresh, 4, levels, guide)
        assert ctx.scene_info(sc)["refits"] >= 1 and ctx.scene_info(sc)["packs"] == 1
        assert (got["reason"] == T.NO_HISTORY).all() and (got["source"] == T.NONE).all() and not got["prior_n"].any()
        for f in T.FIELDS:
            if f in ("source", "reason"):
                assert np.array_equal(got[f], want[f]), f
            else:
                assert N.same_bits_nan(got[f], want[f]), f
        assert N.same_bits_nan(pic[0], wpic[0]) and np.array_equal(pic[1], wpic[1]) and N.same_bits(pic[2], wpic[2])
    # and the accumulation under it is the edited scene's
    comp_mean = O.render(moved, ocam, W, H, SPP, DEPTH, seed=SEED + 4)[0]
    comp_sum = (_frame_sum(comp_mean, SPP) + _frame_sum(O.render(moved, ocam, W, H, SPP, DEPTH, seed=SEED + 5)[0], SPP)).astype(F)
    assert np.array_equal(got["total_a"].view(np.uint32), comp_sum.view(np.uint32))
    ctx.close()
    other.close()
    fresh.close()
    sc.close()
