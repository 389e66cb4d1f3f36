"""Geometry edits in place (fr_scene_update) on the GPU, bit for bit against the oracle.

A geometric edit leaves the scene's device copy where it is: the edited primitives' records are
scattered by scene_patch_kernel and every node of the tree is recomputed by bvh_refit_kernel,
inside the next call that uses the scene. Every test that means that path asserts
FR_SCENE_SYNC_REFIT in scene_info, so none passes on a silent re-pack; the fallbacks must read
FR_SCENE_SYNC_PACK. Scenes, rays and move sets: tests/refit_fixtures.py (held against the oracle
and tests/c/refit_check.cpp by tests/test_refit_fixtures.py and tests/test_refit_host.py)."""
import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import gbuffer_ref as G
from tests import occlude_fixtures as OF
from tests import ray_edge_fixtures as X
from tests import refit_fixtures as R
from tests.test_accum_error import _refused
from tests.test_plan import ROOT

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, DEPTH, SEED = 32, 24, 4, 4, 5

_cache = {}


def _moved_hits(gpu, kind):
    if ("hits", kind) not in _cache:
        b = CF.batch(gpu, kind)
        _cache["hits", kind] = CF.hits(R.moved_prims(kind), b["o"], b["d"])
    return _cache["hits", kind]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return R.build_check(ROOT, str(tmp_path_factory.mktemp("refit_gpu") / "refit_check"))


def _refit(info, prims, nodes=None):
    assert info["last_sync"] == 2, info  # FR_SCENE_SYNC_REFIT
    assert info["prims_patched"] == prims, info
    if nodes is not None:
        assert info["nodes_refit"] == nodes and (info["refit_launches"] >= 1) == (nodes > 0), info


def _packed(info):
    assert info["last_sync"] == 1, info  # FR_SCENE_SYNC_PACK


@pytest.mark.parametrize("kind", R.KINDS)
def test_cast_after_a_move(gpu, kind):
    b = CF.batch(gpu, kind)
    sc = gpu.Scene.from_prims(b["prims"])
    ctx = gpu.RenderContext(0)
    assert CF.same(ctx.cast(sc, b["o"], b["d"]), CF.expected(gpu, kind)) == []
    first = ctx.scene_info(sc)
    _packed(first)
    assert first["has_tree"] == 1 and first["n_nodes"] > 0 and (first["packs"], first["refits"]) == (1, 0)
    idx, new = R.move_set(kind)
    sc.update(idx, new)
    got = ctx.cast(sc, b["o"], b["d"])
    info = ctx.scene_info(sc)
    _refit(info, len(idx), first["n_nodes"])
    assert (info["packs"], info["refits"]) == (1, 1) and info["edit_seq"] == 1 and info["version"] == first["version"]
    assert CF.same(got, _moved_hits(gpu, kind)) == []
    ci = ctx.cast_info()
    assert ci["tree"] == 1 and ci["waves_tree"] > 0
    # the host list is the edited one
    words = R.prim_words(R.moved_prims(kind))
    have = np.array([np.frombuffer(bytes(p), np.uint32) for p in sc.prims()])
    assert np.array_equal(have, words)
    # a second cast finds the copy current
    assert CF.same(ctx.cast(sc, b["o"], b["d"]), _moved_hits(gpu, kind)) == []
    assert ctx.scene_info(sc)["last_sync"] == 0
    ctx.close()


@pytest.mark.parametrize("kind", R.KINDS)
def test_tables_equal_the_host_refit(gpu, check, tmp_path, kind):
    b = CF.batch(gpu, kind)
    prims = b["prims"]
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    none = np.zeros((0, 3), F)
    ctx.cast(sc, b["o"][:64], b["d"][:64])
    names = ("records", "leaf_records", "leaf_order", "nodes")
    first = {n: sc.download_table(0, n) for n in names}
    _, _, _, host0 = R.run_check(check, tmp_path, kind + "0", prims, [], [], none, none, tables=True)
    for n in names:
        assert np.array_equal(first[n], host0[n]), n
    idx, new = R.move_set(kind)
    sc.update(idx, new)
    ctx.cast(sc, b["o"][:64], b["d"][:64])
    _refit(ctx.scene_info(sc), len(idx))
    _, _, _, host = R.run_check(check, tmp_path, kind, prims, idx, new, none, none, tables=True)
    for n in names:
        assert np.array_equal(sc.download_table(0, n), host[n]), n
    assert not np.array_equal(host["nodes"], host0["nodes"]) and not np.array_equal(host["records"], host0["records"])
    sc.update(idx, [prims[int(i)] for i in idx])  # everything back
    ctx.cast(sc, b["o"][:64], b["d"][:64])
    _refit(ctx.scene_info(sc), len(idx))
    for n in names:
        assert np.array_equal(sc.download_table(0, n), first[n]), n
    ctx.close()


@pytest.mark.parametrize("kind", R.KINDS)
def test_occlusion_and_gbuffer_after_a_move(gpu, kind):
    w = h = 16
    cam, ocam = X.edge_camera(gpu, w=w, h=h, **X.fixture(kind, "R0_control").cam)
    o, d = CF.camera_rays(ocam, w, h)
    moved = R.moved_prims(kind)
    t_max = OF.t_max_of(CF.hits(moved, o, d)["t"])
    want = OF.ranged(moved, o, d, t_max)["occluded"]
    sc = gpu.Scene.from_prims(CF.lattice_prims(kind))
    ctx = gpu.RenderContext(0)
    ctx.occluded(sc, o, d, t_max=t_max)
    idx, new = R.move_set(kind)
    sc.update(idx, new)
    got = ctx.occluded(sc, o, d, t_max=t_max)
    _refit(ctx.scene_info(sc), len(idx))
    assert np.array_equal(got, want) and want.any() and not want.all()
    assert ctx.occluded_info()["tree"] == 1
    # the G-buffer is the first use after another edit: back, and moved again
    sc.update(idx, [CF.lattice_prims(kind)[int(i)] for i in idx])
    ctx.gbuffer(sc, cam, w, h)
    _refit(ctx.scene_info(sc), len(idx))
    assert G.same(ctx.download_gbuffer(w, h), G.gbuffer(CF.lattice_prims(kind), ocam, w, h)) == []
    sc.update(idx, new)
    ctx.gbuffer(sc, cam, w, h)
    _refit(ctx.scene_info(sc), len(idx))
    assert ctx.gbuffer_info() == "tree"
    assert G.same(ctx.download_gbuffer(w, h), G.gbuffer(moved, ocam, w, h)) == []
    ctx.close()


@pytest.mark.parametrize("kind", ["sphere", "mixed"])
def test_five_successive_move_sets(gpu, kind):
    b = CF.batch(gpu, kind)
    sc = gpu.Scene.from_prims(b["prims"])
    ctx, other = gpu.RenderContext(0), gpu.RenderContext(0)
    ctx.cast(sc, b["o"], b["d"])
    cur = list(b["prims"])
    steps = [R.move_set(kind)] + R.successive(kind)[:4]
    for k, (idx, new) in enumerate(steps):
        sc.update(idx, new)
        cur = R.applied(cur, idx, new)
        got = ctx.cast(sc, b["o"], b["d"])
        info = ctx.scene_info(sc)
        _refit(info, len(idx))
        assert info["refits"] == k + 1 and info["packs"] == 1
        assert CF.same(got, CF.hits(cur, b["o"], b["d"])) == [], k
        fresh = gpu.Scene.from_prims(cur)
        assert CF.same(got, other.cast(fresh, b["o"], b["d"])) == [], k
        fresh.close()
    ctx.close()
    other.close()


def _frame_case(gpu, kind, size, variant):
    """(prims, edit, moved prims, FrCamera, OrCamera) of a rendered-frame case: the kind's move set
    on the big lattice, the first two cells moved on a small one."""
    prims = X.lattice(kind, size, 0, variant)
    if size == "big":
        idx = np.array([i for i, _ in R.MOVES[kind]], np.uint32)
        new = [R.translated(prims[i], dd) for i, dd in R.MOVES[kind]]
    else:
        idx = np.array([0, 1], np.uint32)
        new = [R.translated(prims[0], (0.0, -2.5, 2.5)), R.translated(prims[1], (0.0, 2.5, 1.0))]
    cam, ocam = X.edge_camera(gpu, w=W, h=H, **X.fixture(kind, "R0_control").cam)
    return prims, (idx, new), R.applied(prims, idx, new), cam, ocam


def _same_frame(got, want):
    mean, u8, st = got
    omean, ou8, ocnt, _ = want
    assert np.array_equal(mean.view(np.uint32), omean.view(np.uint32)), \
        int((mean.view(np.uint32) != omean.view(np.uint32)).any(axis=2).sum())
    assert np.array_equal(u8, ou8)
    assert (st["segments"], st["hits"], st["scatters"]) == (ocnt["segments"], ocnt["hits"], ocnt["scatters"])


@pytest.mark.parametrize("kind,size,variant,jit", [("sphere", "big", "classes", False), ("sphere", "big", "full", False),
                                                   ("box", "small", "full", False), ("box", "small", "full", "wait")])
def test_rendered_frames_after_a_move(gpu, kind, size, variant, jit):
    """The class-record BVH kernel, the 12-B-record BVH kernel, the list kernel (records patched,
    no tree) and the scene-specialised list kernel, whose constants are the records."""
    prims, (idx, new), moved, cam, ocam = _frame_case(gpu, kind, size, variant)
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    p = gpu.make_params(W, H, SPP, DEPTH, seed=SEED, scene_jit=jit)
    ctx.render(sc, cam, p)
    st = ctx.sync()
    before = O.render(prims, ocam, W, H, SPP, DEPTH, seed=SEED)
    _same_frame(ctx.download(W, H) + (st,), before)
    if jit:
        assert ctx.jit_info()["used"]
    sc.update(idx, new)
    ctx.render(sc, cam, p)
    st = ctx.sync()
    info = ctx.scene_info(sc)
    _refit(info, len(idx))
    assert info["has_tree"] == (1 if size == "big" else 0)
    assert (info["nodes_refit"] > 0) == (size == "big")
    after = O.render(moved, ocam, W, H, SPP, DEPTH, seed=SEED)
    assert not np.array_equal(before[1], after[1])
    _same_frame(ctx.download(W, H) + (st,), after)
    if jit:
        assert ctx.jit_info()["used"]
    ctx.close()


def test_streamed_frames_with_an_update_before_each(gpu):
    kind = "box"
    prims, (idx, new), moved, cam, ocam = _frame_case(gpu, kind, "big", "full")
    steps = [(idx, new)] + R.successive(kind)[:2]
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    p = gpu.make_params(W, H, SPP, DEPTH, seed=SEED)
    ctx.render(sc, cam, p)
    ctx.sync()
    frames = [gpu.PinnedFrame(W, H) for _ in steps]
    cur, states = list(prims), []
    for (i, n), fr_ in zip(steps, frames):
        sc.update(i, n)
        cur = R.applied(cur, i, n)
        states.append(cur)
        ctx.render(sc, cam, p)
        _refit(ctx.scene_info(sc), len(i))
        ctx.download_async(fr_)
    st = ctx.sync()
    ctx.wait()
    for k, (state, fr_) in enumerate(zip(states, frames)):
        want = O.render(state, ocam, W, H, SPP, DEPTH, seed=SEED)
        assert np.array_equal(fr_.mean.view(np.uint32), want[0].view(np.uint32)), k
        assert np.array_equal(fr_.u8, want[1]), k
    assert st["segments"] == want[2]["segments"]
    for fr_ in frames:
        fr_.close()
    ctx.close()


def test_an_update_restarts_the_accumulation(gpu):
    kind = "sphere"
    prims, (idx, new), moved, cam, ocam = _frame_case(gpu, kind, "big", "classes")
    sc = gpu.Scene.from_prims(prims)
    ctx = gpu.RenderContext(0)
    for k in range(2):
        ctx.render(sc, cam, gpu.make_params(W, H, SPP, DEPTH, seed=SEED + k, accumulate="error"))
    assert ctx.accum_info() == (2, 2 * SPP)
    ctx.gbuffer(sc, cam, W, H)
    ctx.denoise(guided=True)  # accepted: the G-buffer is of this upload
    sc.update(idx, new)
    ctx.render(sc, cam, gpu.make_params(W, H, SPP, DEPTH, seed=SEED + 2, accumulate="error"))
    _refit(ctx.scene_info(sc), len(idx))
    assert ctx.accum_info() == (1, SPP)
    st = ctx.sync()
    _same_frame(ctx.download(W, H) + (st,), O.render(moved, ocam, W, H, SPP, DEPTH, seed=SEED + 2))
    ctx.render(sc, cam, gpu.make_params(W, H, SPP, DEPTH, seed=SEED + 3, accumulate="error"))
    assert ctx.accum_info() == (2, 2 * SPP)
    _refused(gpu, lambda: ctx.denoise(guided=True), "another scene upload")
    ctx.close()


def test_two_contexts_on_one_device(gpu):
    kind = "obb"
    b = CF.batch(gpu, kind)
    sc = gpu.Scene.from_prims(b["prims"])
    a, c = gpu.RenderContext(0), gpu.RenderContext(0)
    a.cast(sc, b["o"], b["d"])
    c.cast(sc, b["o"], b["d"])
    assert (a.scene_info(sc)["last_sync"], c.scene_info(sc)["last_sync"]) == (1, 0)
    idx, new = R.move_set(kind)
    sc.update(idx, new)
    # no sync between the two: the second context's stream waits for the first one's patch
    rays = _rays(b)  # (host rays are copied before the call returns)
    gpu.check(gpu.lib().fr_ctx_cast(a._h, sc._h, rays.ctypes.data, len(rays), 0))
    got_c = c.cast(sc, b["o"], b["d"])
    got_a = a.download_hits(len(b["o"]))
    _refit(a.scene_info(sc), len(idx))
    ic = c.scene_info(sc)
    assert ic["last_sync"] == 0 and (ic["packs"], ic["refits"]) == (1, 1)
    assert CF.same(got_a, _moved_hits(gpu, kind)) == [] and CF.same(got_c, _moved_hits(gpu, kind)) == []
    a.close()
    c.close()


def _rays(b):
    rays = np.zeros((len(b["o"]), 8), F)
    rays[:, 0:3], rays[:, 4:7] = b["o"], b["d"]
    return rays


def test_multi_context_shards_catch_up(gpu):
    kind = "sphere"
    prims, (idx, new), moved, cam, ocam = _frame_case(gpu, kind, "big", "classes")
    sc = gpu.Scene.from_prims(prims)
    mc = gpu.MultiContext([0, 0])
    p = gpu.make_params(W, H, SPP, DEPTH, seed=SEED)
    mc.render(sc, cam, p)
    mc.sync()
    sc.update(idx, new)
    mc.render(sc, cam, p)
    st = mc.sync()
    kinds = sorted(mc.context(i).scene_info(sc)["last_sync"] for i in range(2))
    assert kinds == [0, 2], kinds  # one device, one copy: one shard patched it, the other waited for its event
    assert mc.context(0).scene_info(sc)["refits"] == 1
    mean, u8 = mc.frame()
    _same_frame((mean, u8, st), O.render(moved, ocam, W, H, SPP, DEPTH, seed=SEED))
    mc.close()


@pytest.mark.parametrize("kind", R.KINDS)
def test_fallbacks_pack_again(gpu, kind):
    b = CF.batch(gpu, kind)
    prims = b["prims"]
    o, d = b["o"][:512], b["d"][:512]
    ctx = gpu.RenderContext(0)
    edits = dict(R.structural_edits(kind), outside=R.outside_move(kind), nonfinite=R.nonfinite_move(kind))
    for name, (idx, new) in edits.items():
        sc = gpu.Scene.from_prims(prims)
        ctx.cast(sc, o, d)
        sc.update(idx, new)
        got = ctx.cast(sc, o, d)
        _packed(ctx.scene_info(sc))
        assert ctx.scene_info(sc)["packs"] == 2, name
        assert CF.same(got, CF.hits(R.applied(prims, idx, new), o, d)) == [], name
        sc.close()
    idx, new = R.move_set(kind)
    moved = CF.hits(R.moved_prims(kind), o, d)
    sc = gpu.Scene.from_prims(prims)
    ctx.cast(sc, o, d)
    sc.update(idx, new, rebuild=True)  # FR_UPDATE_REBUILD
    assert CF.same(ctx.cast(sc, o, d), moved) == []
    _packed(ctx.scene_info(sc))
    sc.update(idx, [prims[int(i)] for i in idx])
    ctx.cast(sc, o, d)
    _refit(ctx.scene_info(sc), len(idx))
    sc.update(idx, new)
    sc.rebuild()  # fr_scene_rebuild after a geometric edit: the pack wins
    assert CF.same(ctx.cast(sc, o, d), moved) == []
    _packed(ctx.scene_info(sc))
    # a bad index: FR_EARG, and the list is as it was
    have = [bytes(p) for p in sc.prims()]
    bad = np.array([int(idx[0]), len(prims)], np.uint32)
    with pytest.raises(gpu.ForMaError) as e:
        sc.update(bad, [prims[0], prims[1]])
    assert e.value.code == gpu.FR_EARG
    assert [bytes(p) for p in sc.prims()] == have
    sc.update([], [])  # n = 0: a no-op
    assert ctx.scene_info(sc)["edit_seq"] == 2
    ctx.cast(sc, o, d)
    assert ctx.scene_info(sc)["last_sync"] == 0
    sc.close()
    ctx.close()


def test_the_deep_tree(gpu, check, tmp_path):
    """10,000 spheres, every one moved by its own y offset through set_spheres: one refit of every
    node, through every height of the tree."""
    w = h = 16
    prims, o, d, _ = CF.gen_batch(gpu, 10000, w, h)
    text = CF.gen_spheres(gpu, 10000, w, h)[0]
    sc = gpu.Scene.from_json(text, w, h)
    ctx = gpu.RenderContext(0)
    ctx.cast(sc, o, d)
    first = ctx.scene_info(sc)
    moved = R.gen_moved(prims)
    centers = np.array([p["g"][:3] for p in moved], F)
    sc.set_spheres(None, centers)
    got = ctx.cast(sc, o, d)
    info = ctx.scene_info(sc)
    _refit(info, len(prims), first["n_nodes"])
    assert info["refit_launches"] >= 8 and first["n_nodes"] > 2000
    assert CF.same(got, CF.hits(moved, o, d)) == []
    assert ctx.cast_info() == {"n": len(o), "tree": 1, "waves_tree": (len(o) + 63) // 64, "waves_list": 0}
    _, _, _, host = R.run_check(check, tmp_path, "deep", prims, np.arange(len(prims)), moved, o[:0], d[:0], tables=True)
    assert np.array_equal(sc.download_table(0, "nodes"), host["nodes"])
    assert np.array_equal(sc.download_table(0, "leaf_records"), host["leaf_records"])
    # set_spheres with indices and radii: a few spheres back to where they were
    sel = np.array([0, 17, 9999], np.uint32)
    sc.set_spheres(sel, np.array([prims[int(i)]["g"][:3] for i in sel], F), radii=np.full(3, 2.5, F))
    ctx.cast(sc, o[:64], d[:64])
    _refit(ctx.scene_info(sc), 3, first["n_nodes"])
    ctx.close()
