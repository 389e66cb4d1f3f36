"""In-place scene edits without a device: tests/c/refit_check.cpp, a CPU program built with
-fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off together with the
library's packer and tree builder.

- bvh_refit over the unmoved primitives reproduces the builder's nodes byte for byte: every big
  lattice, every bundled scene with the tree forced, the 10,000-sphere generator scene.
- After each move set the refitted tables pass cast.h's host walks: tree = list = oracle.
- The old nodes with the new records do not (the stale-tree control).
- Moving everything back restores the first tables byte for byte.
- The height schedule lists every node once, after both of its children."""
import glob
import os

import numpy as np
import pytest

from oracle import scene_ref as S
from tests import cast_fixtures as CF
from tests import ray_edge_fixtures as X
from tests import refit_fixtures as R
from tests.test_plan import ROOT

NONE = np.zeros((0, 3), np.float32)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return R.build_check(ROOT, str(tmp_path_factory.mktemp("refit") / "refit_check"))


def _clean(info):
    return info["returncode"] == 0 and info["refit"] == 0 and info["sched"] == 0 and info["mismatch"] == 0 and \
        info["restore"] == 0


@pytest.mark.parametrize("kind", X.KINDS)
def test_refit_reproduces_the_builder_on_the_lattices(check, tmp_path, fr, kind):
    prims = X.lattice(kind, "big", 0)
    info, _, _, _ = R.run_check(check, tmp_path, kind, prims, [], [], NONE, NONE)
    assert _clean(info), info
    assert info["tree"] == (0 if kind == "plane" else 1)
    if info["tree"]:
        assert info["nodes"] > 0 and 1 <= info["heights"] <= 16


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ROOT, "fo-rma_amd", "scenes", "scene_*.min.json"))),
                         ids=lambda p: os.path.basename(p)[:8])
def test_refit_reproduces_the_builder_on_the_bundled_scenes(check, tmp_path, path):
    with open(path) as f:
        prims, _ = S.load_json(f.read())
    info, _, _, _ = R.run_check(check, tmp_path, "scene", prims, [], [], NONE, NONE, force=True)
    assert _clean(info), info
    assert info["tree"] == (1 if prims else 0)  # (scene_07 is empty)


def test_refit_reproduces_the_builder_on_10000_spheres(check, tmp_path, fr):
    prims = CF.gen_spheres(fr, 10000, 16, 16)[1]
    info, _, _, _ = R.run_check(check, tmp_path, "gen", prims, [], [], NONE, NONE)
    assert _clean(info), info
    assert info["tree"] == 1 and info["nodes"] > 2000 and info["heights"] >= 8


@pytest.mark.parametrize("kind", R.KINDS)
def test_move_sets_refit_to_the_oracle(check, tmp_path, fr, kind):
    b = CF.batch(fr, kind)
    idx, new = R.move_set(kind)
    info, _, got, _ = R.run_check(check, tmp_path, kind, b["prims"], idx, new, b["o"], b["d"])
    print(kind, "stale-tree wrong rays:", info["stale"])
    assert _clean(info), info
    assert info["tree"] == 1 and info["patchable"] == 1
    assert info["stale"] >= 1
    assert CF.same(got, CF.hits(R.moved_prims(kind), b["o"], b["d"])) == []


@pytest.mark.parametrize("kind", R.KINDS)
def test_successive_sets_refit_to_the_oracle(check, tmp_path, fr, kind):
    """The accumulated state after five further sets, applied as one edit of the first pack."""
    b = CF.batch(fr, kind)
    prims = b["prims"]
    cur = R.moved_prims(kind)
    for idx, new in R.successive(kind):
        cur = R.applied(cur, idx, new)
    idx = [i for i in range(len(prims)) if cur[i] is not prims[i]]
    info, _, got, _ = R.run_check(check, tmp_path, kind, prims, idx, [cur[i] for i in idx], b["o"], b["d"])
    assert _clean(info), info
    assert info["patchable"] == 1
    assert CF.same(got, CF.hits(cur, b["o"], b["d"])) == []


def test_the_deep_tree_refits_every_level(check, tmp_path, fr):
    prims, o, d, _ = CF.gen_batch(fr, 10000, 16, 16)
    moved = R.gen_moved(prims)
    info, _, got, _ = R.run_check(check, tmp_path, "gen_moved", prims, np.arange(len(prims)), moved, o, d)
    assert _clean(info), info
    assert info["patchable"] == 1 and info["heights"] >= 8
    assert CF.same(got, CF.hits(moved, o, d)) == []
