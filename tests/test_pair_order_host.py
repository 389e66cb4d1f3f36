"""The mirrored box pair's test in ray order (rt_core.h slab_pair_root) without a device.

tests/c/pair_order_check.cpp, a CPU program built with -fsanitize=address,undefined
-fno-sanitize-recover=all -ffp-contract=off, runs the pair form and the list in order (slab3_fused +
slab_root on the first box, then on the second) on scene_08's pair shapes, a separated and a
touching synthetic pair, each in both list orders, over every combination of the origin and
direction components its header lists, and three bounds per hit. It exits non-zero on the first
difference in the hit decision, the winner's index or the accepted t's bits: there is no allowance.

The constructed tie rays (an origin inside either box of a touching pair, leaving through the shared
plane) must reach equal accepted roots, and the winner must be the list's first box: the oracle is
asked first, then the program's two forms."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests.test_plan import ROOT

SHAPES = ["scene08_0_1", "scene08_1_0", "scene08_3_4", "scene08_4_3", "scene08_2_5", "scene08_5_2", "separated_x",
          "separated_x_rev", "touching_z", "touching_z_rev"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pair_order") / "pair_order_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math",
                    os.path.join(ROOT, "tests", "c", "pair_order_check.cpp"), "-o", out], check=True, timeout=600)
    return out


def _run(exe_path, args=()):
    """The stand-alone sanitizer program: it must end clean."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, *args], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return p.stdout


def test_pair_form_equals_the_list_in_order(check):
    rows = [json.loads(ln) for ln in _run(check).splitlines()]
    print(rows)
    assert [r["shape"] for r in rows] == SHAPES
    for r in rows:
        # 17 special values and the two boxes' four coordinates with their neighbours, per component
        assert r["component_combos"] == [29 * 29] * 3
        assert r["rays"] == r["distinct"][0] * r["distinct"][1] * r["distinct"][2]
        assert r["tests"] == r["rays"] + 2 * r["hits"]
        # both boxes win: the second one of the list too
        assert 0 < r["second_wins"] < r["hits"]
    # a list order and its reverse see the same rays: the second box's wins and ties aside, the same hits
    for a, b in zip(rows[0::2], rows[1::2]):
        assert (a["rays"], a["hits"]) == (b["rays"], b["hits"])


def _tie_rows(check):
    rows = []
    for ln in _run(check, ["ties"]).splitlines():
        f = ln.split()
        v = [float.fromhex(x) for x in f[1:19]]
        rows.append({"shape": f[0], "first": v[0:6], "second": v[6:12], "o": v[12:15], "d": v[15:18],
                     "winner": int(f[19]), "t_bits": int(f[20], 16), "tie": int(f[21])})
    return rows


def test_tie_rays_leave_the_lists_first_box(check):
    rows = _tie_rows(check)
    assert sorted({r["shape"] for r in rows}) == sorted(["scene08_0_1", "scene08_1_0", "touching_z", "touching_z_rev"])
    ties = 0
    for r in rows:
        prims = [S.prim(S.AABB, S.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0, r[k]) for k in ("first", "second")]
        best, rec = O.closest_hit(prims, r["o"], r["d"])
        # the reference first: its winner and its t are what the two forms returned
        assert best == r["winner"], r
        assert int(np.float32(rec[0]).view(np.uint32)) == r["t_bits"], (r, rec)
        if r["tie"]:
            ties += 1
            assert best == 0, r
    # per shape: from inside either box towards the shared plane, whichever the ray meets first
    assert ties == 2 * 4


def test_scene_08_camera_wall_tie_is_box_0():
    """scene_08 itself: boxes 0 and 1 touch at y = 0. A ray from inside box 1 down through that
    plane meets box 1 first and ties with box 0's entry: the oracle's winner is box 0."""
    import forma_rt as fr
    with open(fr.scene_path("scene_08")) as f:
        prims, _ = S.load_json(f.read())
    g0, g1 = prims[0]["g"], prims[1]["g"]
    assert g0[4] == 0.0 and g1[1] == 0.0 and g0[1] == -g1[4]  # y: [-30, 0] and [0, 30]
    for o, d, want in (((0.01, 0.5, 0.0), (0.001, -1.0, 0.002), 0), ((0.01, -0.5, 0.0), (0.001, 1.0, 0.002), 0)):
        best, _ = O.closest_hit(prims, o, d)
        assert best == want, (o, d, best)
