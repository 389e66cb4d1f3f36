"""Move sets for the in-place scene edit tests (fr_scene_update): shared by
tests/test_refit_fixtures.py, tests/test_refit_host.py and tests/test_refit.py; not a test module.

The scenes are the "big" lattices of tests/ray_edge_fixtures.py (cells of pitch 2 at x in {0, 2},
y in -6 .. 4, z in -4 .. -14, and a mirror behind the camera) and the rays are the batches of
tests/cast_fixtures.py. A move set lists (index, (dx, dy, dz)): the primitive is translated by
more than the cell pitch to a place that was empty, inside the lattice's extent (16; 130 for the
sphere lattice, from its radius-64 sphere), and mostly in front of the first layer, where the
batch's rays see it. The indices were chosen from the trees the builder makes for these lists
(tests/c/refit_check.cpp prints where each edited primitive sits) so that every set holds two
primitives of one leaf, primitives of both children of one node and a primitive under each child
of the root; tests/test_refit_fixtures.py checks those properties against the program, so a change
of the builder that breaks them is seen there and not as a vacuous pass of the GPU tests.

Also per kind: an `outside` move (past the extent: the copy must be packed again), `structural`
edits (a colour change and a kind change) and a non-finite centre."""
import copy
import os
import subprocess

import numpy as np

from oracle import scene_ref as S
from tests import cast_fixtures as CF

F = np.float32
KINDS = ("box", "sphere", "obb", "tri", "mixed")
EXTENT = {"box": 16.0, "sphere": 130.0, "obb": 16.0, "tri": 16.0, "mixed": 16.0}

# (index, delta) per kind; see the module docstring
_BOXY = ((0, (0.0, -2.5, 2.5)), (14, (-4.0, 0.0, 0.0)), (5, (0.0, 0.0, 2.5)), (12, (4.0, 0.0, 0.0)), (54, (0.0, 0.0, 3.0)))
MOVES = {
    "box": _BOXY,
    "sphere": ((0, (0.0, -2.5, 2.5)), (6, (-4.0, 0.0, 0.0)), (5, (0.0, 0.0, 2.5)), (12, (4.0, 0.0, 0.0)), (54, (3.0, 0.0, 0.0))),
    "obb": _BOXY,
    "tri": ((0, (0.0, -2.5, 2.5)), (1, (0.0, -2.5, 2.5)), (12, (-4.0, 0.0, 0.0)), (16, (4.0, 0.0, 1.0)), (9, (0.0, 0.0, 2.5)),
            (108, (0.0, 0.0, 3.0))),
    # (5: a plane, 6: a stub)
    "mixed": ((0, (0.0, -2.5, 2.5)), (3, (2.0, 2.5, 2.5)), (4, (2.0, 2.5, 2.5)), (1, (-3.0, 0.0, 0.0)), (5, (0.0, 0.0, 2.5)),
              (6, (1.0, 2.0, 3.0)), (16, (4.0, 0.0, 0.0))),
}
# what refit_check's `topo` lines must show for the sets above: a pair of indices in one leaf, a
# pair under the two children of one node, a pair under the two children of the root
SAME_LEAF = {"box": (0, 14), "sphere": (0, 6), "obb": (0, 14), "tri": (0, 1), "mixed": (3, 4)}
SIBLINGS = {"box": (0, 5), "sphere": (0, 5), "obb": (0, 5), "tri": (12, 16), "mixed": (0, 3)}
ROOT_SIDES = {"box": (0, 54), "sphere": (0, 54), "obb": (0, 54), "tri": (0, 108), "mixed": (1, 0)}


def translated(p, d):
    """A copy of primitive dict p moved by d (a stub's geometry words, which nothing reads, change)."""
    q = copy.deepcopy(p)
    g = [float(x) for x in q["g"]]
    d = [float(x) for x in d]
    spans = {S.SPHERE: 1, S.AABB: 2, S.OBB: 1, S.TRIANGLE: 3, S.PLANE: 1, S.STUB: 1}[p["kind"]]
    for v in range(spans):
        for k in range(3):
            g[3 * v + k] = float(F(g[3 * v + k]) + F(d[k]))
    q["g"] = g
    return q


def own_extent(prims):
    """bvh.cpp's extent of a list: the largest |coordinate| of the bounded primitives' own bounds
    (cast_fixtures.extent_bounds with the oriented boxes' exact spans, which are exact sums here)."""
    m = CF.extent_bounds([p for p in prims if p["kind"] not in (S.OBB, S.PLANE)])[0]
    for p in prims:
        if p["kind"] == S.OBB:
            g = [float(x) for x in p["g"]]
            for k in range(3):
                m = max(m, abs(g[k]) + sum(abs(g[3 + 3 * j + k]) * g[12 + j] for j in range(3)))
    return m


def move_set(kind):
    """(indices [k] uint32, new primitive dicts [k]) of the kind's move set on lattice_prims(kind)."""
    prims = CF.lattice_prims(kind)
    idx = [i for i, _ in MOVES[kind]]
    return np.array(idx, np.uint32), [translated(prims[i], d) for i, d in MOVES[kind]]


def applied(prims, idx, new):
    out = list(prims)
    for i, p in zip(idx, new):
        out[int(i)] = p
    return out


def moved_prims(kind):
    return applied(CF.lattice_prims(kind), *move_set(kind))


def successive(kind, steps=5):
    """`steps` move sets applied one after the other: step s moves the set's primitive s (and the
    next one) further by one pitch along x, alternating sign, staying inside the extent."""
    prims = CF.lattice_prims(kind)
    cur = moved_prims(kind)
    out = []
    base = [m for m in MOVES[kind] if m[0] != len(prims) - 1]  # (the mirror fills the extent in x and y)
    for s in range(steps):
        pick = [base[s % len(base)][0], base[(s + 1) % len(base)][0]]
        pick = list(dict.fromkeys(pick))
        new = [translated(cur[i], (0.0, 2.0 if s % 2 == 0 else -2.0, -0.5 * (s + 1))) for i in pick]
        out.append((np.array(pick, np.uint32), new))
        cur = applied(cur, pick, new)
    assert len(prims) == len(cur)
    return out


def first_movable(kind):
    """The index of the set's first primitive that has bounds (not a plane or a stub)."""
    prims = CF.lattice_prims(kind)
    return next(i for i, _ in MOVES[kind] if prims[i]["kind"] not in (S.PLANE, S.STUB))


def outside_move(kind):
    """One primitive moved past the extent: (indices, prims)."""
    prims = CF.lattice_prims(kind)
    i = first_movable(kind)
    return np.array([i], np.uint32), [translated(prims[i], (0.0, 3.0 * EXTENT[kind], 0.0))]


def structural_edits(kind):
    """{"colour": (indices, prims), "kind": (indices, prims)}: edits that are not geometric."""
    prims = CF.lattice_prims(kind)
    i = first_movable(kind)
    col = copy.deepcopy(prims[i])
    col["color"] = [0.125, 0.5, 0.875]
    other = S.sphere((2.0, 8.0, -4.0), 1.0, prims[i]["material"], prims[i]["color"], prims[i]["fuzz"]) \
        if prims[i]["kind"] != S.SPHERE else \
        S.prim(S.AABB, prims[i]["material"], prims[i]["color"], prims[i]["fuzz"], [1.0, 7.0, -5.0, 3.0, 9.0, -3.0])
    return {"colour": (np.array([i], np.uint32), [col]), "kind": (np.array([i], np.uint32), [other])}


def nonfinite_move(kind):
    """The first movable primitive with a NaN centre: its y moved by NaN, which makes every corner's
    or vertex's y NaN. No bounds and no hit, in the tree or in the list."""
    prims = CF.lattice_prims(kind)
    i = first_movable(kind)
    return np.array([i], np.uint32), [translated(prims[i], (0.0, float("nan"), 0.0))]


def gen_moved(prims):
    """The generator's sphere scene (y from 0 to 4995, the extent's own range) with every sphere
    moved by its own y offset of up to 2 (a multiple of 1 / 16: exact), up in the lower part and
    down in the upper part, so that every sphere stays inside the extent."""
    out = []
    for i, p in enumerate(prims):
        k = ((i * 7) % 32 + 1) / 16.0
        out.append(translated(p, (0.0, k if float(p["g"][1]) < 2000.0 else -k, 0.0)) if p["kind"] == S.SPHERE else p)
    return out


# ---- tests/c/refit_check.cpp ---------------------------------------------------------------------

def prim_words(prims):
    out = []
    for p in prims:
        out += [np.array([p["kind"], p["material"]], np.uint32), np.asarray(p["color"], F).view(np.uint32),
                np.array([p["fuzz"]], F).view(np.uint32), np.asarray(p["g"], F).view(np.uint32)]
    return np.concatenate(out).reshape(len(prims), 22) if prims else np.zeros((0, 22), np.uint32)


def build_check(root, out):
    csrc = os.path.join(root, "fo-rma_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "refit_check.cpp"),
                    os.path.join(csrc, "pack.cpp"), os.path.join(csrc, "bvh.cpp"), "-o", out], check=True, timeout=600)
    return out


def run_check(exe, tmp_path, name, prims, idx, new, o, d, force=False, tables=False):
    """(info dict, topo rows [k, 5], list-loop hit dict of the edited scene, tables dict or None) of
    refit_check. The tables: records, leaf_records, leaf_order, nodes, slot_bounds, node_unions."""
    path = str(tmp_path / f"{name}.bin")
    rays = np.zeros((len(o), 8), F)
    if len(o):
        rays[:, 0:3], rays[:, 4:7] = o, d
    edits = np.concatenate([np.asarray(idx, np.uint32).reshape(-1, 1), prim_words(new)], axis=1) if len(idx) else \
        np.zeros((0, 23), np.uint32)
    np.concatenate([np.array([len(prims), len(o), len(idx), 1 if force else 0], np.uint32), prim_words(prims).reshape(-1),
                    edits.reshape(-1), rays.reshape(-1).view(np.uint32)]).tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    tpath = str(tmp_path / f"{name}.tables")
    p = subprocess.run([exe, path] + ([tpath] if tables else []), capture_output=True, text=True, timeout=600, env=env)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines and lines[0].startswith("info "), (p.returncode, p.stderr[-2000:])
    tok = lines[0].split()[1:]
    info = {k: int(v) for k, v in zip(tok[0::2], tok[1::2])}
    info["returncode"] = p.returncode
    k = len(idx)
    topo = np.array([[int(t, 16) if c else int(t) for c, t in enumerate(line.split()[1:])] for line in lines[1:1 + k]],
                    np.int64).reshape(k, 5)
    rows = np.array([[int(t, 16) for t in line.split()] for line in lines[1 + k:]], np.uint32).reshape(len(o), 12)
    got = {"prim": rows[:, 0].copy(), "t": rows[:, 1].copy().view(F), "normal": np.ascontiguousarray(rows[:, 2:5]).view(F),
           "position": np.ascontiguousarray(rows[:, 5:8]).view(F), "albedo": np.ascontiguousarray(rows[:, 8:11]).view(F),
           "fallback": rows[:, 11] != 0}  # (cast_fallback at the packed reach; CF.same does not read it)
    tabs = None
    if tables:
        w = np.fromfile(tpath, np.uint32)
        n, slots, nodes = int(w[0]), int(w[1]), int(w[2])
        assert int(w[3]) == 1, f"refit_check TABLES format {int(w[3])}, this reader knows 1"
        at = 4
        tabs = {}
        for key, rows_, width in (("records", n, 16), ("leaf_records", slots, 16), ("leaf_order", slots, 1), ("nodes", nodes, 16),
                                  ("slot_bounds", slots, 8), ("node_unions", nodes, 8)):
            tabs[key] = w[at:at + rows_ * width].reshape(rows_, width)
            at += rows_ * width
        assert at == len(w)
    return info, topo, got, tabs
