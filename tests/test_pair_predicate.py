"""Which boxes the scene kernel tests as a mirrored pair (trace_kernel.h jit_pair_axis over its
constant records, rt_core.h slab_mirror_axis), asked of the kernel's own constant expression. No
GPU: hipcc parses trace_kernel.h with a list's records as FR_JIT_REC, as jit.cpp's prelude defines
them, and a static_assert per list index states the axis the pair that starts there mirrors on,
or -1.

A render cannot tell: the pair form and the list in order give the same bits (tests/test_pair_order.py),
so a predicate that silently returned -1, or one that paired the off-by-one-ulp or the
non-adjacent boxes of that test's scenes, would pass there. Also pinned here: the kind check on
both boxes, the bound on the magnitudes, flat and straddling slabs, and a chain A, B, C in which
B mirrors both neighbours (pairs are taken from the front and do not overlap)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import test_pair_order as P
from tests.test_plan import ROOT

HIPCC = "/opt/rocm/bin/hipcc"  # tools/isa_sections.py's compiler
CSRC = os.path.join(ROOT, "fo-rma_amd", "csrc")
FR_SPHERE, FR_AABB = 1, 2
F = np.float32


def _records(boxes, kinds=None):
    """64-B device records (pack.cpp pack_scene) of axis-aligned boxes [lo, hi]; kinds overrides
    the kind word of some indices."""
    out = []
    for i, g in enumerate(boxes):
        rec = list(struct.unpack("16I", struct.pack("16f", g[0], g[1], g[2], 0, g[3], g[4], g[5], 0, *([0.0] * 8))))
        rec[15] = (kinds or {}).get(i, FR_AABB)
        out.append(rec)
    return out


def _boxes(prims):
    return [[float(F(x)) for x in p["g"][:6]] for p in prims]


def _mirror(b, axis):
    lo, hi = list(b[:3]), list(b[3:])
    lo[axis], hi[axis] = -b[3 + axis], -b[axis]
    return lo + hi


A = [-1.0, 0.5, -2.0, 1.5, 2.0, 0.0]  # touches z = 0 from below
B = _mirror(A, 2)
BIG = float(F(2.0 ** 27))
CASES = {
    # scene_08: (0, 1) touch in y, (3, 4) are apart in z, 2 and 5 mirror each other with 3 and 4 between
    "scene_08": (None, [1, -1, -1, 2, -1, -1]),
    "pairs": (_boxes(P.SCENES["pairs"]), [0, -1, 2, -1, -1, -1]),
    "reversed": (_boxes(P.SCENES["reversed"]), [0, -1, 2, -1, -1, -1]),
    "ulp_off": (_boxes(P.SCENES["ulp_off"]), [-1] * 6),
    "non_adjacent": (_boxes(P.SCENES["non_adjacent"]), [-1] * 6),
    "wall_x": (_boxes(P.SCENES["wall_x"]), [0, -1, -1, -1]),
    "wall_y": (_boxes(P.SCENES["wall_y"]), [1, -1, -1, -1]),
    "wall_z": (_boxes(P.SCENES["wall_z"]), [2, -1, -1, -1]),
    # B mirrors A and C = A: (A, B) is taken, B starts no pair, C is alone; then four in a row pair twice
    "chain_abc": ([A, B, A], [2, -1, -1]),
    "chain_abab": ([A, B, A, B], [2, -1, 2, -1]),
    "single": ([A], [-1]),
    "same_box_twice": ([A, A], [-1, -1]),
    # the bound on the magnitudes (kSlabSymMax = 2^27): at it, and one ulp past it
    "at_the_bound": ([[-1.0, 0.5, -BIG, 1.5, 2.0, -1.0], [-1.0, 0.5, 1.0, 1.5, 2.0, BIG]], [2, -1]),
    "past_the_bound": ([[-1.0, 0.5, -P._up(BIG), 1.5, 2.0, -1.0], [-1.0, 0.5, 1.0, 1.5, 2.0, P._up(BIG)]], [-1, -1]),
    "flat": ([[-1.0, 0.5, 0.0, 1.5, 2.0, 0.0], [-1.0, 0.5, 0.0, 1.5, 2.0, 0.0]], [-1, -1]),
    "straddling": ([[-1.0, 0.5, -1.0, 1.5, 2.0, 2.0], [-1.0, 0.5, -2.0, 1.5, 2.0, 1.0]], [-1, -1]),
    "two_axes_mirrored": ([[1.0, 0.5, -2.0, 1.5, 2.0, 0.0], [-1.5, 0.5, 0.0, -1.0, 2.0, 2.0]], [-1, -1]),
}
# a mirrored pair of coordinates whose first or second record is not a box
KINDS = {
    "first_is_a_sphere": ([A, B], {0: FR_SPHERE}, [-1, -1]),
    "second_is_a_sphere": ([A, B], {1: FR_SPHERE}, [-1, -1]),
    "sphere_then_pair": ([A, A, B], {0: FR_SPHERE}, [-1, 2, -1]),
}


def _scene_08_records():
    import forma_rt as fr
    sc = fr.Scene.from_file(fr.scene_path("scene_08"), 64, 36)
    return _records([list(p.g[:6]) for p in sc.prims()])


def _check(tmp_path, name, recs, want):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc absent")
    assert len(recs) == len(want)
    src = f"#define FR_JIT_N {len(recs)}u\n#define FR_JIT_REC " + ",".join(
        "{" + ",".join(f"0x{w:08x}u" for w in r) + "}" for r in recs) + '\n#include "trace_kernel.h"\n'
    for i, ax in enumerate(want):
        src += f'static_assert(fr::jit_pair_axis({i}u) == {ax}, "{name}: box {i}");\n'
    path = tmp_path / f"{name}.hip"
    path.write_text(src)
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.mark.parametrize("name", sorted(CASES))
def test_pairs_of_a_list(tmp_path, fr, name):
    boxes, want = CASES[name]
    _check(tmp_path, name, _scene_08_records() if boxes is None else _records(boxes), want)


@pytest.mark.parametrize("name", sorted(KINDS))
def test_both_records_must_be_boxes(tmp_path, name):
    boxes, kinds, want = KINDS[name]
    _check(tmp_path, name, _records(boxes, kinds), want)


def test_a_wrong_expectation_fails(tmp_path):
    """The static_assert is evaluated: the chain with a pair claimed at B does not compile."""
    with pytest.raises(AssertionError, match="chain_abc_wrong: box 1"):
        _check(tmp_path, "chain_abc_wrong", _records([A, B, A]), [2, 2, -1])
