"""Adaptive sampling (FR_FLAG_ADAPTIVE) without a device.

- Every case of tests/test_adaptive.py keeps its condition on the oracle: at the first adapt of
  the flow some tiles are active and some are not (the thresholds are conditions, not measurements).
- tests/adaptive_ref.py with every tile active equals tests/accum_error_ref.py's ErrorComposite
  bit for bit.
- tests/c/adapt_check.cpp, a CPU program built like tests/c/plan_check.cpp (sanitizers on),
  prints the plan of adaptive frames and the tiled bookkeeping's decisions.
- tests/c/adapt_abi.c pins fr_adapt_info's layout from C; the ctypes mirror agrees."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import accum_error_ref as R
from tests import adaptive_ref as AR
from tests.test_plan import ROOT, _kernel, _run

F = np.float32
FR_EARG = -1
WRITE_U8, ACCUMULATE, ACCUM_ERROR, ADAPTIVE = 1, 32, 64, 128


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


@pytest.mark.parametrize("case", sorted(AR.CASES))
def test_every_gpu_case_mixes_active_and_inactive_tiles(case):
    key, w, h, depth, spp, thr, mins = AR.CASES[case]
    steps = AR.reference_flow(key, w, h, depth, spp, thr, mins)
    acts = [s["summary"] for s in steps if s["op"] == "A"]
    print(case, [(a["active_tiles"], a["tiles"]) for a in acts])
    if case == "cubes100_zero":  # threshold 0: exactly the tiles with a pixel of rel > 0
        first = next(s for s in steps if s["op"] == "A")
        tiles = {(y // 8, x // 8) for y, x in zip(*np.nonzero(first["rel"] > 0))}
        assert {(int(s), int(c)) for s, c in zip(*np.nonzero(first["mask"]))} == tiles and tiles
        return
    assert 0 < acts[0]["active_tiles"] < acts[0]["tiles"]
    if case == "cubes100_16":  # ends on the empty list: the last frame traces nothing
        assert acts[-1]["active_tiles"] == 0 and acts[-2]["active_tiles"] > 0
    # a tile that was inactive stays inactive under the same threshold
    masks = [s["mask"] for s in steps if s["op"] == "A"]
    for a, b in zip(masks, masks[1:]):
        assert not (b & ~a).any()


def test_min_samples_case():
    key, w, h, depth, spp, _, _ = AR.CASES["scene08_16"]
    steps = AR.reference_flow(key, w, h, depth, spp, AR.INF, 48)
    assert [s["summary"]["active_tiles"] for s in steps if s["op"] == "A"] == [15, 0, 0]


def test_every_tile_active_equals_the_uniform_composite():
    key, w, h, depth = "scene_08", 33, 17, 8
    from tests.test_accumulate import _frame_sum, _oracle_frame
    uni, ada = R.ErrorComposite(), AR.AdaptiveComposite(w, h)
    for k, spp in enumerate((16, 4, 16, 2)):
        omean, _, _, _ = _oracle_frame(key, w, h, spp, depth, AR.SEED0 + k)
        s = _frame_sum(omean, spp)
        m1 = uni.add(s, spp)
        m2 = ada.add(s, spp, np.ones(ada.shape, bool) if k else None)
        assert np.array_equal(_bits(m1), _bits(m2))
        assert np.array_equal(_bits(uni.a), _bits(ada.a)) and np.array_equal(_bits(uni.q), _bits(ada.q))
        if k:
            assert np.array_equal(_bits(uni.rel()), _bits(ada.rel()))
            for thr in (0.0, 2.0 ** -3, AR.INF):
                want = uni.summary(thr)
                mask, got = ada.select(thr)
                for name in ("frames", "samples", "pixels", "converged"):
                    assert got[name] == want[name]
                assert _bits(got["max_rel"]) == _bits(want["max_rel"])
                assert got["active_pixels"] == int(ada.pixels(mask).sum())
    assert (ada.n == 38).all() and (ada.k == 4).all()


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adapt") / "adapt_check")
    srcs = [os.path.join(ROOT, "tests", "c", "adapt_check.cpp")] + [
        os.path.join(ROOT, "fo-rma_amd", "csrc", f)
        for f in ("plan.cpp", "pack.cpp", "json_min.cpp", "scene.cpp", "bvh.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), *srcs, "-o", out], check=True, timeout=600)
    return out


def _plans(check, tiles, w, h, spp):
    plain, ada = _run(check, "plan", str(tiles), str(w), str(h), str(spp))
    assert plain["plan"] == "plain" and ada["plan"] == "adaptive"
    return plain, ada


def test_adaptive_plan_of_seven_tiles(check):
    plain, ada = _plans(check, 7, 33, 17, 16)
    assert (plain["n_tiles"], plain["P"]) == (15, 960) and plain["pass"] == [[0, 1, 960, 960, 0]]
    assert (ada["n_tiles"], ada["P"], ada["magic_ok"]) == (7, 448, 1)
    assert ada["pass"] == [[0, 1, 448, 448, 0]]
    assert ada["per_block"] == 448 * 16 * 2 * 4 and ada["running_bytes"] == 448 * 12
    # the flag never reaches the kernel's flags, and the kernel is the plain frame's
    assert ada["flags"] == plain["flags"] and ada["flags"] & (ACCUMULATE | ACCUM_ERROR | ADAPTIVE) == 0
    assert ada["kernel"] == plain["kernel"] == _kernel(1, 0, 9, 8, 0, 0, 2, 1)
    assert ada["tiles_per_row"] == 5 and ada["list"] == 0  # (the list's pointer is the driver's to set)


def test_adaptive_plan_of_one_tile_and_of_none(check):
    _, one = _plans(check, 1, 33, 17, 16)
    assert (one["n_tiles"], one["P"], one["magic_ok"]) == (1, 64, 1) and one["pass"] == [[0, 1, 64, 64, 0]]
    _, none = _plans(check, 0, 33, 17, 16)
    assert (none["n_tiles"], none["P"], none["passes"], none["pass"]) == (0, 0, 0, [])
    assert none["slot_bytes"] == 0 and none["nblocks"] == 0
    _, capped = _plans(check, 99, 33, 17, 16)  # never more than the shard's tiles
    assert capped["n_tiles"] == 15


def test_adaptive_plan_fine_items_over_a_compact_p(check):
    plain, ada = _plans(check, 7, 33, 17, 32)
    # block 0 whole (P items), block 1 as four sub-blocks of 4 samples: n_coarse = P, 5 P items
    assert plain["pass"] == [[0, 2, 5 * 960, 960, 1]]
    assert ada["pass"] == [[0, 2, 5 * 448, 448, 1]]
    _, short = _plans(check, 7, 33, 17, 20)  # a last block of 4 samples: one sub-block
    assert short["pass"] == [[0, 2, 2 * 448, 448, 1]]


def test_tiled_bookkeeping(check):
    got = {r["case"]: r for r in _run(check, "decision")}
    assert got["adaptive_first"]["rc"] == FR_EARG and "would start a new accumulation" in got["adaptive_first"]["error"]
    assert (got["plain_2"]["frames"], got["plain_2"]["samples"], got["plain_2"]["tiled"]) == (2, 32, 0)
    assert got["adaptive_untiled"]["rc"] == FR_EARG and "no tile list" in got["adaptive_untiled"]["error"]
    assert (got["adaptive_untiled"]["frames"], got["adaptive_untiled"]["samples"]) == (2, 32)
    a7 = got["adaptive_7"]
    assert (a7["rc"], a7["empty"], a7["start"], a7["frames"], a7["samples"], a7["tiled"]) == (0, 0, 0, 3, 48, 1)
    pt = got["plain_in_tiled"]
    assert (pt["start"], pt["frames"], pt["samples"], pt["tiled"]) == (0, 4, 52, 1)
    e = got["adaptive_empty"]
    assert (e["rc"], e["empty"], e["frames"], e["samples"], e["tiled"]) == (0, 1, 4, 52, 1)
    m = got["adaptive_moved"]
    assert m["rc"] == FR_EARG and (m["frames"], m["samples"]) == (4, 52)
    r = got["plain_moved"]
    assert (r["start"], r["frames"], r["samples"], r["tiled"]) == (1, 1, 16, 0)  # the list died with the accumulation
    assert got["adaptive_after_restart"]["rc"] == FR_EARG and "no tile list" in got["adaptive_after_restart"]["error"]
    assert got["adaptive_overflow"]["rc"] == FR_EARG and "32-bit count" in got["adaptive_overflow"]["error"]
    for f in (ADAPTIVE, ADAPTIVE | ACCUMULATE):
        assert got[f"flags_{f}"]["rc"] == FR_EARG and "FR_FLAG_ADAPTIVE needs" in got[f"flags_{f}"]["error"]
    assert got[f"flags_{ADAPTIVE | ACCUMULATE | ACCUM_ERROR}"]["rc"] == 0


def test_struct_layout_from_c(tmp_path, fr):
    import ctypes as C
    exe_path = str(tmp_path / "adapt_abi")
    libdir = os.path.join(ROOT, "fo-rma_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "adapt_abi.c"), "-L", libdir, "-lforma_rt",
                    f"-Wl,-rpath,{libdir}", "-o", exe_path], check=True)
    lay = json.loads(subprocess.run([exe_path], check=True, capture_output=True, text=True).stdout)
    assert lay["sizeof"] == 56 == C.sizeof(fr.FrAdaptInfo)
    want = {"frames": [0, 4], "samples": [4, 4], "tiles": [8, 4], "active_tiles": [12, 4], "pixels": [16, 8],
            "active_pixels": [24, 8], "converged": [32, 8], "max_rel": [40, 4], "threshold": [44, 4],
            "min_samples": [48, 4], "pad": [52, 4]}
    for name, (off, size) in want.items():
        assert lay[name] == [off, size], name
        field = getattr(fr.FrAdaptInfo, name)
        assert (field.offset, field.size) == (off, size), name
    assert [f for f, _ in fr.FrAdaptInfo._fields_] == list(want)
    assert lay["flag"] == 128 and lay["abi_version"] == 6
    assert lay["null_rc"] == [FR_EARG] * 3


def test_python_mirror(fr):
    assert fr.FR_FLAG_ADAPTIVE == ADAPTIVE and fr.FR_ABI_VERSION == 6
    assert fr.make_params(8, 8, 1, accumulate="error").flags & ADAPTIVE == 0
    p = fr.make_params(8, 8, 1, accumulate="adaptive")
    assert p.flags == WRITE_U8 | ACCUMULATE | ACCUM_ERROR | ADAPTIVE
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    assert "#define FR_FLAG_ADAPTIVE 128u" in hdr and "#define FR_ABI_VERSION 6" in hdr
    for name in ("fr_ctx_adapt", "fr_ctx_download_counts", "fr_mctx_adapt"):
        assert name in fr.EXPORTS and hasattr(fr.lib(), name)
    assert callable(fr.RenderContext.adapt) and callable(fr.RenderContext.download_counts)
    assert callable(fr.MultiContext.adapt)
    import inspect
    sig = inspect.signature(fr.render_converged)
    assert sig.parameters["adaptive"].default is False and sig.parameters["min_samples"].default == 0
