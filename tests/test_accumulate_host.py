"""Progressive accumulation (FR_FLAG_ACCUMULATE) without a device.

The flag never enters the frame plan: an accumulating frame is planned, traced and cached as
the plain frame (tests/c/plan_check.cpp prints the plan). The continue / restart / overflow
decision (fo-rma_amd/csrc/plan.cpp: accum_step) is pure; tests/c/accum_check.cpp walks it
through one context's history as a CPU program built with -fsanitize=address,undefined
-fno-sanitize-recover=all, like plan_check."""
import os
import subprocess

import pytest

from tests.test_plan import HEADLINE, MIXED, ROOT, SMALL, SPHERES_10K, _plan, _run, exe  # noqa: F401 (exe: fixture)

FR_EARG = -1
ACCUMULATE, SCENE_JIT, WRITE_U8, MT_BANDS = 32, 4, 1, 2


@pytest.mark.parametrize("case", ["headline", "small_spp3", "mixed", "bvh", "shard", "streamed"])
def test_the_flag_never_reaches_the_plan(exe, case):
    kv = {"headline": HEADLINE, "small_spp3": dict(SMALL, spp=3), "mixed": MIXED, "bvh": SPHERES_10K,
          "shard": dict(HEADLINE, shard="0/8"), "streamed": dict(HEADLINE, prev_in_flight=1)}[case]
    for base in (0, SCENE_JIT, WRITE_U8 | SCENE_JIT):
        plain = _plan(exe, **dict(kv, flags=base))
        acc = _plan(exe, **dict(kv, flags=base | ACCUMULATE))
        assert plain["rc"] == 0 and acc == plain, base  # every printed field, kp.flags and the kernel included
        assert acc["flags"] & ACCUMULATE == 0


def test_the_flag_with_mt_bands_is_refused_with_the_parameters(exe):
    r = _plan(exe, **dict(MIXED, depth=8, flags=ACCUMULATE | MT_BANDS))
    assert r["rc"] == FR_EARG and "FR_FLAG_ACCUMULATE with FR_FLAG_MT_BANDS" in r["error"]
    assert _plan(exe, **dict(MIXED, depth=8, flags=MT_BANDS))["rc"] == 0


@pytest.fixture(scope="module")
def history(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("accum") / "accum_check")
    srcs = [os.path.join(ROOT, "tests", "c", "accum_check.cpp")] + [
        os.path.join(ROOT, "fo-rma_amd", "csrc", f)
        for f in ("plan.cpp", "pack.cpp", "json_min.cpp", "scene.cpp", "bvh.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), *srcs, "-o", out], check=True, timeout=600)
    return _run(out)  # asserts exit status 0 (every internal check held) and a clean sanitizer log


def test_continue_restart_and_overflow(history):
    got = [(r["case"], r["rc"], r.get("start"), r.get("frames"), r.get("samples")) for r in history
           if not r["case"].startswith("mt_bands")]
    top = 2 ** 32 - 1
    assert got == [
        ("first", 0, 1, 1, 4),
        ("continue", 0, 0, 2, 8),  # another seed
        ("continue_other_flags", 0, 0, 3, 12),
        ("mixed_spp", 0, 0, 4, 13), ("mixed_spp", 0, 0, 5, 29), ("mixed_spp", 0, 0, 6, 31),
        ("scene_upload", 0, 1, 1, 4), ("continue", 0, 0, 2, 8),
        ("camera_orbit", 0, 1, 1, 4), ("continue", 0, 0, 2, 8),
        ("camera_last_field_bit", 0, 1, 1, 4),
        ("camera_first_field", 0, 1, 1, 4),
        ("width", 0, 1, 1, 4), ("height", 0, 1, 1, 4), ("max_depth", 0, 1, 1, 4),
        ("shard_count", 0, 1, 1, 4), ("shard_index", 0, 1, 1, 4), ("continue", 0, 0, 2, 8),
        ("reset", 0, 1, 1, 4),
        ("fill_to_limit", 0, 0, 2, top),  # n = 2^32 - 1 is reachable
        ("overflow", FR_EARG, None, 2, top),  # one more sample is not, and the state stays
        ("zero_spp_at_limit", 0, 0, 3, top),
        ("restart_at_limit", 0, 1, 1, 1),  # a restart counts from its own spp
    ]
    (err,) = [r["error"] for r in history if r["case"] == "overflow"]
    assert "4294967295 samples per pixel cannot take 1 more" in err


def test_mt_bands_check(history):
    by = {r["case"]: r for r in history}
    assert by["mt_bands"]["rc"] == FR_EARG and "save_image_mt has its own averaging" in by["mt_bands"]["error"]
    assert by["mt_bands_plain"]["rc"] == 0


def test_python_mirror_carries_the_flag(fr):
    assert fr.FR_FLAG_ACCUMULATE == ACCUMULATE
    assert fr.make_params(8, 8, 1).flags & ACCUMULATE == 0
    p = fr.make_params(8, 8, 1, accumulate=True, scene_jit="wait")
    assert p.flags == WRITE_U8 | SCENE_JIT | 8 | ACCUMULATE
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    assert "#define FR_FLAG_ACCUMULATE 32u" in hdr


def test_one_shot_renders_refuse_the_flag_before_they_touch_a_device(fr):
    import ctypes as C
    sc = fr.Scene.builtin(0, 8, 8)
    p = fr.make_params(8, 8, 1, accumulate=True)
    for call in (lambda: fr.lib().fr_render_hip(sc._h, C.byref(sc.camera), C.byref(p), 0, None, None, None),
                 lambda: fr.lib().fr_render_hip_multi(sc._h, C.byref(sc.camera), C.byref(p), 1, None, None, None)):
        assert call() == FR_EARG
        assert b"FR_FLAG_ACCUMULATE" in fr.lib().fr_last_error()
    for name in ("fr_ctx_accum_reset", "fr_mctx_accum_reset"):  # null handles
        assert getattr(fr.lib(), name)(None) == FR_EARG
    for name in ("fr_ctx_accum_info", "fr_mctx_accum_info"):
        assert getattr(fr.lib(), name)(None, None, None) == FR_EARG
