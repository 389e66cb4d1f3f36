"""Occlusion queries and ranged casts (fr_ctx_occluded, FR_CAST_TMAX) without a device.

- tests/c/occlude_check.cpp, a CPU program built with -fsanitize=address,undefined
  -fno-sanitize-recover=all -ffp-contract=off together with the library's scene packer and tree
  builder, walks the definitions the kernels compile (fo-rma_amd/csrc/cast.h) over the tables the
  library packs: on every ray that passes the fallback test the ranged tree walk must equal the
  ranged list loop (winner and root bits) and the any-hit tree walk the any-hit list, and on
  every ray the any-hit list must equal "the ranged list loop found a winner".
- Its list results must equal the oracle-based reference the GPU tests rely on
  (tests/occlude_fixtures.py) on every lattice batch and on the generator's spheres.
- The header and the Python mirror carry the calls as specified."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cast_fixtures as CF
from tests import occlude_fixtures as OF
from tests import ray_edge_fixtures as X
from tests.test_plan import ROOT

F = np.float32
FR_EARG = -1


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("occlude") / "occlude_check")
    csrc = os.path.join(ROOT, "fo-rma_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "occlude_check.cpp"),
                    os.path.join(csrc, "pack.cpp"), os.path.join(csrc, "bvh.cpp"), "-o", out], check=True, timeout=600)
    return out


def _words(prims, o, d, t_max):
    rays = np.zeros((len(o), 8), F)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, t_max
    out = [np.array([len(prims), len(o)], np.uint32)]
    for p in prims:
        out += [np.array([p["kind"], p["material"]], np.uint32), np.asarray(p["color"], F).view(np.uint32),
                np.array([p["fuzz"]], F).view(np.uint32), np.asarray(p["g"], F).view(np.uint32)]
    return np.concatenate(out + [rays.reshape(-1).view(np.uint32)])


def run_check(exe_path, tmp_path, name, prims, o, d, t_max):
    """(info dict, ranged list-loop hit dict with "occluded", [n] bool fallback) of occlude_check."""
    path = str(tmp_path / f"{name}.bin")
    _words(prims, o, d, t_max).tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, path], capture_output=True, text=True, timeout=600, env=env)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines and lines[0].startswith("info "), (p.returncode, p.stderr[-2000:])
    tok = lines[0].split()[1:]
    info = {k: int(v) for k, v in zip(tok[0::2], tok[1::2])}
    assert p.returncode == 0, (info, p.stderr[-4000:])
    rows = np.array([[int(t, 16) for t in line.split()] for line in lines[1:]], np.uint32).reshape(len(o), 13)
    got = {"prim": rows[:, 0].copy(), "t": rows[:, 1].copy().view(F), "normal": np.ascontiguousarray(rows[:, 2:5]).view(F),
           "position": np.ascontiguousarray(rows[:, 5:8]).view(F), "albedo": np.ascontiguousarray(rows[:, 8:11]).view(F),
           "occluded": rows[:, 12] != 0}
    return info, got, rows[:, 11] != 0


def _agrees(info, got, want):
    assert info["ranged"] == 0 and info["anyhit"] == 0 and info["equiv"] == 0
    assert CF.same(got, want) == []
    assert np.array_equal(got["occluded"], want["occluded"])


@pytest.mark.parametrize("kind", X.KINDS)
def test_walks_agree_and_equal_the_reference_on_the_lattices(check, tmp_path, fr, kind):
    b, t_max, want = OF.lattice(fr, kind)
    info, got, fb = run_check(check, tmp_path, kind, b["prims"], b["o"], b["d"], t_max)
    _agrees(info, got, want)
    assert info["tree"] == (0 if kind == "plane" else 1)
    assert np.array_equal(fb, CF.falls_back(b["prims"], b["o"], b["d"])) and info["fallback"] == int(fb.sum())
    if info["tree"]:
        # the any-hit walk stops early and culls at t_max: never more node steps than the ranged walk
        assert 0 < info["osteps"] <= info["steps"]


@pytest.mark.parametrize("count", [200, 2000, 10000])
def test_walks_agree_and_equal_the_reference_on_the_generator_spheres(check, tmp_path, fr, count):
    prims, o, d, t_max, want = OF.spheres(fr, count)
    info, got, fb = run_check(check, tmp_path, f"gen{count}", prims, o, d, t_max)
    _agrees(info, got, want)
    assert info["tree"] == 1 and not fb.any() and 0 < info["osteps"] <= info["steps"]
    assert want["occluded"].any() and not want["occluded"].all()


def test_an_unbounded_range_is_the_cast(check, tmp_path, fr):
    """t_max = FLT_MAX on every ray: the ranged loop is fr_ctx_cast's, and a ray is occluded iff it hits."""
    b, want = CF.batch(fr, "mixed"), CF.expected(fr, "mixed")
    info, got, _ = run_check(check, tmp_path, "unbounded", b["prims"], b["o"], b["d"], np.full(len(b["o"]), OF.FLT_MAX, F))
    assert info["ranged"] == 0 and info["anyhit"] == 0 and info["equiv"] == 0
    assert CF.same(got, want) == [] and np.array_equal(got["occluded"], want["prim"] != CF.MISS)


def test_an_empty_scene_occludes_nothing(check, tmp_path, fr):
    b = CF.batch(fr, "box")
    info, got, _ = run_check(check, tmp_path, "empty", [], b["o"][:70], b["d"][:70], np.full(70, OF.FLT_MAX, F))
    assert info["tree"] == 0 and not got["occluded"].any() and (got["prim"] == CF.MISS).all()


def test_header_and_python_mirror(fr):
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    for decl in (
            "#define FR_CAST_TMAX 16u", "#define FR_CAST_OUT_DEVICE 8u",
            "typedef struct fr_occl_info { uint32_t n, tree, waves_tree, waves_list, occluded, pad[3]; } fr_occl_info;",
            "int fr_ctx_occluded(fr_ctx* ctx, fr_scene* scene, const fr_ray* rays, uint32_t n, uint32_t flags, uint8_t* out);",
            "int fr_ctx_download_occluded(fr_ctx* ctx, uint8_t* host);",
            "int fr_ctx_occluded_info(fr_ctx* ctx, fr_occl_info* out);",
            "int fr_ctx_hit_buffers(fr_ctx* ctx, void** g0, void** g1, void** alb, uint32_t* n);",
            "int fr_ctx_cast(fr_ctx* ctx, fr_scene* scene, const fr_ray* rays, uint32_t n, uint32_t flags);",
            "#define FR_ABI_VERSION 6"):
        assert decl in hdr, decl
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fr_ctx_occluded", "fr_ctx_download_occluded", "fr_ctx_occluded_info", "fr_ctx_hit_buffers"):
        assert name in fr.EXPORTS and hasattr(fr.lib(), name) and name in integ, name
    assert "FR_CAST_TMAX" in integ and "FR_CAST_OUT_DEVICE" in integ and "fr_occl_info" in integ
    assert C.sizeof(fr.FrOcclInfo) == 32 and C.sizeof(fr.FrRay) == 32
    assert (fr.FR_CAST_LIST, fr.FR_CAST_RAYS_DEVICE, fr.FR_CAST_TMAX, fr.FR_CAST_OUT_DEVICE) == (1, 2, 16, 8)
    assert fr.FR_ABI_VERSION == 6 and fr.lib().fr_abi_version() == 6
    for name in ("occluded", "visible", "occluded_info", "download_occluded", "hit_buffers", "cast"):
        assert callable(getattr(fr.RenderContext, name))


def test_null_arguments_are_refused_without_a_device(fr):
    L = fr.lib()
    rays = np.zeros((4, 8), F)
    rp = rays.ctypes.data_as(C.c_void_p)
    assert L.fr_ctx_occluded(None, None, None, 1, 0, None) == FR_EARG
    assert L.fr_ctx_occluded(None, None, rp, 4, fr.FR_CAST_TMAX, None) == FR_EARG
    assert b"fr_ctx_occluded" in L.fr_last_error()
    assert L.fr_ctx_download_occluded(None, None) == FR_EARG
    assert L.fr_ctx_occluded_info(None, None) == FR_EARG
    i = fr.FrOcclInfo()
    assert L.fr_ctx_occluded_info(None, C.byref(i)) == FR_EARG
    assert L.fr_ctx_hit_buffers(None, None, None, None, None) == FR_EARG
