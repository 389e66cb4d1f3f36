"""Ray queries (fr_ctx_cast) without a device.

- tests/c/cast_check.cpp, a CPU program built with -fsanitize=address,undefined
  -fno-sanitize-recover=all -ffp-contract=off together with the library's scene packer and tree
  builder, walks the definition the kernels compile (fo-rma_amd/csrc/cast.h) over the tables the
  library packs: the tree walk must equal the list loop bit for bit on every ray that passes the
  fallback test, cast_ray of a pixel ray must have gb_primary_ray's bits, and a sphere's leaf
  record must carry the product sphere_root forms.
- The list loop's output must equal the oracle-based reference the GPU tests rely on
  (tests/cast_fixtures.py) on every lattice batch.
- The header and the Python mirror carry the calls as specified."""
import os
import subprocess

import numpy as np
import pytest

from tests import cast_fixtures as CF
from tests import gbuffer_ref as G
from tests import ray_edge_fixtures as X
from tests.test_plan import ROOT

F = np.float32
FR_EARG = -1


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cast") / "cast_check")
    csrc = os.path.join(ROOT, "fo-rma_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "cast_check.cpp"),
                    os.path.join(csrc, "pack.cpp"), os.path.join(csrc, "bvh.cpp"), "-o", out], check=True, timeout=600)
    return out


def _words(prims, cam, w, h, o, d):
    rays = np.zeros((len(o), 8), F)
    rays[:, 0:3], rays[:, 4:7] = o, d
    out = [np.array([len(prims), len(o), w, h], np.uint32), np.concatenate(G.cam_fields(cam)).view(np.uint32)]
    for p in prims:
        out += [np.array([p["kind"], p["material"]], np.uint32), np.asarray(p["color"], F).view(np.uint32),
                np.array([p["fuzz"]], F).view(np.uint32), np.asarray(p["g"], F).view(np.uint32)]
    return np.concatenate(out + [rays.reshape(-1).view(np.uint32)])


def run_check(exe_path, tmp_path, name, prims, cam, w, h, o, d):
    """(info dict, list-loop hit dict, [n] bool fallback) of cast_check over the rays."""
    path = str(tmp_path / f"{name}.bin")
    _words(prims, cam, w, h, o, d).tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, path], capture_output=True, text=True, timeout=600, env=env)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines and lines[0].startswith("info "), (p.returncode, p.stderr[-2000:])
    tok = lines[0].split()[1:]
    info = {k: int(v, 16) if k == "reach" else int(v) for k, v in zip(tok[0::2], tok[1::2])}
    assert p.returncode == 0, (info, p.stderr[-4000:])
    rows = np.array([[int(t, 16) for t in line.split()] for line in lines[1:]], np.uint32).reshape(len(o), 12)
    got = {"prim": rows[:, 0].copy(), "t": rows[:, 1].copy().view(F), "normal": np.ascontiguousarray(rows[:, 2:5]).view(F),
           "position": np.ascontiguousarray(rows[:, 5:8]).view(F), "albedo": np.ascontiguousarray(rows[:, 8:11]).view(F)}
    return info, got, rows[:, 11] != 0


@pytest.mark.parametrize("kind", X.KINDS)
def test_tree_equals_list_equals_oracle_on_the_lattices(check, tmp_path, fr, kind):
    b = CF.batch(fr, kind)
    ocam = X.edge_camera(fr, w=16, h=16, **X.fixture(kind, "R0_control").cam)[1]
    info, got, fb = run_check(check, tmp_path, kind, b["prims"], ocam, 16, 16, b["o"], b["d"])
    assert info["mismatch"] == 0 and info["pixel_ray"] == 0 and info["rr"] == 0
    # the 54-plane lattice exceeds kBvhMaxPlanes: no tree; every other big lattice has one
    assert info["tree"] == (0 if kind == "plane" else 1)
    assert CF.same(got, CF.expected(fr, kind)) == []
    # the program's fallback test is the restated one, with the reach the library derives
    reach = float(np.array([info["reach"]], np.uint32).view(F)[0])
    lo, hi = CF.reach_bounds(b["prims"])
    assert lo <= reach <= hi
    want = CF.falls_back(b["prims"], b["o"], b["d"])
    assert np.array_equal(fb, want) and info["fallback"] == int(want.sum())
    # the specials fall back; so do the still cameras' rays (d = 0), and nothing else
    assert want[b["special"]].all()
    others = want & ~np.isin(np.arange(len(want)), b["special"])
    assert (b["d"][others] == 0).all() and all(str(x).startswith("family:R5_") for x in b["label"][others])
    if info["tree"]:
        assert info["steps"] > 0


@pytest.mark.parametrize("count,w,h", [(200, 24, 16), (2000, 24, 16), (10000, 24, 16)])
def test_tree_equals_list_on_the_generator_spheres(check, tmp_path, fr, count, w, h):
    prims, o, d, want = CF.gen_batch(fr, count, w, h)
    ocam = CF.gen_spheres(fr, count, w, h)[2]
    info, got, fb = run_check(check, tmp_path, f"gen{count}", prims, ocam, w, h, o, d)
    assert info["tree"] == 1 and info["mismatch"] == 0 and info["pixel_ray"] == 0 and info["rr"] == 0
    assert not fb.any() and len(o) > w * h  # bounce rays are in, and every ray walks the tree
    assert CF.same(got, want) == []
    if count >= 2000:
        assert info["levels"] >= 8  # a deep tree: the traversal stack is exercised


def test_an_empty_scene_misses(check, tmp_path, fr):
    b = CF.batch(fr, "box")
    ocam = X.edge_camera(fr, w=4, h=4, **X.fixture("box", "R0_control").cam)[1]
    info, got, _ = run_check(check, tmp_path, "empty", [], ocam, 4, 4, b["o"][:70], b["d"][:70])
    assert info["tree"] == 0 and (got["prim"] == CF.MISS).all() and (got["t"] == 0).all() and (got["albedo"] == 1).all()


def test_header_and_python_mirror(fr):
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    for decl in (
            "typedef struct fr_ray { float o[3]; float pad0; float d[3]; float pad1; } fr_ray;",
            "typedef struct fr_cast_info { uint32_t n, tree, waves_tree, waves_list; } fr_cast_info;",
            "#define FR_CAST_LIST        1u", "#define FR_CAST_RAYS_DEVICE 2u",
            "int fr_camera_pixel_ray(const fr_camera* cam, uint32_t x, uint32_t y, uint32_t W, uint32_t H, fr_ray* out);",
            "int fr_ctx_cast(fr_ctx* ctx, fr_scene* scene, const fr_ray* rays, uint32_t n, uint32_t flags);",
            "int fr_ctx_download_hits(fr_ctx* ctx, uint32_t* prim, float* t, float* normal, float* position, float* albedo);",
            "int fr_ctx_cast_info(fr_ctx* ctx, fr_cast_info* out);", "int fr_ctx_gbuffer_info(fr_ctx* ctx, int* tree);",
            "#define FR_ABI_VERSION 6"):
        assert decl in hdr, decl
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fr_camera_pixel_ray", "fr_ctx_cast", "fr_ctx_download_hits", "fr_ctx_cast_info", "fr_ctx_gbuffer_info"):
        assert name in fr.EXPORTS and hasattr(fr.lib(), name) and name in integ, name
    import ctypes as C
    assert C.sizeof(fr.FrRay) == 32 and C.sizeof(fr.FrCastInfo) == 16
    assert (fr.FR_CAST_LIST, fr.FR_CAST_RAYS_DEVICE) == (1, 2)
    for name in ("cast", "cast_info", "gbuffer_info", "pick", "download_hits"):
        assert callable(getattr(fr.RenderContext, name))
    assert callable(fr.pixel_ray)
    L = fr.lib()
    assert L.fr_ctx_cast(None, None, None, 1, 0) == FR_EARG
    assert L.fr_ctx_download_hits(None, None, None, None, None, None) == FR_EARG
    assert L.fr_ctx_cast_info(None, None) == FR_EARG and L.fr_ctx_gbuffer_info(None, None) == FR_EARG


@pytest.mark.parametrize("name", ["builtin0", "lattice_mixed", "axis_neg0", "huge_t"])
def test_pixel_ray_is_the_gbuffer_ray(fr, name):
    """fr_camera_pixel_ray needs no device: o and d of every pixel are gbuffer_ref.primary_rays'."""
    _, cam, ocam, w, h, _ = G.case(fr, name)
    pos, d = G.primary_rays(ocam, w, h)
    for y in range(h):
        for x in range(w):
            o1, d1 = fr.pixel_ray(cam, x, y, w, h)
            assert np.array_equal(o1.view(np.uint32), pos.view(np.uint32))
            assert np.array_equal(d1.view(np.uint32), d[y, x].view(np.uint32)), (x, y)
    r = fr.FrRay()
    import ctypes as C
    for bad in ((w, 0, w, h), (0, h, w, h), (0, 0, 0, h), (0, 0, w, 0)):
        assert fr.lib().fr_camera_pixel_ray(C.byref(cam), *bad, C.byref(r)) == FR_EARG
    assert fr.lib().fr_camera_pixel_ray(None, 0, 0, w, h, C.byref(r)) == FR_EARG
    assert fr.lib().fr_camera_pixel_ray(C.byref(cam), 0, 0, w, h, None) == FR_EARG
