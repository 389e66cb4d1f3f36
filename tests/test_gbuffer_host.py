"""The first-hit feature buffers (fr_ctx_gbuffer) without a device.

- tests/c/gbuffer_check.cpp, a CPU program built with -fsanitize=address,undefined
  -fno-sanitize-recover=all -ffp-contract=off together with the library's scene packer, runs the
  arithmetic the kernel compiles (fo-rma_amd/csrc/gbuffer.h) over the records the library packs;
  the oracle-based reference the GPU tests rely on (tests/gbuffer_ref.py) must equal its bits on
  every case the GPU tests use.
- The cases really contain what they are chosen for, asserted here on the oracle alone: hit and
  miss pixels, winners followed by a plane that passes its denominator test and fails its
  bounds (the shared record's t is stale there), exact zero direction components, roots past
  2^40, a list past the BVH threshold.
- The header and the Python mirror carry the calls as specified."""
import os
import subprocess

import numpy as np
import pytest

from oracle import scene_ref as S
from tests import gbuffer_ref as G
from tests.test_plan import ROOT

F = np.float32
FR_EARG = -1


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gbuffer") / "gbuffer_check")
    csrc = os.path.join(ROOT, "fo-rma_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "gbuffer_check.cpp"),
                    os.path.join(csrc, "pack.cpp"), os.path.join(csrc, "bvh.cpp"), "-o", out], check=True, timeout=600)
    return out


def _words(prims, cam, w, h):
    out = [np.array([w, h, len(prims)], np.uint32), np.concatenate(G.cam_fields(cam)).view(np.uint32)]
    for p in prims:
        out += [np.array([p["kind"], p["material"]], np.uint32), np.asarray(p["color"], F).view(np.uint32),
                np.array([p["fuzz"]], F).view(np.uint32), np.asarray(p["g"], F).view(np.uint32)]
    return np.concatenate(out)


def header_gbuffer(exe_path, tmp_path, name, prims, cam, w, h):
    """gbuffer.h on the CPU over pack.cpp's records: a G-buffer dict as gbuffer_ref returns it."""
    path = str(tmp_path / f"{name}.bin")
    _words(prims, cam, w, h).tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, path], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    rows = np.array([[int(t, 16) for t in line.split()] for line in p.stdout.splitlines()], np.uint32)
    assert rows.shape == (w * h, 11)
    return {"prim": rows[:, 0].reshape(h, w), "depth": rows[:, 1].reshape(h, w).view(F),
            "normal": np.ascontiguousarray(rows[:, 2:5]).reshape(h, w, 3).view(F),
            "position": np.ascontiguousarray(rows[:, 5:8]).reshape(h, w, 3).view(F),
            "albedo": np.ascontiguousarray(rows[:, 8:11]).reshape(h, w, 3).view(F)}


@pytest.mark.parametrize("name", list(G.CASES))
def test_header_bits_equal_the_oracle_reference(check, tmp_path, fr, name):
    prims, cam, ocam, w, h, _ = G.case(fr, name)
    # the product's camera is the oracle's in the fields the ray reads
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(G.cam_fields(cam), G.cam_fields(ocam)))
    want = G.expected(fr, name)
    got = header_gbuffer(check, tmp_path, name, prims, ocam, w, h)
    assert G.same(got, want) == []
    miss = want["prim"] == G.MISS
    assert (want["depth"][miss] == 0).all() and (want["normal"][miss] == 0).all() and (want["albedo"][miss] == 1).all()
    assert (want["prim"][~miss] < len(prims)).all()


def test_an_empty_scene_misses_everywhere(check, tmp_path, fr):
    _, _, ocam, w, h, _ = G.case(fr, "builtin0")
    got = header_gbuffer(check, tmp_path, "empty", [], ocam, 5, 3)
    assert (got["prim"] == G.MISS).all() and (got["depth"] == 0).all() and (got["albedo"] == 1).all()


def test_the_cases_contain_what_they_are_chosen_for(fr):
    want = {name: G.expected(fr, name) for name in G.CASES}
    for name in ("builtin0", "lattice_mixed", "spheres200"):  # hit and miss pixels
        miss = want[name]["prim"] == G.MISS
        assert miss.any() and (~miss).any(), name
    # winners followed by a failing plane: the shared record's t is not the winner's
    for name in ("lattice_plane", "lattice_mixed"):
        assert want[name]["stale"].any() and not want[name]["stale"].all(), name
    # every primitive kind wins somewhere in its lattice; the mixed one has stubs, which never do
    kinds = {"lattice_box": S.AABB, "lattice_sphere": S.SPHERE, "lattice_obb": S.OBB, "lattice_tri": S.TRIANGLE,
             "lattice_plane": S.PLANE}
    for name, kind in kinds.items():
        prims = G.case(fr, name)[0]
        won = {prims[i]["kind"] for i in np.unique(want[name]["prim"]) if i != G.MISS}
        assert kind in won, name
    prims = G.case(fr, "lattice_mixed")[0]
    won = {prims[i]["kind"] for i in np.unique(want["lattice_mixed"]["prim"]) if i != G.MISS}
    assert len(won) >= 4 and S.STUB in {p["kind"] for p in prims} and S.STUB not in won
    # light-class winners read albedo 1, whatever their colour
    for name in ("lattice_sphere", "lattice_tri"):
        prims = G.case(fr, name)[0]
        light = [i for i, p in enumerate(prims) if p["material"] == S.LIGHT]
        sel = np.isin(want[name]["prim"], light)
        assert sel.any() and (want[name]["albedo"][sel] == 1).all() and all((prims[i]["color"] != 1).any() for i in light)
    # exact zero direction components, of both signs
    for name, neg in (("axis_neg0", True), ("axis_face", False)):
        _, _, ocam, w, h, _ = G.case(fr, name)
        dx = G.primary_rays(ocam, w, h)[1][..., 0]
        assert (dx == 0).all() and bool(np.signbit(dx).all()) == neg, name
    assert float(want["huge_t"]["depth"].max()) > 2.0 ** 40
    assert len(G.case(fr, "spheres200")[0]) >= 200  # past the 48-primitive BVH threshold


def test_header_and_python_mirror(fr):
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    assert "int fr_ctx_gbuffer(fr_ctx* ctx, fr_scene* scene, const fr_camera* cam, uint32_t width, uint32_t height);" in hdr
    assert "int fr_ctx_download_gbuffer(fr_ctx* ctx, uint32_t* prim, float* depth, float* normal, float* position," in hdr
    assert "#define FR_ABI_VERSION 6" in hdr and "#define FR_GBUFFER_MISS 0xFFFFFFFFu" in hdr
    for name in ("fr_ctx_gbuffer", "fr_ctx_download_gbuffer"):
        assert name in fr.EXPORTS and hasattr(fr.lib(), name)
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert fr.FR_GBUFFER_MISS == G.MISS == 0xFFFFFFFF
    for name in ("gbuffer", "download_gbuffer"):
        assert callable(getattr(fr.RenderContext, name))
    assert fr.lib().fr_ctx_gbuffer(None, None, None, 1, 1) == FR_EARG
    assert fr.lib().fr_ctx_download_gbuffer(None, None, None, None, None, None) == FR_EARG
