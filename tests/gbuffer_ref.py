"""The first-hit feature buffers (fr_ctx_gbuffer) from the oracle: a numpy-f32 primary ray per
pixel, the oracle's closest-hit loop for the winner, its normal and its own root, and the point
and the albedo restated in numpy (tests/test_gbuffer_host.py holds this against the bits of the
header the kernel compiles). Shared by the host and the GPU tests; not a test module."""
import ctypes as C

import numpy as np

from oracle import oracle_py as O
from oracle import scene_ref as S

F = np.float32
MISS = 0xFFFFFFFF


def cam_fields(cam):
    """position, lower_left, horizontal, vertical of an FrCamera or OrCamera as f32 [3] arrays."""
    return tuple(np.array(list(getattr(cam, n)), dtype=F) for n in ("position", "lower_left", "horizontal", "vertical"))


def primary_rays(cam, w, h):
    """(o [3], d [H, W, 3]): get_ray with the jitter fixed at 0.5 and no lens offset,
    u = ((float)x + 0.5) / W, v = ((float)(H - y) + 0.5) / H, d = ((ll + u hor) + v ver) - pos."""
    pos, ll, hor, ver = cam_fields(cam)
    with np.errstate(all="ignore"):
        u = ((np.arange(w, dtype=np.uint32).astype(F) + F(0.5)).astype(F) / F(w)).astype(F)
        v = (((np.uint32(h) - np.arange(h, dtype=np.uint32)).astype(F) + F(0.5)).astype(F) / F(h)).astype(F)
        a = (ll[None, None, :] + (u[None, :, None] * hor[None, None, :]).astype(F)).astype(F)
        b = (a + (v[:, None, None] * ver[None, None, :]).astype(F)).astype(F)
        d = (b - pos[None, None, :]).astype(F)
    return pos, d


def albedo_of(p):
    """pack.cpp's attenuation: the colour, or 1 for the light class (scatter_class: a plane is
    metal or lambertian whatever its material says, a stub has no class; the others are light
    for material 3)."""
    kind = p["kind"] if p["kind"] <= S.TRIANGLE else S.STUB
    light = kind not in (S.PLANE, S.STUB) and p["material"] == S.LIGHT
    return np.ones(3, F) if light else np.asarray(p["color"], F)


def gbuffer(prims, cam, w, h):
    """{"prim" [H, W] u32, "depth" [H, W], "normal", "position", "albedo" [H, W, 3] f32, and "stale"
    [H, W] bool: the shared record's t after the whole list differs from the winner's own}."""
    o, d = primary_rays(cam, w, h)
    arr = O.prims_to_c(prims)
    hit = O.lib().oracle_closest_hit
    out = {"prim": np.full((h, w), MISS, np.uint32), "depth": np.zeros((h, w), F), "normal": np.zeros((h, w, 3), F),
           "position": np.zeros((h, w, 3), F), "albedo": np.ones((h, w, 3), F), "stale": np.zeros((h, w), bool)}
    oo = (C.c_float * 3)(*[float(x) for x in o])
    rec, own = (C.c_float * 7)(), (C.c_float * 7)()
    for y in range(h):
        for x in range(w):
            dd = (C.c_float * 3)(*[float(c) for c in d[y, x]])
            best = hit(arr, len(prims), oo, dd, rec)  # O.closest_hit(prims, o, d)
            if best < 0:
                continue
            # the list cut after the winner: the winner is the last test to write the record, so
            # a later plane's stale write cannot show in t
            assert hit(arr, best + 1, oo, dd, own) == best
            t = F(own[0])
            out["prim"][y, x] = best
            out["depth"][y, x] = t
            out["normal"][y, x] = np.array(rec[4:7], F)
            assert np.array_equal(np.array(own[4:7], F).view(np.uint32), out["normal"][y, x].view(np.uint32))
            with np.errstate(all="ignore"):
                out["position"][y, x] = (o + (t * d[y, x]).astype(F)).astype(F)
            out["albedo"][y, x] = albedo_of(prims[best])
            out["stale"][y, x] = np.float32(rec[0]).view(np.uint32) != t.view(np.uint32)
    for a in out.values():
        a.setflags(write=False)
    return out


_cache = {}


def cached(key, prims, cam, w, h):
    """gbuffer() computed once per `key` and shared, read-only."""
    if key not in _cache:
        _cache[key] = gbuffer(prims, cam, w, h)
    return _cache[key]


def same(got, want):
    """The names whose bits differ between two G-buffers (an empty list: equal)."""
    bad = []
    for name in ("prim", "depth", "normal", "position", "albedo"):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            bad.append((name, int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))) if a.shape == b.shape else -1))
    return bad


# ---- the scenes the host and the GPU tests share -----------------------------------------

def _gen_spheres():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(root, "tools", "gen_scene.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    return gs.dumps(gs.generator_scene(200, "sphere"))


# name: (source, width, height). Sizes that are no multiple of the 32 x 8 workgroup; one lattice
# per primitive kind (planes: "plane", and "mixed" with stubs); an axis-parallel fan with an
# exact -0 direction component; roots past 2^40; 200 spheres, past the 48-primitive BVH threshold.
CASES = {
    "builtin0": ("scene", 32, 24), "scene_08": ("scene", 33, 17), "scene_01": ("scene", 33, 17),
    "lattice_box": ("edge:box:R0_control", 16, 16), "lattice_sphere": ("edge:sphere:R0_control", 16, 16),
    "lattice_obb": ("edge:obb:R0_control", 16, 16), "lattice_tri": ("edge:tri:R0_control", 16, 16),
    "lattice_plane": ("edge:plane:R0_control", 16, 16), "lattice_mixed": ("edge:mixed:R0_control", 16, 16),
    "axis_neg0": ("edge:mixed:R2_neg0", 16, 16), "axis_face": ("edge:box:R1_face", 16, 16),
    "huge_t": ("magnitude:mixed:small:M7_s20_k-64", 16, 16),
    "spheres200": ("gen", 16, 9),
}


def case(fr, name):
    """(oracle prims, FrCamera, OrCamera, w, h, product Scene) of one of CASES."""
    from tests import magnitude_fixtures as M
    from tests import ray_edge_fixtures as X
    from tests.test_accumulate import _oracle_scene, _product_scene
    src, w, h = CASES[name]
    if src == "scene":
        prims, ocam = _oracle_scene(name, w, h)
        sc = _product_scene(fr, name, w, h)
        return prims, sc.camera, ocam, w, h, sc
    if src == "gen":
        text = _gen_spheres()
        prims, (frm, at, vup, fov) = S.load_json(text)
        sc = fr.Scene.from_json(text, w, h)
        return prims, sc.camera, O.camera_look(frm, at, vup, fov, 0.1, w, h), w, h, sc
    parts = src.split(":")
    if parts[0] == "edge":
        fx = X.fixture(parts[1], parts[2])
        prims = X.lattice(parts[1], "small", fx.shift)
    else:
        fx = M.fixture(parts[1], parts[2], parts[3])
        prims = M.scene(parts[1], parts[2], fx)
    cam, ocam = X.edge_camera(fr, w=w, h=h, **fx.cam)
    return prims, cam, ocam, w, h, fr.Scene.from_prims(prims)


def expected(fr, name):
    prims, _, ocam, w, h, _ = case(fr, name)
    return cached(name, prims, ocam, w, h)
