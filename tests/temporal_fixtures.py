"""The views the temporal-reuse tests share (tests/test_temporal_host.py, test_temporal_fixtures.py,
test_temporal.py): per case a scene, a size and a list of camera moves V0, V1, V2 ..., each applied
to the camera the move before left; the oracle's frames and first hits of every view, computed
once. Frames are 4 spp at depth 8. Not a test module."""
import functools

import numpy as np

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import accum_error_ref as R
from tests import gbuffer_ref as G
from tests import nonfinite_fixtures as N
from tests import temporal_ref as T
from tests.test_accumulate import _oracle_scene, _product_scene

F = np.float32
SPP, DEPTH, SEED0 = 4, 8, 0x7E40

# name: (scene, width, height, moves, options). The orbits are small (V0 -> V1 keeps most of the
# picture), the translate re-aims the camera (camera.rs translate looks at (0, 0, -1)).
# 40 is no multiple of the 32-pixel workgroup's width, 17 none of its 8 rows.
CASES = {
    "spheres": ("builtin0", 32, 24, (("orbit", (0.3, 0.5, 0.0)), ("orbit", (0.04, 0.02, 0.0)),
                                     ("translate", (0.1, 0.0, 0.0))), {}),
    "spheres_33x17": ("builtin0", 33, 17, (("orbit", (0.3, 0.5, 0.0)), ("orbit", (-0.03, 0.0, 0.0)),
                                           ("translate", (0.0, 0.1, 0.0))), {}),
    "boxes": ("scene_08", 40, 24, (("translate", (0.5, 0.0, 0.0)), ("translate", (0.6, 0.4, 0.0)),
                                   ("orbit", (0.02, 0.0, 0.0))), {}),
    "scene_01": ("scene_01", 33, 17, (("translate", (0.5, 0.0, 0.0)), ("translate", (0.05, 0.03, 0.0))), {}),
    # the quality rows' views: the spheres from above, where the ground fills the frame (no pixel
    # misses), and the objects scene from nearby
    "spheres_down": ("builtin0", 32, 24, (("orbit", (1.45, 1.5, -3.5)), ("orbit", (0.04, 0.02, 0.0))), {}),
    "metal_near": ("builtin2", 32, 24, (("orbit", (1.3, 0.3, -3.0)), ("orbit", (0.04, 0.02, 0.0))), {}),
    # objects_scene: two metal and two dielectric spheres; n_max 6 scales the history, the
    # specular cap of 0 reuses nothing on them
    "metal": ("builtin2", 32, 24, (("orbit", (0.3, 0.5, 0.0)), ("orbit", (0.04, 0.02, 0.0)),
                                   ("translate", (0.1, 0.0, 0.0))), dict(n_max=6.0, n_max_specular=0.0)),
    # a tight plane test and a loose normal test: curved surfaces reach "plane distance"
    "spheres_tight": ("builtin0", 32, 24, (("orbit", (0.3, 0.5, 0.0)), ("orbit", (0.04, 0.02, 0.0))),
                      dict(sigma_z=2.0 ** -9, normal_min=0.5)),
    # every reason code in one pair (codes_scene below); the tight plane test and the loose normal
    # test leave both reachable on the spheres, the normal test also on the box's edges
    "codes": ("codes", 32, 24, (("orbit", (0.5, 0.6, 0.0)), ("orbit", (0.06, 0.05, 0.0))),
              dict(sigma_z=2.0 ** -9, normal_min=0.5)),
}


def codes_scene():
    """Objects before the sky over a far ground that the second view sees more of: a diffuse
    sphere and a diffuse box seen from a corner (its faces meet in edges where the id stays and the normal turns), a metal sphere, and a small
    sphere whose colour has a NaN component: every path that meets it leaves a NaN pixel, so its
    own pixels carry non-finite totals."""
    return [S.sphere((-0.9, 0.0, 0.0), 0.6, S.LAMBERTIAN, (0.2, 0.6, 0.3), 0.0),
            S.prim(S.AABB, S.LAMBERTIAN, (0.7, 0.4, 0.1), 0.0, (0.1, -0.5, -0.5, 1.1, 0.5, 0.5)),
            S.sphere((0.0, 1.1, 0.0), 0.4, S.METAL, (0.9, 0.9, 0.9), 0.1),
            S.sphere((0.2, -1.3, 0.3), 0.35, S.LAMBERTIAN, (0.5, np.nan, 0.5), 0.0),
            S.sphere((0.0, -1002.0, 0.0), 1000.0, S.LAMBERTIAN, (0.3, 0.3, 0.3), 0.0)]


def scene(fr, name):
    """(oracle prims, product Scene or None without fr, w, h) of a case."""
    key, w, h, _, _ = CASES[name]
    if key == "codes":
        prims = codes_scene()
        return prims, (fr.Scene.from_prims(prims) if fr else None), w, h
    if key.startswith("builtin"):
        which = int(key[len("builtin"):])
        return S.BUILTIN[which](), (fr.Scene.builtin(which, w, h) if fr else None), w, h
    return _oracle_scene(key, w, h)[0], (_product_scene(fr, key, w, h) if fr else None), w, h


def _base_camera(name):
    key, w, h, _, _ = CASES[name]
    return O.camera_new(w, h) if key.startswith("builtin") or key == "codes" else _oracle_scene(key, w, h)[1]


def oracle_views(name):
    """The OrCamera of every view."""
    cam, out = _base_camera(name), []
    for kind, delta in CASES[name][3]:
        cam = O.OrCamera.from_buffer_copy(cam)
        (O.camera_orbit if kind == "orbit" else O.camera_translate)(cam, list(delta))
        out.append(cam)
    return out


def product_views(fr, name, sc):
    """The FrCamera of every view, moved by the product's own camera functions."""
    cam, out = sc.camera if sc.camera is not None else fr.camera_new(CASES[name][1], CASES[name][2]), []
    for kind, delta in CASES[name][3]:
        cam = fr.FrCamera.from_buffer_copy(cam)
        (fr.camera_orbit if kind == "orbit" else fr.camera_translate)(cam, list(delta))
        out.append(cam)
    return out


@functools.lru_cache(maxsize=None)
def features(name, view):
    prims, _, w, h = scene(None, name)
    return G.gbuffer(prims, oracle_views(name)[view], w, h)


@functools.lru_cache(maxsize=None)
def classes(name):
    return T.scatter_classes(scene(None, name)[0])


@functools.lru_cache(maxsize=None)
def frame_sum(name, view, seed, spp=SPP, depth=DEPTH):
    """S = mean * spp of one oracle frame of a view, read-only."""
    prims, _, w, h = scene(None, name)
    mean, _, _, rows = O.render(prims, oracle_views(name)[view], w, h, spp, depth, seed=seed, threads=8)
    assert rows == h
    s = N.frame_sum(mean, spp)
    s.setflags(write=False)
    return s


def key_of(name, uid=0, depth=DEPTH):
    _, w, h, _, _ = CASES[name]
    return (uid, w, h, depth)


def run(name, script, levels=4, k=4.0, guide=None, opt=None):
    """The restatement over a script of steps: ("frame", view) adds one frame of the view (another
    view, or one after "restart", starts a new accumulation), ("restart",) is fr_ctx_accum_reset,
    ("reset",) fr_ctx_temporal_reset, ("call",) fr_ctx_temporal. Returns the list of the calls'
    results (tests/temporal_ref.py's Temporal.call)."""
    opt = dict(CASES[name][4], **(opt or {}))
    tp, comp, cur, gen, frames, out = T.Temporal(), None, None, 0, 0, []
    cams = oracle_views(name)
    for op in script:
        if op[0] == "frame":
            if comp is None or op[1] != cur:
                comp, cur, gen = R.ErrorComposite(), op[1], gen + 1
            comp.add(frame_sum(name, cur, SEED0 + frames), SPP)
            frames += 1
        elif op[0] == "restart":
            comp = None
        elif op[0] == "reset":
            tp.reset()
        else:
            out.append(tp.call(gen, key_of(name), comp.a, comp.q, comp.n, comp.frames, features(name, cur), cams[cur],
                               classes(name), levels, k, guide, **opt))
    return out


# V0 -> V1 -> V2 with two frames, a call, another frame and a call in every view
SEQUENCE = tuple(op for v in range(3) for op in (("frame", v), ("frame", v), ("call",), ("frame", v), ("call",)))
