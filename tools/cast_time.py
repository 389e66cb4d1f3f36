"""Times of ray queries (fr_ctx_cast) at 1920x1080 rays.

Two batches of W x H rays on scene_08 (6 boxes: no tree, the list loop) and on the 10,000-sphere
generator scene (BASELINE config C5: a tree): the pinhole rays of the view, and one bounce ray per
pixel built from the view's G-buffer (o = P, d = N + r with r uniform in [-1, 1)^3 from a seeded
generator; a miss keeps its pixel ray). The rays are handed over as a device tensor
(FR_CAST_RAYS_DEVICE), so no copy is timed. Each batch is cast through the tree and through the
list (FR_CAST_LIST), the two alternating, and timed twice: by the launch log's HIP events
(fr_ctx_trace_log_read, which = 5) and as the host wall time of a group of `calls` enqueues plus
one wait over `calls`, as tools/gbuffer_time.py measures. The hits of the two walks are compared
bit for bit.

Prints one JSON line and with --out writes it (indented) to that file:

    python tools/cast_time.py [--width 1920] [--height 1080] [--spheres 10000] [--calls 10] \
        [--groups 5] [--out profiles/cast_1080p.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "fo-rma_amd"))
sys.path.insert(0, ROOT)
import forma_rt as fr  # noqa: E402
from tools.gbuffer_time import gen_spheres, groups_ms, summary  # noqa: E402

SEED = 0xCA57


def pixel_rays(cam, w, h):
    """[w h, 8] f32: (o, 0, d, 0) of every pixel, restated in numpy f32 (forma_rt.h)."""
    F = np.float32
    pos, ll, hor, ver = (np.array(list(getattr(cam, n)), F) for n in ("position", "lower_left", "horizontal", "vertical"))
    u = ((np.arange(w, dtype=np.uint32).astype(F) + F(0.5)) / F(w)).astype(F)
    v = (((np.uint32(h) - np.arange(h, dtype=np.uint32)).astype(F) + F(0.5)) / F(h)).astype(F)
    d = ((ll[None, None, :] + u[None, :, None] * hor[None, None, :]) + v[:, None, None] * ver[None, None, :]) - pos[None, None, :]
    rays = np.zeros((h * w, 8), F)
    rays[:, 0:3] = pos
    rays[:, 4:7] = d.reshape(h * w, 3)
    return rays


def bounce_rays(primary, g):
    rays = primary.copy()
    hit = (g["prim"] != fr.FR_GBUFFER_MISS).reshape(-1)
    r = np.random.default_rng(SEED).uniform(-1.0, 1.0, size=(len(rays), 3)).astype(np.float32)
    rays[hit, 0:3] = g["position"].reshape(-1, 3)[hit]
    rays[hit, 4:7] = (g["normal"].reshape(-1, 3) + r)[hit]
    return rays


def hits_equal(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("prim", "t", "normal", "position", "albedo"))


def time_batch(ctx, scene, rays_np, calls, groups):
    import torch
    L = fr.lib()
    n = len(rays_np)
    t = torch.from_numpy(rays_np).to("cuda:0")
    torch.cuda.synchronize()
    ptr = C.c_void_p(t.data_ptr())
    wait = lambda: fr.check(L.fr_ctx_download_hits(ctx._h, None, None, None, None, None))  # noqa: E731
    cast = {"tree": lambda: fr.check(L.fr_ctx_cast(ctx._h, scene._h, ptr, n, fr.FR_CAST_RAYS_DEVICE)),
            "list": lambda: fr.check(L.fr_ctx_cast(ctx._h, scene._h, ptr, n, fr.FR_CAST_RAYS_DEVICE | fr.FR_CAST_LIST))}
    out, hits, wall = {}, {}, {"tree": [], "list": []}
    for walk in ("tree", "list"):
        cast[walk]()
        hits[walk] = ctx.download_hits(n)
        out[walk + "_info"] = ctx.cast_info()
    for _ in range(2):  # the two alternating
        for walk in ("tree", "list"):
            wall[walk] += groups_ms(cast[walk], wait, calls if walk == "tree" else max(1, calls // 5), groups)
    ctx.trace_log(True)
    for _ in range(groups + 1):
        for walk in ("tree", "list"):
            cast[walk]()
    ev = ctx.trace_log_read(cast=True)
    ctx.trace_log(False)
    for k, walk in enumerate(("tree", "list")):
        e = summary(ev[2 + k::2])  # (the first pair is a warm-up)
        out[walk + "_event_ms"] = e
        out[walk + "_wall_ms"] = summary(wall[walk])
        out[walk + "_rays_per_s"] = round(n / (e["median"] * 1e-3), 0)
    out["hits_equal"] = hits_equal(hits["tree"], hits["list"])
    out["hit_rays"] = int((hits["tree"]["prim"] != fr.FR_GBUFFER_MISS).sum())
    out["list_over_tree"] = round(out["list_event_ms"]["median"] / out["tree_event_ms"]["median"], 2)
    del t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spheres", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if fr.device_count() < 1:
        raise SystemExit("cast_time: no HIP device")
    w, h = a.width, a.height
    ctx = fr.RenderContext(0)
    res = {"what": "fr_ctx_cast of W x H device rays: HIP-event duration of the cast kernel (which = 5) and host wall time "
                   "of `calls` enqueues plus one wait over `calls`; tree = the default walk, list = FR_CAST_LIST",
           "shape": [w, h], "rays": w * h, "calls": a.calls, "groups": a.groups, "lib": os.path.basename(fr.LIB_PATH)}
    scenes = (("scene_08", fr.Scene.from_file(fr.scene_path("scene_08"), w, h)),
              (f"spheres{a.spheres}", fr.Scene.from_json(gen_spheres(a.spheres), w, h)))
    for name, sc in scenes:
        ctx.gbuffer(sc, sc.camera, w, h)
        g = ctx.download_gbuffer(w, h)
        primary = pixel_rays(sc.camera, w, h)
        res[name] = {"pixel_rays": time_batch(ctx, sc, primary, a.calls, a.groups),
                     "bounce_rays": time_batch(ctx, sc, bounce_rays(primary, g), a.calls, a.groups)}
    ctx.close()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
