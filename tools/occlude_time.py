"""Times of occlusion queries (fr_ctx_occluded) against the closest-hit cast (fr_ctx_cast) of the
same rays, at 1920x1080.

On scene_08 (6 boxes: no tree, the list loop) and on the 10,000-sphere generator scene (BASELINE
config C5: a tree), three ray sets: (a) the view's pixel rays with t_max = FLT_MAX, (b) one bounce
ray per hit pixel of the view's G-buffer (o = P, d = N + r, tools/cast_time.py's) with t_max =
FLT_MAX, (c) the same bounce rays with t_max = 5, short probes. The rays are a device tensor
(FR_CAST_RAYS_DEVICE) and the answers stay on the device, so no copy is timed. Per set the two
calls alternate, a warm-up pair and then `passes` pairs in one run, each kernel timed by the launch
log's HIP events (fr_ctx_trace_log_read, which = 5); median, minimum and maximum are reported. The
answers are held against the cast's: a ray is occluded iff the cast of the same range hits.

Prints one JSON line and with --out writes it (indented) to that file:

    python tools/occlude_time.py [--width 1920] [--height 1080] [--spheres 10000] [--passes 20] \
        [--list-passes 0] [--out profiles/occlude_1080p.json]

--list-passes N also times the two calls with FR_CAST_LIST on the sphere scene, N passes.
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
from tools.cast_time import bounce_rays, pixel_rays  # noqa: E402
from tools.gbuffer_time import gen_spheres, summary  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)
SHORT = 5.0


def time_set(ctx, scene, rays_np, t_max, passes, list_walk=False):
    import torch
    L = fr.lib()
    n = len(rays_np)
    rays_np = rays_np.copy()
    rays_np[:, 7] = t_max
    t = torch.from_numpy(rays_np).to("cuda:0")
    torch.cuda.synchronize()
    ptr = C.c_void_p(t.data_ptr())
    flags = fr.FR_CAST_RAYS_DEVICE | fr.FR_CAST_TMAX | (fr.FR_CAST_LIST if list_walk else 0)
    occluded = lambda: fr.check(L.fr_ctx_occluded(ctx._h, scene._h, ptr, n, flags, None))  # noqa: E731
    cast = lambda: fr.check(L.fr_ctx_cast(ctx._h, scene._h, ptr, n, flags))  # noqa: E731
    occluded()
    occ = ctx.download_occluded(n)
    info = ctx.occluded_info()
    cast()
    hit = ctx.download_hits(n)["prim"] != fr.FR_GBUFFER_MISS
    ctx.trace_log(True)
    for _ in range(passes + 1):
        occluded()
        cast()
    ev = ctx.trace_log_read(cast=True)
    ctx.trace_log(False)
    o, c = summary(ev[2::2]), summary(ev[3::2])  # (the first pair is a warm-up)
    del t
    return {"rays": n, "t_max": "FLT_MAX" if t_max == FLT_MAX else t_max, "occluded_event_ms": o, "cast_event_ms": c,
            "occluded_over_cast": round(o["median"] / c["median"], 3), "occluded_below_cast": bool(o["median"] < c["median"]),
            "occluded_rays": int(occ.sum()), "occluded_rays_counted_on_device": info["occluded"],
            "equals_cast_hits": bool(np.array_equal(occ, hit)), "info": info,
            "occluded_rays_per_s": round(n / (o["median"] * 1e-3), 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spheres", type=int, default=10000)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--list-passes", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if fr.device_count() < 1:
        raise SystemExit("occlude_time: no HIP device")
    w, h = a.width, a.height
    ctx = fr.RenderContext(0)
    res = {"what": "fr_ctx_occluded against fr_ctx_cast (both FR_CAST_TMAX) of the same device rays, alternating in one run: "
                   "HIP-event durations of the kernels (which = 5), median / min / max of `passes` passes",
           "shape": [w, h], "passes": a.passes, "lib": os.path.basename(fr.LIB_PATH)}
    scenes = (("scene_08", fr.Scene.from_file(fr.scene_path("scene_08"), w, h)),
              (f"spheres{a.spheres}", fr.Scene.from_json(gen_spheres(a.spheres), w, h)))
    for name, sc in scenes:
        ctx.gbuffer(sc, sc.camera, w, h)
        g = ctx.download_gbuffer(w, h)
        primary = pixel_rays(sc.camera, w, h)
        hit = (g["prim"] != fr.FR_GBUFFER_MISS).reshape(-1)
        bounce = np.ascontiguousarray(bounce_rays(primary, g)[hit])
        res[name] = {"pixel_rays": time_set(ctx, sc, primary, FLT_MAX, a.passes),
                     "bounce_rays": time_set(ctx, sc, bounce, FLT_MAX, a.passes),
                     "bounce_rays_short": time_set(ctx, sc, bounce, SHORT, a.passes)}
        if a.list_passes and name != "scene_08":  # the list loop over every primitive (FR_CAST_LIST): its exit ballot
            res[name + "_list"] = {"pixel_rays": time_set(ctx, sc, primary, FLT_MAX, a.list_passes, True),
                                   "bounce_rays_short": time_set(ctx, sc, bounce, SHORT, a.list_passes, True)}
    ctx.close()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
