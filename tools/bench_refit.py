"""What a moving scene costs per frame: fr_scene_update's in-place catch-up (records patched,
tree refitted on the device) against the only way without it, a new scene of the moved list
(pack, host SAH build, upload).

Three measurements on one device, each warm, device times by HIP events (fr_ctx_scene_info's
parts of the catch-up, fr_stats.kernel_ms of a render), host times as wall time around calls that
end in a wait:

- frame: the generator's sphere scene (10,000 spheres, BASELINE config C5) at W x H. Every frame
  moves every sphere (its own y offset, a new one each frame, inside the extent) and then runs
  (a) one cast of the view's primary rays (a device tensor) or (b) one 16-spp frame. `rebuild`
  is fr_scene_create of the moved list (from a numpy buffer, no per-primitive Python) followed by
  the same call; `inplace` is Scene.set_spheres followed by the same call. Reported: wall ms per
  frame of both, the host time of the edit call itself, and the catch-up's parts.
- quality: the same scene with every sphere moved by about one grid spacing (5 units): the trace
  kernel's time of one 16-spp frame on the refitted tree against the tree of Scene.rebuild() over
  the same list.
- overlap: `--frames` streamed 16-spp frames of the headline scene (scene_08) with a
  one-primitive update before each against none: the step per frame.

The `rebuild` half uses nothing this tool's subject added, so `--baseline-only` runs on a
library without fr_scene_update. Prints one JSON line and with --out writes it (indented):

    python tools/bench_refit.py [--width 1920] [--height 1080] [--spheres 10000] [--reps 12] \
        [--frames 20] [--part all|frame|quality|overlap] [--baseline-only] [--out profiles/refit_1080p.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "fo-rma_amd"))
sys.path.insert(0, ROOT)
import forma_rt as fr  # noqa: E402
from tools.cast_time import pixel_rays  # noqa: E402
from tools.gbuffer_time import gen_spheres, summary  # noqa: E402

F = np.float32
SPP, DEPTH = 16, 8


def prim_words(scene):
    n = len(scene)
    words = np.zeros((n, 22), np.uint32)
    fr.check(fr.lib().fr_scene_get_prims(scene._h, words.ctypes.data_as(C.POINTER(fr.FrPrim)), n))
    return words


def scene_of(words):
    h = C.c_void_p()
    fr.check(fr.lib().fr_scene_create(words.ctypes.data_as(C.POINTER(fr.FrPrim)), len(words), C.byref(h)))
    return fr.Scene(h)


def offsets(base, k, scale):
    """Frame k's centres: every sphere's y moved by its own multiple of 1 / 16 of up to `scale`,
    towards the middle of the scene's y range, so that none leaves the extent."""
    i = np.arange(len(base), dtype=np.int64)
    step = (((i * 7 + k * 13) % 32 + 1) / 32.0 * scale).astype(F)
    out = base.copy()
    mid = 0.5 * (float(base[:, 1].min()) + float(base[:, 1].max()))
    out[:, 1] = np.where(base[:, 1] < mid, base[:, 1] + step, base[:, 1] - step).astype(F)
    return out


def frame_cost(a, res):
    import torch
    w, h = a.width, a.height
    L = fr.lib()
    sc0 = fr.Scene.from_json(gen_spheres(a.spheres), w, h)
    cam = sc0.camera
    words0 = prim_words(sc0)
    base = words0[:, 6:9].copy().view(F)
    rays = torch.from_numpy(pixel_rays(cam, w, h)).to("cuda:0")
    torch.cuda.synchronize()
    ptr, n = C.c_void_p(rays.data_ptr()), w * h
    p = fr.make_params(w, h, SPP, DEPTH)
    ctx = fr.RenderContext(0)

    def cast(sc):
        fr.check(L.fr_ctx_cast(ctx._h, sc._h, ptr, n, fr.FR_CAST_RAYS_DEVICE))
        fr.check(L.fr_ctx_download_hits(ctx._h, None, None, None, None, None))

    def render(sc):
        ctx.render(sc, cam, p)
        return ctx.sync()

    out = {}
    for what, call in (("cast", cast), ("frame16", render)):
        reps = a.reps if what == "cast" else max(3, a.reps // 3)
        walls = {"rebuild": [], "inplace": []}
        edit = {"rebuild": [], "inplace": []}
        parts = {k: [] for k in ("host_ms", "h2d_ms", "patch_ms", "refit_ms")}
        live = scene_of(words0)
        call(live)
        info = None
        for k in range(reps + 1):  # (the first of each is a warm-up)
            centres = offsets(base, k, 2.0)
            for how in (("rebuild",) if a.baseline_only else ("rebuild", "inplace")):
                t0 = time.perf_counter()
                if how == "rebuild":
                    words = words0.copy()
                    words[:, 6:9] = centres.view(np.uint32)
                    sc = scene_of(words)
                    t1 = time.perf_counter()
                    call(sc)
                    t2 = time.perf_counter()
                    sc.close()
                else:
                    live.set_spheres(None, centres)
                    t1 = time.perf_counter()
                    call(live)
                    t2 = time.perf_counter()
                    info = ctx.scene_info(live)
                    assert info["last_sync"] == fr.FR_SCENE_SYNC_REFIT, info
                    if k:
                        for name in parts:
                            parts[name].append(info[name])
                if k:
                    walls[how].append((t2 - t0) * 1e3)
                    edit[how].append((t1 - t0) * 1e3)
        r = {"reps": reps, "rebuild_wall_ms": summary(walls["rebuild"]), "rebuild_edit_call_ms": summary(edit["rebuild"])}
        if not a.baseline_only:
            r.update({"inplace_wall_ms": summary(walls["inplace"]), "inplace_edit_call_ms": summary(edit["inplace"]),
                      "catch_up": {name: summary(v) for name, v in parts.items()},
                      "prims_patched": info["prims_patched"], "nodes_refit": info["nodes_refit"],
                      "refit_launches": info["refit_launches"],
                      "rebuild_over_inplace": round(summary(walls["rebuild"])["median"] / summary(walls["inplace"])["median"], 2)})
        out[what] = r
        live.close()
    ctx.close()
    res["frame"] = out


def tree_quality(a, res):
    w, h = a.width, a.height
    sc = fr.Scene.from_json(gen_spheres(a.spheres), w, h)
    cam = sc.camera
    words0 = prim_words(sc)
    base = words0[:, 6:9].copy().view(F)
    rng = np.random.default_rng(0x5EED)
    moved = base.copy()
    lo, hi = base.min(axis=0), base.max(axis=0)
    moved += rng.uniform(-5.0, 5.0, size=base.shape).astype(F)
    moved = np.clip(moved, lo, hi).astype(F)  # inside the extent
    ctx = fr.RenderContext(0)
    p = fr.make_params(w, h, SPP, DEPTH)

    def kernel_ms(reps=4):
        out = []
        for k in range(reps):
            ctx.render(sc, cam, p)
            st = ctx.sync()
            if k:
                out.append(st["kernel_ms"])
        return out

    still = kernel_ms()
    sc.set_spheres(None, moved)
    refit = kernel_ms()
    info = ctx.scene_info(sc)
    mean_refit = ctx.download(w, h)[0]
    sc.rebuild()
    fresh = kernel_ms()
    mean_fresh = ctx.download(w, h)[0]
    res["quality"] = {"moved_by": "uniform in [-5, 5]^3 per sphere, clipped to the scene's range",
                      "unmoved_kernel_ms": summary(still), "refit_kernel_ms": summary(refit), "rebuilt_kernel_ms": summary(fresh),
                      "refit_over_rebuilt": round(summary(refit)["median"] / summary(fresh)["median"], 3),
                      "refits": info["refits"], "same_image": bool(np.array_equal(mean_refit.view(np.uint32), mean_fresh.view(np.uint32)))}
    ctx.close()


def overlap_lost(a, res):
    w, h = a.width, a.height
    sc = fr.Scene.from_file(fr.scene_path("scene_08"), w, h)
    cam = sc.camera
    ctx = fr.RenderContext(0)
    p = fr.make_params(w, h, SPP, DEPTH)
    prim = sc.prims()[0]
    moved = fr.FrPrim.from_buffer_copy(bytes(prim))
    moved.g[1] = prim.g[1] + 0.125
    moved.g[4] = prim.g[4] + 0.125
    steps = {"still": [], "one_update": []}
    ctx.render(sc, cam, p)
    for g in range(4):  # (the first group is a warm-up)
        for how in ("still", "one_update"):
            ctx.sync()
            t0 = time.perf_counter()
            for k in range(a.frames):
                if how == "one_update":
                    sc.update([0], [moved if k % 2 == 0 else prim])
                ctx.render(sc, cam, p)
            ctx.sync()
            if g:
                steps[how].append((time.perf_counter() - t0) * 1e3 / a.frames)
    res["overlap"] = {"scene": "scene_08", "frames": a.frames, "still_step_ms": summary(steps["still"]),
                      "one_update_step_ms": summary(steps["one_update"]),
                      "lost_ms_per_frame": round(summary(steps["one_update"])["median"] - summary(steps["still"])["median"], 4)}
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spheres", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--part", default="all", choices=("all", "frame", "quality", "overlap"))
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if fr.device_count() < 1:
        raise SystemExit("bench_refit: no HIP device")
    if not a.baseline_only and not hasattr(fr.Scene, "update"):
        raise SystemExit("bench_refit: this library has no fr_scene_update; run with --baseline-only")
    res = {"what": "per-frame cost of a moving scene: in-place update (patch + device refit) against a new scene per frame",
           "shape": [a.width, a.height], "spheres": a.spheres, "spp": SPP, "depth": DEPTH, "lib": os.path.basename(fr.LIB_PATH)}
    parts = [("frame", frame_cost)] + ([] if a.baseline_only else [("quality", tree_quality), ("overlap", overlap_lost)])
    for name, run in parts:
        if a.part in ("all", name):
            run(a, res)
            print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)  # (kept if a later part fails)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
