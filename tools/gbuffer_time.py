"""Times of the G-buffer pass (fr_ctx_gbuffer) and of the feature-guided filter
(fr_ctx_denoise_guided) at 1920x1080.

- The G-buffer pass of scene_08 (6 boxes: the list loop) and of the 10,000-sphere generator scene
  (BASELINE config C5) through its tree (gbuffer_tree_kernel) and, in the same run and
  alternating, through the list loop over every primitive for every pixel. The tool picks the walk
  for itself through the environment switch FR_GBUFFER_WALK=tree / list (read by fr_ctx_gbuffer
  at every call), times both by the launch log's HIP events too (fr_ctx_trace_log_read, which =
  5), counts the pixels whose bits differ between the two passes and holds the list pass's
  digest against the recorded one.
- The guided filter at the defaults (levels 4, k 4) on eight accumulating 16-spp frames of
  scene_08, and the unguided filter (fr_ctx_denoise) in the same run, the two alternating.

Each figure is the host wall time of a group of `calls` enqueues plus one wait for the stream
they run on (a download call with no target), divided by `calls`, as tools/denoise_time.py
measures; the stream is idle before a group starts, the first group is a warm-up and is dropped,
and the groups' median, minimum and maximum are reported. The passes run on the context's own
sum stream, which no caller's event can bracket.

Prints one JSON line and with --out writes it (indented) to that file:

    python tools/gbuffer_time.py [--width 1920] [--height 1080] [--spheres 10000] [--calls 20] \
        [--groups 7] [--out profiles/gbuffer_1080p.json]
"""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "fo-rma_amd"))
import forma_rt as fr  # noqa: E402

DEPTH, SEED = 8, 0xD100
LIST_DIGEST = "691d200294e3cec5"  # profiles/gbuffer_1080p.json gbuffer_spheres_sha256_16 (10,000 spheres at 1920x1080)
WALK_ENV = "FR_GBUFFER_WALK"
HEADLINE_FRAME_MS, C5_FRAME_MS, UNGUIDED_MS = 14.06, 39.2, 0.24  # profiles/r06ai_bench.json, README, profiles/denoise_1080p.json


def groups_ms(enqueue, wait, calls, groups):
    """ms per call of each group after the warm-up group."""
    out = []
    for g in range(groups + 1):
        wait()  # idle before the group
        t = time.perf_counter()
        for _ in range(calls):
            enqueue()
        wait()
        ms = (time.perf_counter() - t) * 1e3 / calls
        if g:
            out.append(ms)
    return out


def summary(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


def gen_spheres(count):
    spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(ROOT, "tools", "gen_scene.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    return gs.dumps(gs.generator_scene(count, "sphere"))


def digest(g):
    return hashlib.sha256(b"".join(g[k].tobytes() for k in ("prim", "depth", "normal", "position", "albedo"))).hexdigest()[:16]


def set_walk(walk):
    """The walk the following fr_ctx_gbuffer calls of this process take: "tree", "list" or None
    for the library's default."""
    if walk is None:
        os.environ.pop(WALK_ENV, None)
    else:
        os.environ[WALK_ENV] = walk


def differing_pixels(a, b):
    bad = None
    for k in ("prim", "depth", "normal", "position", "albedo"):
        x, y = a[k].view("uint32"), b[k].view("uint32")
        d = (x != y) if x.ndim == 2 else (x != y).any(axis=2)
        bad = d if bad is None else bad | d
    return int(bad.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spheres", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if fr.device_count() < 1:
        raise SystemExit("gbuffer_time: no HIP device")
    w, h = a.width, a.height
    L = fr.lib()
    ctx = fr.RenderContext(0)
    wait_gb = lambda: fr.check(L.fr_ctx_download_gbuffer(ctx._h, None, None, None, None, None))  # noqa: E731
    wait_dn = lambda: fr.check(L.fr_ctx_download_denoised(ctx._h, None, None, None))  # noqa: E731

    # the 10,000-sphere list: one call per group member is tens of ms, so fewer calls per group
    big = fr.Scene.from_json(gen_spheres(a.spheres), w, h)
    set_walk(None)
    ctx.gbuffer(big, big.camera, w, h)
    wait_gb()
    default_walk = ctx.gbuffer_info()
    big_call = lambda: ctx.gbuffer(big, big.camera, w, h)  # noqa: E731
    tree, lst, walks = [], [], {}
    for _ in range(3):  # the two alternating: the same machine state for both
        for walk, out, calls in (("tree", tree, a.calls), ("list", lst, max(1, a.calls // 5))):
            set_walk(walk)
            big_call()
            wait_gb()
            walks[walk] = ctx.gbuffer_info()
            out += groups_ms(big_call, wait_gb, calls, a.groups // 2 + 1)
    # the same two passes by the launch log's events, alternating call by call
    ctx.trace_log(True)
    for _ in range(a.groups + 1):
        for walk in ("tree", "list"):
            set_walk(walk)
            big_call()
    ev = ctx.trace_log_read(cast=True)
    ctx.trace_log(False)
    ev_tree, ev_list = ev[2::2], ev[3::2]  # (the first pair is a warm-up)
    set_walk("list")
    big_call()
    g_list = ctx.download_gbuffer(w, h)
    set_walk("tree")
    big_call()
    g_tree = ctx.download_gbuffer(w, h)
    set_walk(None)
    big_call()
    g_big = ctx.download_gbuffer(w, h)
    c5 = tree if default_walk == "tree" else lst
    hit_big = int((g_big["prim"] != fr.FR_GBUFFER_MISS).sum())

    sc = fr.Scene.from_file(fr.scene_path("scene_08"), w, h)
    for k in range(a.frames):
        ctx.render(sc, sc.camera, fr.make_params(w, h, a.spp, DEPTH, SEED + k, accumulate="error", scene_jit="wait"))
    ctx.sync()
    ctx.gbuffer(sc, sc.camera, w, h)
    wait_gb()
    s08_walk = ctx.gbuffer_info()
    s08 = groups_ms(lambda: ctx.gbuffer(sc, sc.camera, w, h), wait_gb, a.calls, a.groups)
    g_s08 = ctx.download_gbuffer(w, h)
    levels, kk = fr.FR_DN_LEVELS_DEFAULT, fr.FR_DN_K_DEFAULT
    guided_call = lambda: fr.check(L.fr_ctx_denoise_guided(ctx._h, levels, C.c_float(kk), None))  # noqa: E731
    plain_call = lambda: fr.check(L.fr_ctx_denoise(ctx._h, levels, C.c_float(kk)))  # noqa: E731
    guided_call()
    wait_dn()
    guided, plain = [], []
    for _ in range(3):  # the two alternating: the same machine state for both
        guided += groups_ms(guided_call, wait_dn, a.calls, a.groups // 2 + 1)
        plain += groups_ms(plain_call, wait_dn, a.calls, a.groups // 2 + 1)
    by_levels = {}
    for n in range(1, 7):
        by_levels[str(n)] = summary(groups_ms(lambda: fr.check(L.fr_ctx_denoise_guided(ctx._h, n, C.c_float(kk), None)),
                                              wait_dn, a.calls, 3))
    guided_call()
    mean, u8, var = ctx.download_denoised(w, h, want_var=True)
    gd, pl, s8, c5s = summary(guided), summary(plain), summary(s08), summary(c5)
    trs, lss = summary(tree), summary(lst)
    diff = differing_pixels(g_tree, g_list)
    res = {"what": "fr_ctx_gbuffer and fr_ctx_denoise_guided, host wall time of `calls` enqueues plus one wait over `calls`",
           "shape": [w, h], "calls": a.calls, "groups": a.groups,
           "gbuffer_scene_08_ms": s8["median"], "gbuffer_scene_08_spread": [s8["min"], s8["max"]],
           "gbuffer_spheres": a.spheres, "gbuffer_spheres_ms": c5s["median"], "gbuffer_spheres_spread": [c5s["min"], c5s["max"]],
           "gbuffer_spheres_default_walk": default_walk, "gbuffer_scene_08_walk": s08_walk,
           "gbuffer_spheres_walks_forced": walks,
           "gbuffer_spheres_tree_ms": trs["median"], "gbuffer_spheres_tree_spread": [trs["min"], trs["max"]],
           "gbuffer_spheres_list_ms": lss["median"], "gbuffer_spheres_list_spread": [lss["min"], lss["max"]],
           "gbuffer_spheres_list_over_tree": round(lss["median"] / trs["median"], 2),
           "gbuffer_spheres_tree_event_ms": summary(ev_tree), "gbuffer_spheres_list_event_ms": summary(ev_list),
           "gbuffer_spheres_differing_pixels": diff,
           "gbuffer_spheres_tree_sha256_16": digest(g_tree), "gbuffer_spheres_list_sha256_16": digest(g_list),
           "gbuffer_spheres_list_sha256_16_recorded": LIST_DIGEST,
           "tree_is_default_by_rule": bool(diff == 0 and trs["median"] < lss["min"]),
           "gbuffer_spheres_hit_pixels": hit_big, "sphere_tests": a.spheres * w * h,
           "sphere_tests_per_s": round(a.spheres * w * h / (c5s["median"] * 1e-3), 0),
           "c5_frame_ms": C5_FRAME_MS, "gbuffer_spheres_over_c5_frame": round(c5s["median"] / C5_FRAME_MS, 3),
           "accumulation": {"frames": a.frames, "spp": a.spp, "depth": DEPTH}, "levels": levels, "k": kk,
           "sigma_z": fr.FR_DN_SIGMA_Z_DEFAULT, "normal_pow2": fr.FR_DN_NORMAL_POW2_DEFAULT, "demodulate": 1,
           "guided_ms": gd["median"], "guided_spread": [gd["min"], gd["max"]],
           "unguided_ms_same_run": pl["median"], "unguided_spread_same_run": [pl["min"], pl["max"]],
           "unguided_ms_recorded": UNGUIDED_MS, "guided_over_unguided": round(gd["median"] / pl["median"], 2),
           "guided_ms_by_levels": by_levels, "headline_frame_ms": HEADLINE_FRAME_MS,
           "guided_share_of_headline_frame": round(gd["median"] / HEADLINE_FRAME_MS, 4),
           "gbuffer_scene_08_share_of_headline_frame": round(s8["median"] / HEADLINE_FRAME_MS, 4),
           "lib": os.path.basename(fr.LIB_PATH),
           "gbuffer_scene_08_sha256_16": digest(g_s08), "gbuffer_spheres_sha256_16": digest(g_big),
           "guided_sha256_16": hashlib.sha256(mean.tobytes() + u8.tobytes() + var.tobytes()).hexdigest()[:16]}
    ctx.close()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if (w, h, a.spheres) == (1920, 1080, 10000) and digest(g_list) != LIST_DIGEST:
        raise SystemExit(f"gbuffer_time: the list pass's digest {digest(g_list)} is not the recorded {LIST_DIGEST}")


if __name__ == "__main__":
    main()
