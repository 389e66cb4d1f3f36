"""Time of fr_ctx_denoise on the headline scene: scene_08 at 1920x1080, eight accumulating 16-spp
frames with accumulate="error" and the scene kernel, then groups of 20 fr_ctx_denoise calls at
the defaults (levels 4, k 4), each group timed as the host wall time of its 20 enqueues plus one
wait (fr_ctx_download_denoised with no target), divided by 20. The stream is idle before a group
starts, the first group is a warm-up and is dropped, the groups' median, minimum and maximum are
reported. The same for levels 1 to 6, so the cost of the level at step 2^(L-1) reads as the
difference between L and L-1 levels (the last level of a call also writes the three outputs).

Prints one JSON line and with --out writes it (indented) to that file:

    python tools/denoise_time.py [--width 1920] [--height 1080] [--frames 8] [--spp 16] \
        [--calls 20] [--groups 9] [--out profiles/denoise_1080p.json]

The yardsticks it quotes: the headline frame (bench.py, 14.06 ms per 16-spp frame) and the
traffic floor of prep plus four levels, each pass reading and writing one 16-byte pixel per
image pixel (prep reads 24 bytes of A and Q instead, the last level writes 33 bytes more), at
the 6.29 TB/s copy rate measured on the MI355X.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "fo-rma_amd"))
import forma_rt as fr  # noqa: E402

DEPTH, SEED = 8, 0xD100
HEADLINE_FRAME_MS = 14.06
COPY_TBPS = 6.29


def time_groups(ctx, levels, k, calls, groups):
    """ms per denoise of each group after the warm-up group."""
    L = fr.lib()
    out = []
    for g in range(groups + 1):
        fr.check(L.fr_ctx_download_denoised(ctx._h, None, None, None) if g else 0)  # idle before the group
        t = time.perf_counter()
        for _ in range(calls):
            fr.check(L.fr_ctx_denoise(ctx._h, levels, C.c_float(k)))
        fr.check(L.fr_ctx_download_denoised(ctx._h, None, None, None))
        ms = (time.perf_counter() - t) * 1e3 / calls
        if g:
            out.append(ms)
    return out


def summary(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--groups", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if fr.device_count() < 1:
        raise SystemExit("denoise_time: no HIP device")
    w, h = a.width, a.height
    sc = fr.Scene.from_file(fr.scene_path("scene_08"), w, h)
    ctx = fr.RenderContext(0)
    for k in range(a.frames):
        ctx.render(sc, sc.camera, fr.make_params(w, h, a.spp, DEPTH, SEED + k, accumulate="error", scene_jit="wait"))
    ctx.sync()
    levels, kk = fr.FR_DN_LEVELS_DEFAULT, fr.FR_DN_K_DEFAULT
    default = time_groups(ctx, levels, kk, a.calls, a.groups)
    by_levels = {str(n): summary(time_groups(ctx, n, kk, a.calls, a.groups)) for n in range(1, 7)}
    again = time_groups(ctx, levels, kk, a.calls, a.groups)  # the same command again: the run-to-run spread
    px = w * h
    floor_bytes = px * (24 + 16) + levels * px * 32 + px * 33
    floor_ms = floor_bytes / (COPY_TBPS * 1e12) * 1e3
    d = summary(default)
    mean, u8, var = ctx.download_denoised(w, h, want_var=True)
    res = {"what": "fr_ctx_denoise, scene_08, host wall time of `calls` enqueues plus one wait over `calls`",
           "shape": [w, h, a.spp, DEPTH], "frames": a.frames, "levels": levels, "k": kk, "calls": a.calls,
           "groups": a.groups, "ms_per_denoise": d["median"], "ms_per_denoise_spread": [d["min"], d["max"]],
           "ms_per_denoise_repeat": summary(again), "ms_per_level": round(d["median"] / levels, 5),
           "ms_by_levels": by_levels, "headline_frame_ms": HEADLINE_FRAME_MS,
           "share_of_headline_frame": round(d["median"] / HEADLINE_FRAME_MS, 4),
           "traffic_floor_bytes": floor_bytes, "traffic_floor_ms": round(floor_ms, 4),
           "times_the_floor": round(d["median"] / floor_ms, 2),
           "lib": os.path.basename(fr.LIB_PATH), "env": {k: v for k, v in os.environ.items() if k.startswith("FR_DN_")},
           "mean_sum": float(mean.astype("float64").sum()), "u8_sum": int(u8.astype("uint64").sum()),
           "var_sum": float(var.astype("float64").sum()),
           "sha256_16": hashlib.sha256(mean.tobytes() + u8.tobytes() + var.tobytes()).hexdigest()[:16]}
    ctx.close()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
