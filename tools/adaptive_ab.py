"""Uniform against adaptive convergence on the headline scene: render_converged on scene_08 at
1920x1080 with 16-spp frames and the scene kernel, once with adaptive=False and once with
adaptive=True at the same threshold, fraction and min_samples, on one context each.

Writes profiles/<tag>.json: per mode the frames, the samples traced, the wall time to
convergence, the time spent inside the check (fr_ctx_accum_error / fr_ctx_adapt, which includes
a host wait for the enqueued frames) and for the adaptive run the histogram of the final
per-tile sample counts; and profiles/<tag>_counts.json, the final per-tile count map [135, 240]
(text: profiles hold no binary files).

    python tools/adaptive_ab.py [--threshold 0.05] [--fraction 1.0] [--min-samples 32] \
        [--max-frames 64] [--check-every 1] [--reps 3] [--tag adaptive_ab]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "fo-rma_amd"))
import forma_rt as fr  # noqa: E402

W, H, SPP, DEPTH, SEED = 1920, 1080, 16, 8, 0xADA0


def run(sc, adaptive, a):
    ctx = fr.RenderContext(0)
    ctx.prepare(sc, sc.camera, fr.make_params(W, H, SPP, DEPTH, SEED, accumulate="error", scene_jit="wait"))
    checks = []
    name = "adapt" if adaptive else "accum_error"
    inner = getattr(ctx, name)

    def timed(*args, **kw):
        t = time.perf_counter()
        r = inner(*args, **kw)
        checks.append((time.perf_counter() - t) * 1e3)
        return r

    setattr(ctx, name, timed)
    t = time.perf_counter()
    _, _, s = fr.render_converged(ctx, sc, sc.camera, W, H, SPP, DEPTH, SEED, a.threshold, fraction=a.fraction,
                                  max_frames=a.max_frames, check_every=a.check_every, scene_jit="wait",
                                  adaptive=adaptive, min_samples=a.min_samples)
    wall = (time.perf_counter() - t) * 1e3
    n, _ = ctx.download_counts()
    tiles = n[::8, ::8]  # a tile's pixels share its count
    out = {"mode": "adaptive" if adaptive else "uniform", "frames": s["frames"], "samples_per_pixel_max": s["samples"],
           "traced": s["traced"] if adaptive else s["pixels"] * s["samples"], "converged": s["converged"],
           "pixels": s["pixels"], "max_rel": float(s["max_rel"]), "wall_ms": round(wall, 3),
           "checks": len(checks), "check_ms_total": round(sum(checks), 3),
           "check_ms_median": round(sorted(checks)[len(checks) // 2], 4) if checks else None,
           "count_histogram": {str(int(v)): int(c) for v, c in zip(*np.unique(tiles, return_counts=True))}}
    if adaptive:
        out["active_tiles_last"] = s["active_tiles"]
    ctx.close()
    return out, tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--fraction", type=float, default=1.0)
    ap.add_argument("--min-samples", type=int, default=32)
    ap.add_argument("--max-frames", type=int, default=64)
    ap.add_argument("--check-every", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tag", default="adaptive_ab")
    a = ap.parse_args()
    sc = fr.Scene.from_file(fr.scene_path("scene_08"), W, H)
    runs, tiles = [], None
    for rep in range(a.reps):  # interleaved; the first repetition also warms the kernel cache up
        for adaptive in (False, True):
            r, t = run(sc, adaptive, a)
            r["rep"] = rep
            runs.append(r)
            print(json.dumps(r), flush=True)
            if adaptive:
                tiles = t
    res = {"args": vars(a), "shape": [W, H, SPP, DEPTH], "runs": runs}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", a.tag + ".json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(ROOT, "profiles", a.tag + "_counts.json"), "w") as f:
        f.write('{"what": "samples per pixel of each 8x8 tile after the adaptive run, rows of tiles top to bottom", '
                '"tiles": [\n')
        f.write(",\n".join(json.dumps([int(v) for v in row], separators=(",", ":")) for row in tiles))
        f.write("\n]}\n")


if __name__ == "__main__":
    main()
