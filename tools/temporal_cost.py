#!/usr/bin/env python3
"""What fr_ctx_temporal costs beside fr_ctx_denoise and fr_ctx_denoise_guided: the
headline scene at 1080p. The three stages of fr_ctx_temporal are timed with HIP events on the
context's sum stream (fr_ctx_trace_log, which = 4): the prior (the reprojection and the copy of
the view's two G-buffer words), totals and prep, and the picture (four levels, or the finalise
kernel), the median of --reps calls each; the calls that keep the prior are enqueued in bursts, back
to back, since a stage that starts on an idle stream reads longer by the idle time. fr_ctx_denoise and fr_ctx_denoise_guided, which log no
events, are timed whole on the host around a drained stream (fr_ctx_wait before and after), and so
is a whole temporal call beside them. Prints one JSON line.

    python3 tools/temporal_cost.py [--scene scene_08] [--width 1920] [--height 1080] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fo-rma_amd"))
import forma_rt as fr  # noqa: E402


def timed(ctx, call):
    ctx.wait()
    t0 = time.perf_counter()
    call()
    ctx.wait()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="scene_08")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    w, h = a.width, a.height
    sc = fr.Scene.from_file(fr.scene_path(a.scene), w, h)
    cams = [sc.camera, fr.FrCamera.from_buffer_copy(sc.camera)]
    fr.camera_translate(cams[1], [0.05, 0.03, 0.0])
    ctx = fr.RenderContext(0)
    seed = [0]

    def view(v, frames=2):
        for _ in range(frames):
            seed[0] += 1
            ctx.render(sc, cams[v], fr.make_params(w, h, 1, 8, seed[0], accumulate="error"))
        ctx.gbuffer(sc, cams[v], w, h)
        ctx.sync()

    med = lambda f: statistics.median(f() for _ in range(a.reps))  # noqa: E731
    view(0)
    out = {"scene": a.scene, "width": w, "height": h, "reps": a.reps}
    out["denoise_4_ms"] = med(lambda: timed(ctx, lambda: ctx.denoise(4)))
    out["denoise_guided_4_ms"] = med(lambda: timed(ctx, lambda: ctx.denoise(4, guided=True)))
    ctx.temporal(0)
    out["temporal_keep_0_ms"] = med(lambda: timed(ctx, lambda: ctx.temporal(0)))  # prep and finalise
    out["temporal_keep_4_ms"] = med(lambda: timed(ctx, lambda: ctx.temporal(4)))
    out["temporal_keep_guided_4_ms"] = med(lambda: timed(ctx, lambda: ctx.temporal(4, guide=True)))
    ctx.trace_log(True)
    for i in range(a.reps):  # a new accumulation of the other view: the call builds the prior
        view(1 - i % 2)
        ctx.temporal(0)
    for _ in range(a.reps):  # then bursts of calls that keep it, enqueued back to back
        ctx.temporal(0)
    for _ in range(a.reps):
        ctx.temporal(4)
    for _ in range(a.reps):
        ctx.temporal(4, guide=True)
    ev = ctx.trace_log_read(temporal=True)
    ctx.trace_log(False)
    assert len(ev) == 12 * a.reps
    n = 3 * a.reps
    col = lambda burst, k: statistics.median(ev[burst * n + k:(burst + 1) * n:3])  # noqa: E731
    out["events"] = {"reproject_and_copies_ms": col(0, 0), "prep_ms": col(1, 1), "finalise_ms": col(1, 2),
                     "prep_before_levels_ms": col(2, 1), "levels_4_ms": col(2, 2), "prep_guided_ms": col(3, 1),
                     "levels_4_guided_ms": col(3, 2)}
    reused = int((ctx.download_temporal(w, h)["reason"] == fr.FR_TP_REUSED).sum())
    out["reused_pixels"] = reused
    ctx.close()
    out["events"] = {k: round(v, 4) for k, v in out["events"].items()}
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
