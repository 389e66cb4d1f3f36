"""Frame time of the interactive path, tracer.rs:30-55 update(): one 1-spp frame of the
simple scene (get_simple_scene, max_depth 50) with an orbiting camera, on the model's
persistent render context, including the u8 download into model.pixels.

    python tools/time_update.py [W H] [frames] [--accumulate | --error[=N]]

Prints one JSON line: median / p90 host wall time per update() call, and the same frame
through the one-shot fr_render_hip (a context made and freed per call) for comparison.
--accumulate: the timed calls are update(..., accumulate=True) with no key pressed, so the
camera stands still and every frame continues the accumulation (the resolve's read and write
of the accumulator); "accum_frames" then says how many frames the last picture holds.
--error[=N]: the same frames with accumulate="error" (the resolve also reads and writes Q), and
an accum_error(2^-4) after every N-th frame (default 10) inside the timed call; "error_ms_median"
is the host time of those calls alone and "error" the last summary."""
import json
import os
import sys
import time

ROOT = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fo-rma_amd"))
import forma_rt as fr  # noqa: E402


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    err = [a for a in opts if a.split("=")[0] == "--error"]
    every = int(err[0].split("=")[1]) if err and "=" in err[0] else 10
    accumulate = "error" if err else "--accumulate" in opts
    w, h = (int(argv[0]), int(argv[1])) if len(argv) > 1 else (1920, 1080)
    frames = int(argv[2]) if len(argv) > 2 else 30
    m = fr.create_model(w, h)
    fr.update(m, 0b001000, 1.0 / 60)  # first frame: context, scene upload, buffers
    if accumulate:
        fr.update(m, 0, 1.0 / 60, accumulate=accumulate)  # the accumulator's allocation
    ts, es, summary = [], [], None
    for k in range(frames):
        t = time.perf_counter()
        if accumulate:
            fr.update(m, 0, 1.0 / 60, accumulate=accumulate)
            if err and (k + 1) % every == 0:
                te = time.perf_counter()
                summary = m.ctx.accum_error(2.0 ** -4)
                es.append((time.perf_counter() - te) * 1e3)
        else:
            fr.update(m, 0b001000 if k % 2 else 0b000100, 1.0 / 60)
        ts.append((time.perf_counter() - t) * 1e3)
    st = m.last_stats
    accum_frames = m.ctx.accum_info()[0] if accumulate else 0
    one = []
    for _ in range(5):
        t = time.perf_counter()
        fr.render(m.scene, m.scene.camera, w, h, 1, fr.MAX_DEPTH, 1234)
        one.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    one.sort()
    es.sort()
    extra = {}
    if err:
        extra = {"error_every": every, "error_calls": len(es),
                 "error_ms_median": round(es[len(es) // 2], 3) if es else None, "error": summary}
    print(json.dumps({"workload": f"update() simple scene {w}x{h} 1spp depth 50", "frames": frames,
                      "accumulate": bool(accumulate), "accum_frames": accum_frames, **extra,
                      "ms_median": round(ts[len(ts) // 2], 3), "ms_p90": round(ts[int(0.9 * len(ts))], 3),
                      "kernel_ms": round(st["kernel_ms"], 3), "fps_median": round(1e3 / ts[len(ts) // 2], 1),
                      "one_shot_render_ms_median": round(one[len(one) // 2], 3),
                      "segments_per_sample": round(st["segments"] / st["samples"], 3)}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
