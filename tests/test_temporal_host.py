"""Temporal reuse of a progressive accumulation (fr_ctx_temporal) without a device.

- tests/c/temporal_check.cpp, a CPU program built with -fsanitize=address,undefined
  -fno-sanitize-recover=all -ffp-contract=off, runs the arithmetic the kernels compile
  (fo-rma_amd/csrc/temporal.h) and plan.cpp's temporal_step; the numpy f32 restatement the GPU
  tests rely on (tests/temporal_ref.py, written from DESIGN.md §4.5f) must equal its bits in every
  downloadable field over a sequence of views V0 -> V1 -> V2, and its decisions as printed.
- Quality, on oracle frames only: a moved camera's first frame with the previous view's history
  is closer to a 4096-spp frame than the raw frame (this pins the definition, not the product).
- The header, the Python mirror and update()'s keyword carry the feature as specified, and
  tests/c/temporal_abi.c checks the prototypes and the options' layout from C."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import denoise_guided_ref as DG
from tests import temporal_fixtures as X
from tests import temporal_ref as T
from tests.test_denoise_guided_host import OTHER
from tests.test_plan import ROOT

F = np.float32
FR_EARG = -1


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("temporal") / "temporal_check")
    srcs = [os.path.join(ROOT, "tests", "c", "temporal_check.cpp")] + [
        os.path.join(ROOT, "fo-rma_amd", "csrc", f) for f in ("plan.cpp", "pack.cpp", "json_min.cpp", "scene.cpp", "bvh.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), *srcs, "-o", out], check=True, timeout=600)
    return out


def _run(exe_path, args):
    """The stand-alone sanitizer program: it must end clean."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, *args], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return p.stdout


def _g_words(g):
    g0 = np.concatenate([_bits(g["normal"]), _bits(g["depth"])[..., None]], -1)
    g1 = np.concatenate([_bits(g["position"]), np.asarray(g["prim"], np.uint32)[..., None]], -1)
    return g0.ravel(), g1.ravel()


def _header_view(exe_path, tmp_path, name, a, q, n, frames, g, cls, hist, levels, k, guide, opt):
    """One call of one view on temporal.h's own functions: the dict of T.FIELDS as bits, plus
    "mean", "var" (bits), "u8" and "valid". hist: None, or {"g", "cam", "ta", "tq"} with the
    previous view's features, camera fields and totals as [H, W, 4] bit arrays."""
    h, w = a.shape[:2]
    n = np.broadcast_to(np.asarray(n, np.uint32), (h, w))
    frames = np.broadcast_to(np.asarray(frames, np.uint32), (h, w))
    gd = dict(dict(sigma_z=DG.SIGMA_Z, normal_pow2=DG.NORMAL_POW2, demodulate=True), **(guide or {}))
    o = dict(T.OPT, **opt)
    head = np.concatenate([np.array([w, h, levels], np.uint32), _bits(F(k)).reshape(1),
                           np.array([int(guide is not None)], np.uint32), _bits(F(gd["sigma_z"])).reshape(1),
                           np.array([gd["normal_pow2"], int(gd["demodulate"])], np.uint32),
                           _bits(np.array([o["n_max"], o["n_max_specular"], o["sigma_z"], o["normal_min"]], F)),
                           np.array([int(hist is not None), len(cls)], np.uint32)])
    cam = _bits(np.concatenate(hist["cam"])) if hist is not None else np.zeros(12, np.uint32)
    words = [head, np.asarray(cls, np.uint32), cam, _bits(a).ravel(), _bits(q).ravel(), n.ravel(), frames.ravel(),
             *_g_words(g), _bits(g["albedo"]).ravel()]
    if hist is not None:
        words += [*_g_words(hist["g"]), hist["ta"].ravel(), hist["tq"].ravel()]
    path = str(tmp_path / f"{name}.bin")
    np.concatenate(words).tofile(path)
    rows = np.array([[int(t, 16) for t in line.split()] for line in _run(exe_path, ["view", path]).splitlines()], np.uint32)
    assert rows.shape == (w * h, 26)
    r = rows.reshape(h, w, 26)
    return {"prior_a": r[..., 0:3], "prior_n": r[..., 3], "prior_q": r[..., 4:7], "prior_k": r[..., 7],
            "total_a": r[..., 8:11], "total_n": r[..., 11], "total_q": r[..., 12:15], "total_k": r[..., 15],
            "source": r[..., 16], "reason": r[..., 17], "mean": r[..., 18:21], "var": r[..., 21],
            "u8": r[..., 22:25].astype(np.uint8), "valid": r[..., 25].astype(bool), "ta": r[..., 8:12], "tq": r[..., 12:16]}


def _same(got, want, name):
    """Every field of the header's call equals the restatement's, NaN for NaN of any payload."""
    for f in T.FIELDS + ("mean", "var"):
        gb = got[f]
        wb = want[f] if f in ("source", "reason") else _bits(want[f])
        nan = np.zeros(wb.shape, bool) if f in ("source", "reason") else (
            np.isnan(gb.view(F)) & np.isnan(wb.view(F)))
        assert np.array_equal(gb[~nan], wb[~nan]), (name, f, int(np.count_nonzero(gb[~nan] != wb[~nan])))
    assert np.array_equal(got["u8"], want["u8"]), name


def _hold_sequence(check, tmp_path, name, levels, k, guide):
    """X.SEQUENCE through the restatement and, call by call, through the header: the prior of a
    view is reprojected from the header's own totals of the view before."""
    want = X.run(name, X.SEQUENCE, levels, k, guide)
    cams, cls, opt = X.oracle_views(name), X.classes(name), X.CASES[name][4]
    from tests import accum_error_ref as R
    comp, cur, frames, prev, last, calls = None, None, 0, None, None, 0
    for op in X.SEQUENCE:
        if op[0] == "frame":
            if op[1] != cur:
                comp, cur, prev = R.ErrorComposite(), op[1], last  # the history freezes at the view before's last call
            comp.add(X.frame_sum(name, cur, X.SEED0 + frames), X.SPP)
            frames += 1
            continue
        g = X.features(name, cur)
        got = _header_view(check, tmp_path, f"{name}_{calls}", comp.a, comp.q, comp.n, comp.frames, g, cls, prev, levels, k,
                           guide, opt)
        _same(got, want[calls], (name, calls))
        assert want[calls]["action"] == ("keep" if calls % 2 else "empty" if prev is None else "reproject")
        last = dict(g=g, cam=T.cam_fields(cams[cur]), ta=got["ta"], tq=got["tq"])
        calls += 1
    return want


@pytest.mark.parametrize("name", ["spheres", "spheres_33x17", "boxes", "metal"])
def test_sequence_bits_equal_the_numpy_restatement(check, tmp_path, name):
    want = _hold_sequence(check, tmp_path, name, 4, 4.0, None)
    reused = [int((r["reason"] == T.REUSED).sum()) for r in want]
    assert reused[0] == reused[1] == 0 and min(reused[2:]) > 0
    for r in want[:2]:
        assert (r["reason"] == T.NO_HISTORY).all() and (r["source"] == T.NONE).all() and not r["prior_n"].any()
    for i in (0, 2, 4):  # a still view's later call keeps the prior's bits
        for f in ("prior_a", "prior_q", "prior_n", "prior_k", "source", "reason"):
            assert np.array_equal(_bits(want[i][f]) if want[i][f].dtype == F else want[i][f],
                                  _bits(want[i + 1][f]) if want[i][f].dtype == F else want[i + 1][f])
    if name == "metal":
        # n_max 6 scales the 12-sample history; the specular cap of 0 reuses nothing on metal and glass
        r, g, cls = want[2], X.features(name, 1), X.classes(name)
        ok = r["reason"] == T.REUSED
        spec = ok & np.isin(cls[np.where(ok, g["prim"], 0)], (T.SC_METAL, T.SC_DIELECTRIC))
        assert spec.any() and not r["prior_n"][spec].any() and not r["prior_k"][spec].any()
        assert (r["source"][spec] != T.NONE).all()
        assert (ok & ~spec).any() and (r["prior_n"][ok & ~spec] == 6).all()
        assert np.allclose(r["prior_k"][ok & ~spec], 1 + (3 - 1) * 0.5)


@pytest.mark.parametrize("levels,guide", [(0, None), (1, None), (0, {}), (1, {}), (4, {}), (0, OTHER), (4, OTHER)])
def test_levels_and_guides_bits_equal_the_numpy_restatement(check, tmp_path, levels, guide):
    _hold_sequence(check, tmp_path, "spheres", levels, 4.0, guide)


def test_every_code_and_tiled_counts_bits_equal_the_numpy_restatement(check, tmp_path):
    """The pair that reaches every reason code (tests/test_temporal_fixtures.py), NaN totals
    included, with per-tile counts in the second view."""
    name = "codes"
    first = X.run(name, (("frame", 0), ("frame", 0), ("call",)), 0)[0]
    g0, g1, cls, cams, opt = X.features(name, 0), X.features(name, 1), X.classes(name), X.oracle_views(name), X.CASES[name][4]
    hist = dict(g=g0, cam=T.cam_fields(cams[0]), total_a=first["total_a"], total_q=first["total_q"],
                total_n=first["total_n"], total_k=first["total_k"])
    hist_bits = dict(g=g0, cam=hist["cam"], ta=np.concatenate([_bits(first["total_a"]), _bits(first["total_n"])[..., None]], -1),
                     tq=np.concatenate([_bits(first["total_q"]), _bits(first["total_k"])[..., None]], -1))
    from tests import accum_error_ref as R
    comp = R.ErrorComposite()
    comp.add(X.frame_sum(name, 1, X.SEED0 + 2), X.SPP)
    h, w = g1["prim"].shape
    ty, tx = np.arange(h)[:, None] // 8, np.arange(w)[None, :] // 8
    odd = (ty + tx) % 2 == 1
    n, k = np.where(odd, 12, 4).astype(np.uint32), np.where(odd, 3, 1).astype(np.uint32)
    for levels, guide in ((0, None), (4, {})):
        prior = T.reproject(g1, cls, hist, **dict(T.OPT, **opt))
        tot = T.totals(comp.a, comp.q, n, k, prior)
        mean, u8, var = T.show(tot, g1["prim"] == T.NONE, levels, 4.0, g1 if guide is not None else None)
        got = _header_view(check, tmp_path, f"codes_{levels}", comp.a, comp.q, n, k, g1, cls, hist_bits, levels, 4.0, guide, opt)
        _same(got, dict(prior, **tot, mean=mean, u8=u8, var=var), (name, levels))
        assert set(np.unique(prior["reason"])) == set(range(8)) - {T.NO_HISTORY}
        assert np.array_equal(got["valid"], T.prep(tot, g1["prim"] == T.NONE, g1 if guide is not None else None)[2])
        first_frame = tot["total_k"] < 2
        assert first_frame.any() and (~first_frame).any() and got["valid"][first_frame].any()


def test_temporal_step_decisions(check):
    """plan.cpp's temporal_step, as printed, against the restatement's rules: an empty prior first,
    the prior kept within a generation, a reprojection when it changed and the history's scene,
    size and depth match, the history dropped otherwise and after a reset."""
    calls = ["1:7:32:24:8", "1:7:32:24:8", "2:7:32:24:8", "2:7:32:24:8", "3:7:32:24:8", "5:7:32:24:8", "6:8:32:24:8",
             "7:8:32:24:8", "8:8:33:24:8", "9:8:33:17:8", "10:8:33:17:50", "10:8:33:17:50", "reset", "10:8:33:17:50",
             "11:8:33:17:50", "reset", "12:8:33:17:50"]
    want, state = [], None
    for c in calls:
        if c == "reset":
            state = None
            want.append("reset")
            continue
        gen, uid, w, h, d = (int(x) for x in c.split(":"))
        action, read, write, state = T.step(state, gen, (uid, w, h, d))
        want.append(f"{action} {read} {write}")
    got = _run(check, ["step", *calls]).splitlines()
    assert got == want
    assert got[:6] == ["empty 0 1", "keep 0 1", "reproject 1 0", "keep 1 0", "reproject 0 1", "reproject 1 0"]
    assert got[6] == "empty 0 1" and got[7] == "reproject 1 0" and got[8:11] == ["empty 0 1"] * 3
    assert got[11:] == ["keep 0 1", "reset", "empty 0 1", "reproject 1 0", "reset", "empty 0 1"]


# ---- quality ------------------------------------------------------------------------------
# Two 4-spp frames of V0, then one 4-spp frame of V1 after the small move; ref: a 4096-spp frame of
# V1 of seed 999. The ratios sum (shown - ref)^2 / sum (raw V1 frame - ref)^2 recorded in DESIGN.md
# §5 at the defaults: (case, guided, levels 0, levels 4). The condition, both ratios under 1, is
# asserted on the spheres scene ("spheres": the view of every other test, sky in the frame) and on
# every other row too; each row is also held to the recorded ratio x 1.25, which only leaves room for
# a later change of reference seeds, as tests/test_denoise_guided_host.py's does. On "spheres" the
# margin is small (0.87 and 0.91): half the frame is sky, which has no history and which the
# filter must leave alone (a miss without history takes a variance of 0: with the relative error of
# 1 of the other first-frame pixels the unguided levels read 2.15, worse than the raw frame).
QUALITY = [("spheres", False, 0.8698, 0.9117), ("spheres", True, 0.8698, 0.8274),
           ("spheres_down", False, 0.4182, 0.1841), ("spheres_down", True, 0.4182, 0.2846),
           ("boxes", False, 0.4361, 0.0367), ("boxes", True, 0.4361, 0.0402),
           ("scene_01", False, 0.4414, 0.0787), ("scene_01", True, 0.4414, 0.0769),
           ("metal_near", False, 0.5537, 0.3708), ("metal_near", True, 0.5537, 0.3134)]


def quality(name, guided, opt=None):
    script = (("frame", 0), ("frame", 0), ("call",), ("frame", 1), ("call",))
    ref = (X.frame_sum(name, 1, 999, 4096) / F(4096)).astype(np.float64)
    raw = (X.frame_sum(name, 1, X.SEED0 + 2) / F(X.SPP)).astype(np.float64)
    e = lambda img: float(np.sum((img.astype(np.float64) - ref) ** 2))  # noqa: E731
    out = []
    for levels in (0, 4):
        shown = X.run(name, script, levels, 4.0, {} if guided else None, dict(T.OPT, **(opt or {})))[1]["mean"]
        out.append(e(shown) / e(raw))
    return out


@pytest.mark.parametrize("name,guided,rec0,rec4", QUALITY)
def test_the_definition_removes_noise(name, guided, rec0, rec4):
    r0, r4 = quality(name, guided)
    print(f"{name} guided={guided}: levels 0 {r0:.4f} (recorded {rec0}), levels 4 {r4:.4f} (recorded {rec4})")
    assert r0 < 1 and r4 < 1  # the condition
    assert r0 <= rec0 * 1.25 and r4 <= rec4 * 1.25


# ---- the surface ----------------------------------------------------------------------------

def test_header_and_python_mirror(fr):
    import ctypes as C
    import inspect
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    assert ("int fr_ctx_temporal(fr_ctx* ctx, uint32_t levels, float k, const fr_denoise_guide* guide, "
            "const fr_temporal* opt);") in hdr
    assert "int fr_ctx_temporal_reset(fr_ctx* ctx);" in hdr and "int fr_ctx_download_temporal(fr_ctx* ctx," in hdr
    assert "#define FR_ABI_VERSION 6" in hdr and "fr_ctx_temporal_reset, fr_ctx_download_temporal) */" in hdr
    for sym in ("fr_ctx_temporal", "fr_ctx_temporal_reset", "fr_ctx_download_temporal"):
        assert sym in fr.EXPORTS and hasattr(fr.lib(), sym)
    assert C.sizeof(fr.FrTemporal) == 32
    assert (fr.FR_TP_N_MAX_DEFAULT, fr.FR_TP_N_MAX_SPECULAR_DEFAULT, fr.FR_TP_SIGMA_Z_DEFAULT, fr.FR_TP_NORMAL_MIN_DEFAULT) == (
        T.N_MAX, T.N_MAX_SPECULAR, T.SIGMA_Z, T.NORMAL_MIN)
    assert (fr.FR_TP_REUSED, fr.FR_TP_NO_HISTORY, fr.FR_TP_MISS, fr.FR_TP_OFFSCREEN, fr.FR_TP_ID, fr.FR_TP_NORMAL,
            fr.FR_TP_PLANE, fr.FR_TP_HISTORY, fr.FR_TP_NONE) == (*range(8), T.NONE)
    sig = inspect.signature(fr.RenderContext.temporal)
    assert [sig.parameters[p].default for p in ("levels", "k", "guide", "n_max", "n_max_specular", "sigma_z", "normal_min")] == [
        4, 4.0, None, T.N_MAX, T.N_MAX_SPECULAR, T.SIGMA_Z, T.NORMAL_MIN]
    assert hasattr(fr.RenderContext, "temporal_reset") and hasattr(fr.RenderContext, "download_temporal")
    assert "fr_ctx_temporal" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert fr.lib().fr_ctx_temporal(None, 4, C.c_float(4.0), None, None) == FR_EARG
    assert fr.lib().fr_ctx_temporal_reset(None) == FR_EARG


def test_update_refuses_temporal_without_the_estimate(fr):
    m = fr.create_model(8, 8)
    for mode in ("temporal", "temporal-guided"):
        for acc in (False, True):
            with pytest.raises(ValueError, match=f"denoise='{mode}' needs accumulate"):
                fr.update(m, 0, 0.1, accumulate=acc, denoise=mode)
    assert m.frame == 0 and m.ctx is None
    m.close()


def test_prototypes_from_c(tmp_path, fr):
    exe_path = str(tmp_path / "temporal_abi")
    libdir = os.path.join(ROOT, "fo-rma_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "temporal_abi.c"), "-L", libdir, "-lforma_rt",
                    f"-Wl,-rpath,{libdir}", "-o", exe_path], check=True)
    got = json.loads(subprocess.run([exe_path], check=True, capture_output=True, text=True).stdout)
    assert got == {"none": 0xFFFFFFFF, "reasons": list(range(8)), "n_max": T.N_MAX, "n_max_specular": T.N_MAX_SPECULAR,
                   "n_max_max": 2.0 ** 24, "sigma_z": T.SIGMA_Z, "normal_min": pytest.approx(T.NORMAL_MIN, abs=1e-8),
                   "size": 32, "offsets": [0, 4, 8, 12, 16], "abi_version": 6, "null_rc": [FR_EARG] * 3}
