"""The variance-guided denoise of a progressive accumulation (fr_ctx_denoise) without a device.

- tests/c/denoise_check.cpp, a CPU program built with -fsanitize=address,undefined
  -fno-sanitize-recover=all -ffp-contract=off, runs the arithmetic the kernels compile
  (fo-rma_amd/csrc/denoise.h) on a table of inputs; the numpy f32 restatement the GPU tests rely
  on (tests/denoise_ref.py) must equal its bits.
- The definition removes noise, on oracle frames only: the filtered accumulation is closer to a
  4096-spp frame than the raw one (this pins the definition, not the product).
- The header, the Python mirror and update()'s keyword carry the feature as specified, and
  tests/c/denoise_abi.c checks the three prototypes from C."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import accum_error_ref as R
from tests import denoise_ref as D
from tests.test_accum_error_host import _oracle
from tests.test_plan import ROOT

F = np.float32
FR_EARG = -1
SEED0 = 0xD100


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("denoise") / "denoise_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "denoise_check.cpp"),
                    "-o", out], check=True, timeout=600)
    return out


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _header_bits(exe_path, tmp_path, name, a, q, n, frames, levels, k):
    """Runs denoise.h on the CPU: (mean bits [H, W, 3], var bits [H, W], u8 [H, W, 3], valid [H, W])."""
    h, w = a.shape[:2]
    n = np.broadcast_to(np.asarray(n, np.uint32), (h, w))
    frames = np.broadcast_to(np.asarray(frames, np.uint32), (h, w))
    words = np.concatenate([np.array([w, h, levels], np.uint32), _bits(F(k)).reshape(1), _bits(a).ravel(),
                            _bits(q).ravel(), n.ravel(), frames.ravel()])
    path = str(tmp_path / f"{name}.bin")
    words.tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, path], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    rows = np.array([[int(t, 16) for t in line.split()] for line in p.stdout.splitlines()], np.uint32)
    assert rows.shape == (w * h, 8)
    return (rows[:, :3].reshape(h, w, 3), rows[:, 3].reshape(h, w), rows[:, 4:7].astype(np.uint8).reshape(h, w, 3),
            rows[:, 7].astype(bool).reshape(h, w))


def _hold(check, tmp_path, name, a, q, n, frames, levels=D.LEVELS, k=D.K):
    """denoise_ref equals the header's bits; returns (mean, u8, var, valid) of the reference."""
    got_mean, got_var, got_u8, got_valid = _header_bits(check, tmp_path, name, a, q, n, frames, levels, k)
    mean, u8, var = D.denoise(a, q, n, frames, levels, k)
    valid = D.valid_mask(a, q, n, frames)
    assert np.array_equal(got_valid, valid), name
    assert np.array_equal(got_mean, _bits(mean)), (name, int(np.count_nonzero(got_mean != _bits(mean))))
    assert np.array_equal(got_var, _bits(var)), (name, int(np.count_nonzero(got_var != _bits(var))))
    assert np.array_equal(got_u8, u8), name
    # no output of a valid pixel is NaN; an invalid pixel passes the bits of prep through
    assert not np.isnan(mean[valid]).any() and not np.isnan(var[valid]).any(), name
    c0, v0, _ = D.prep(a, q, n, frames)
    assert np.array_equal(_bits(mean)[~valid], _bits(c0)[~valid]) and np.array_equal(_bits(var)[~valid], _bits(v0)[~valid])
    return mean, u8, var, valid


def _random_table(rng, w, h):
    """A and Q as the resolve builds them from K noisy frames, per-tile n and K that differ."""
    base = rng.random((h, w, 3), dtype=F) * F(2.0)
    base[:, w // 2:] *= F(0.05)  # an edge for the edge-stopping weight
    comp = R.ErrorComposite()
    for _ in range(5):
        spp = int(rng.choice([1, 2, 4, 16]))
        noise = F(1.0) + (rng.random((h, w, 3), dtype=F) - F(0.5)) * F(0.8)
        comp.add((base * noise * F(spp)).astype(F), spp)
    return comp.a, comp.q, comp.n, comp.frames


def test_random_table_bits_equal_the_numpy_restatement(check, tmp_path):
    rng = np.random.default_rng(0xD101)
    w, h = 37, 19
    a, q, n, frames = _random_table(rng, w, h)
    for levels, k in ((4, 4.0), (1, 0.5), (6, 64.0)):
        mean, _, var, valid = _hold(check, tmp_path, f"random_{levels}", a, q, n, frames, levels, k)
        assert valid.all()
    # per-tile counts: another n and K in every other 8x8 tile (A and Q scaled to match would be
    # another accumulation; the arithmetic is what is held)
    ty, tx = np.arange(h)[:, None] // 8, np.arange(w)[None, :] // 8
    odd = (ty + tx) % 2 == 1
    nt = np.where(odd, n + 7, n).astype(np.uint32)
    kt = np.where(odd, frames + 2, frames).astype(np.uint32)
    _hold(check, tmp_path, "random_tiled", a, q, nt, kt)
    # the filter does something: the picture moves, the variance falls
    c0, v0, _ = D.prep(a, q, n, frames)
    assert not np.array_equal(_bits(mean), _bits(c0)) and float(var.sum()) < 0.5 * float(v0.sum())


def test_edge_pixels_bits_equal_the_numpy_restatement(check, tmp_path):
    rng = np.random.default_rng(0xD102)
    w, h = 37, 19
    a, q, n, frames = _random_table(rng, w, h)
    a, q = a.copy(), q.copy()
    fn = F(n)
    edges = {
        "a_nan": ((2, 3), (np.nan, 1.0, 1.0), (1.0, 1.0, 1.0)),
        "a_inf": ((2, 20), (np.inf, 1.0, 1.0), (1.0, 1.0, 1.0)),
        "a_neg_inf": ((9, 9), (1.0, -np.inf, 1.0), (1.0, 1.0, 1.0)),
        "q_inf": ((5, 7), (1.0, 1.0, 1.0), (1.0, np.inf, 1.0)),
        "mean_2p41": ((7, 30), (float(F(2.0 ** 41) * fn), 1.0, 1.0), (1.0, 1.0, 1.0)),
        "mean_2p40_exactly": ((12, 12), (float(F(2.0 ** 40) * fn), 1.0, 1.0), (0.0, 1.0, 1.0)),  # valid: <= the cap
        "var_over_2p80": ((10, 15), (1.0, 1.0, 1.0), (1e30, 1e30, 1e30)),
        "q_below_a2_over_n": ((14, 5), (8.0, 8.0, 8.0), (0.5, 0.25, 0.125)),  # Q - A^2 / n < 0: clamps to 0
        "corner": ((0, 0), (np.nan,) * 3, (np.nan,) * 3),
        "corner_neighbour": ((0, 1), (np.inf,) * 3, (np.inf,) * 3),
        "last": ((h - 1, w - 1), (1.0, np.nan, 1.0), (1.0, 1.0, 1.0)),
    }
    for (y, x), av, qv in edges.values():
        a[y, x], q[y, x] = np.array(av, F), np.array(qv, F)
    assert np.isfinite(a[7, 30]).all() and np.isfinite(a[12, 12]).all()  # (2^41 n is in range)
    mean, u8, var, valid = _hold(check, tmp_path, "edges", a, q, n, frames)
    want_invalid = {"a_nan", "a_inf", "a_neg_inf", "q_inf", "mean_2p41", "var_over_2p80", "corner",
                    "corner_neighbour", "last"}
    for name, ((y, x), _, _) in edges.items():
        assert bool(valid[y, x]) == (name not in want_invalid), name
    assert int((~valid).sum()) == len(want_invalid)
    y, x = edges["q_below_a2_over_n"][0]
    _, v0, _ = D.prep(a, q, n, frames)
    assert v0[y, x] == 0 and np.isfinite(mean[y, x]).all()
    for levels in (1, 6):
        _hold(check, tmp_path, f"edges_{levels}", a, q, n, frames, levels, 0.5)
    # an image of invalid pixels only: everything passes through
    bad = np.full((4, 5, 3), np.nan, F)
    mean, u8, var, valid = _hold(check, tmp_path, "all_invalid", bad, bad, 8, 2)
    assert not valid.any() and (u8 == 0).all()


def test_degenerate_images_bits_equal_the_numpy_restatement(check, tmp_path):
    zero = np.zeros((9, 11, 3), F)
    mean, u8, var, valid = _hold(check, tmp_path, "all_zero", zero, zero, 16, 4)
    # sden = k 0 + 2^-20 > 0 and d2 = 0: every weight is 1, nothing is 0 / 0
    assert valid.all() and (mean == 0).all() and (var == 0).all() and (u8 == 0).all()
    one_a, one_q = np.array([[[3.0, 2.0, 1.0]]], F), np.array([[[5.0, 2.5, 0.75]]], F)
    mean, _, var, valid = _hold(check, tmp_path, "one_pixel", one_a, one_q, 2, 2, 6, 4.0)
    c0, v0, _ = D.prep(one_a, one_q, 2, 2)
    assert valid.all() and np.array_equal(_bits(mean), _bits(c0))  # the centre tap alone: w C / w
    rng = np.random.default_rng(0xD103)
    a, q, n, frames = _random_table(rng, 3, 2)
    _hold(check, tmp_path, "three_by_two", a, q, n, frames, 6, 4.0)


@pytest.mark.parametrize("key,w,h,depth,spps,bound", [
    ("scene_08", 33, 17, 8, (4,) * 4, 0.25),
    ("scene_08", 33, 17, 8, (1, 4, 16, 2), 0.25),
    ("scene_01", 33, 17, 8, (2,) * 4, 0.6),
    ("builtin0", 32, 24, 50, (1,) * 6, 0.8),
])
def test_the_definition_removes_noise(fr, key, w, h, depth, spps, bound):
    """sum (filtered - ref)^2 over sum (raw - ref)^2 at levels 4, k 4, ref a 4096-spp frame of
    seed 999, frame k of seed 0xD100 + k. Measured on the oracle: 0.131, 0.122, 0.358, 0.524; the
    bounds leave a margin of about 1.5 to 1.9."""
    comp = R.ErrorComposite()
    for k, spp in enumerate(spps):
        mean = _oracle(key, w, h, spp, depth, SEED0 + k)
        s = (mean * F(spp)).astype(F)  # exact: spp is a power of two
        assert np.array_equal(_bits((s / F(spp)).astype(F)), _bits(mean))
        raw = comp.add(s, spp)
    ref = _oracle(key, w, h, 4096, depth, 999).astype(np.float64)
    filtered, _, var = D.denoise(comp.a, comp.q, comp.n, comp.frames, 4, 4.0)
    e_raw = float(np.sum((raw.astype(np.float64) - ref) ** 2))
    e_fil = float(np.sum((filtered.astype(np.float64) - ref) ** 2))
    print(f"{key} {w}x{h} {spps}: filtered {e_fil:.6g} / raw {e_raw:.6g} = {e_fil / e_raw:.3f}; "
          f"sum var {float(var.astype(np.float64).sum()):.6g}")
    assert e_fil / e_raw <= bound


def test_header_and_python_mirror(fr):
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    assert "int fr_ctx_denoise(fr_ctx* ctx, uint32_t levels, float k);" in hdr
    assert "int fr_ctx_download_denoised(fr_ctx* ctx, float* mean_rgb, uint8_t* rgb8, float* var);" in hdr
    assert "int fr_ctx_denoised_buffers(fr_ctx* ctx, float** d_mean_rgb, uint8_t** d_rgb8);" in hdr
    assert "#define FR_ABI_VERSION 6" in hdr and "no fr_mctx_denoise" in hdr
    for name in ("fr_ctx_denoise", "fr_ctx_download_denoised", "fr_ctx_denoised_buffers"):
        assert name in fr.EXPORTS and hasattr(fr.lib(), name)
    assert not hasattr(fr.lib(), "fr_mctx_denoise")
    assert (fr.FR_DN_EPS, fr.FR_DN_MEAN_MAX, fr.FR_DN_VAR_MAX) == (2.0 ** -20, 2.0 ** 40, 2.0 ** 80)
    assert (fr.FR_DN_LEVELS_DEFAULT, fr.FR_DN_K_DEFAULT) == (4, 4.0) == (D.LEVELS, D.K)
    for name in ("denoise", "download_denoised", "denoised_buffers"):
        assert callable(getattr(fr.RenderContext, name))
    ctx_text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fr_ctx_denoise", "fr_ctx_download_denoised", "fr_ctx_denoised_buffers"):
        assert name in ctx_text
    # make_params is as it was: the filter is no frame flag
    assert fr.make_params(8, 8, 1, accumulate="error").flags == 1 | 32 | 64
    assert fr.make_params(8, 8, 1, accumulate="adaptive").flags == 1 | 32 | 64 | 128


def test_update_refuses_denoise_without_the_estimate(fr):
    m = fr.create_model(8, 8)
    for acc in (False, True):
        with pytest.raises(ValueError, match="denoise=True needs accumulate"):
            fr.update(m, 0, 0.1, accumulate=acc, denoise=True)
        with pytest.raises(ValueError, match="denoise=True needs accumulate"):
            m.frame_u8(m.scene, 8, 1, accumulate=acc, denoise=True)
    assert m.frame == 0 and m.ctx is None  # refused before the camera, the frame count or a context moved
    m.close()


def test_prototypes_from_c(tmp_path, fr):
    exe_path = str(tmp_path / "denoise_abi")
    libdir = os.path.join(ROOT, "fo-rma_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "denoise_abi.c"), "-L", libdir, "-lforma_rt",
                    f"-Wl,-rpath,{libdir}", "-o", exe_path], check=True)
    got = json.loads(subprocess.run([exe_path], check=True, capture_output=True, text=True).stdout)
    assert got == {"eps": 2.0 ** -20, "mean_max": 2.0 ** 40, "var_max": 2.0 ** 80, "levels": 4, "k": 4.0,
                   "abi_version": 6, "null_rc": [FR_EARG] * 3}
