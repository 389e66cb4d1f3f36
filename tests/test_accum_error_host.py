"""The error estimate of progressive accumulation (FR_FLAG_ACCUM_ERROR) without a device.

- The flag never enters the frame plan (tests/c/plan_check.cpp prints the plan).
- tests/c/accum_error_check.cpp, a CPU program built with -fsanitize=address,undefined
  -fno-sanitize-recover=all -ffp-contract=off, walks the continue / restart decision with the
  flag on and off and runs the arithmetic the kernels compile (fo-rma_amd/csrc/accum_error.h) on
  a table of inputs; the numpy f32 restatement the GPU tests rely on (tests/accum_error_ref.py)
  must equal its bits.
- tests/c/accum_error_abi.c pins fr_accum_error's layout from C.
- The estimator itself, on oracle frames only: the summed estimated variance of the mean
  predicts the real squared error against a 4096-spp frame."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from tests import accum_error_ref as R
from tests.test_plan import HEADLINE, MIXED, ROOT, SMALL, SPHERES_10K, _plan, _run, exe  # noqa: F401 (exe: fixture)

F = np.float32
FR_EARG = -1
ACCUMULATE, ACCUM_ERROR, SCENE_JIT, WRITE_U8 = 32, 64, 4, 1


@pytest.mark.parametrize("case", ["headline", "small_spp3", "mixed", "bvh", "shard", "streamed"])
def test_the_flags_never_reach_the_plan(exe, case):
    kv = {"headline": HEADLINE, "small_spp3": dict(SMALL, spp=3), "mixed": MIXED, "bvh": SPHERES_10K,
          "shard": dict(HEADLINE, shard="0/8"), "streamed": dict(HEADLINE, prev_in_flight=1)}[case]
    for base in (0, SCENE_JIT, WRITE_U8 | SCENE_JIT):
        plain = _plan(exe, **dict(kv, flags=base))
        err = _plan(exe, **dict(kv, flags=base | ACCUMULATE | ACCUM_ERROR))
        assert plain["rc"] == 0 and err == plain, base  # every printed field, kp.flags and the kernel included
        assert err["flags"] & (ACCUMULATE | ACCUM_ERROR) == 0


def test_the_plan_check_refuses_the_flag_alone_and_with_spp_zero(exe):
    r = _plan(exe, **dict(SMALL, spp=3, flags=ACCUM_ERROR))
    assert r["rc"] == FR_EARG and "FR_FLAG_ACCUM_ERROR without FR_FLAG_ACCUMULATE" in r["error"]
    r = _plan(exe, **dict(SMALL, spp=0, flags=ACCUMULATE | ACCUM_ERROR))
    assert r["rc"] == FR_EARG and "FR_FLAG_ACCUM_ERROR with spp 0" in r["error"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("accum_error") / "accum_error_check")
    srcs = [os.path.join(ROOT, "tests", "c", "accum_error_check.cpp")] + [
        os.path.join(ROOT, "fo-rma_amd", "csrc", f)
        for f in ("plan.cpp", "pack.cpp", "json_min.cpp", "scene.cpp", "bvh.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), *srcs, "-o", out], check=True, timeout=600)
    return out


def _hex_rows(exe_path, mode, rows, tmp_path):
    """Runs the table mode on u32 rows; returns the printed bits as a uint32 array [rows, k]."""
    path = str(tmp_path / f"{mode}.bin")
    np.ascontiguousarray(rows, np.uint32).tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, mode, path], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return np.array([[int(w, 16) for w in line.split()] for line in p.stdout.splitlines()], np.uint32)


def test_continue_and_restart_with_the_flag(check):
    got = _run(check, "decision")  # exit status 0: every frame was accepted; clean sanitizer log
    steps = [(r["case"], r["start"], r["frames"], r["samples"], r["has_q"]) for r in got if "start" in r]
    assert steps == [
        ("on", 1, 1, 4, 1),
        ("on_again", 0, 2, 20, 1),  # another seed and spp: continues, Q goes on
        ("off", 1, 1, 16, 0),  # the flag off: a new accumulation without Q
        ("off_again", 0, 2, 32, 0),
        ("on_after_off", 1, 1, 16, 1),  # and on again: Q never misses a frame of its accumulation
        ("reset", 1, 1, 16, 1),
        ("on_again", 0, 2, 32, 1),
    ]
    by = {r["case"]: r for r in got}
    assert by["without_accumulate"]["rc"] == FR_EARG
    assert "FR_FLAG_ACCUM_ERROR without FR_FLAG_ACCUMULATE" in by["without_accumulate"]["error"]
    assert by["spp_zero"]["rc"] == FR_EARG and "FR_FLAG_ACCUM_ERROR with spp 0" in by["spp_zero"]["error"]
    assert by["spp_zero_plain_accumulate"]["rc"] == 0


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def test_q_update_bits_equal_the_numpy_restatement(check, tmp_path):
    rng = np.random.default_rng(0xE220)
    n = 4000
    s = (rng.random(n, dtype=F) * F(64.0)).astype(F)
    s[::7] = (s[::7] * F(1e-6)).astype(F)  # small sums: the square is far below the sum
    spp = rng.integers(1, 300, n).astype(np.uint32)
    q0 = (rng.random(n, dtype=F) * F(4096.0)).astype(F)
    edges = [(0.0, 1, 0.0), (0.0, 16, 3.5), (1.0, 3, 0.0), (3.0, 7, 1.0), (2.0 ** -80, 1, 0.0), (1e30, 1, 1.0),
             (np.inf, 4, 1.0), (np.nan, 4, 1.0), (5.0, 2 ** 24 + 1, 2.0)]
    s = np.concatenate([s, np.array([e[0] for e in edges], F)])
    spp = np.concatenate([spp, np.array([e[1] for e in edges], np.uint32)])
    q0 = np.concatenate([q0, np.array([e[2] for e in edges], F)])
    got = _hex_rows(check, "terms", np.stack([_bits(s), spp, _bits(q0)], 1), tmp_path)
    with np.errstate(all="ignore"):
        want_t = np.stack([R.sq_term(s[i], int(spp[i])) for i in range(len(s))]).astype(F)
        want_q = (q0 + want_t).astype(F)
    nan = np.isnan(want_t)
    assert np.array_equal(np.isnan(got[:, 0].view(F)), nan) and nan.sum() == 1
    assert np.array_equal(got[~nan, 0], _bits(want_t)[~nan])
    assert np.array_equal(got[~nan, 1], _bits(want_q)[~nan])


def _rel_table():
    """(A [k, 3], Q [k, 3], n [k], K [k]) and the indices of the named edges."""
    rng = np.random.default_rng(0xE221)
    a_rows, q_rows, n_rows, k_rows = [], [], [], []
    for _ in range(3000):  # accumulations of K random frames: A and Q as the resolve builds them
        k = int(rng.integers(2, 12))
        comp = R.ErrorComposite()
        base = rng.random(3, dtype=F) * F(rng.choice([1e-3, 0.05, 1.0, 40.0]))
        for _ in range(k):
            spp = int(rng.choice([1, 2, 3, 4, 16, 37, 256]))
            noise = F(1.0) + (rng.random(3, dtype=F) - F(0.5)) * F(rng.choice([0.0, 1e-6, 0.02, 1.0]))
            comp.add((base * noise * F(spp)).astype(F), spp)
        a_rows.append(comp.a), q_rows.append(comp.q), n_rows.append(comp.n), k_rows.append(k)
    edges = {}

    def edge(name, a, q, n, k):
        edges[name] = len(a_rows)
        a_rows.append(np.array(a, F)), q_rows.append(np.array(q, F)), n_rows.append(n), k_rows.append(k)

    edge("clamps", (8.0, 8.0, 8.0), (3.0, 4.0, 3.9999), 16, 4)  # Q < A^2 / n = 4 in every channel but equal in one
    edge("one_channel_clamps", (8.0, 8.0, 8.0), (3.0, 5.0, 4.0), 16, 4)
    edge("a_zero", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 64, 4)
    edge("below_floor", (0.01, 0.01, 0.01), (0.001, 0.001, 0.001), 16, 4)  # mean sum 0.001875 < 2^-7
    edge("at_floor", (2.0 ** -5, 2.0 ** -5, 0.0), (0.01, 0.01, 0.0), 8, 2)  # mean sum exactly 2^-7
    edge("above_floor", (0.5, 0.25, 0.125), (0.1, 0.05, 0.02), 8, 3)
    edge("a_nan", (np.nan, 1.0, 1.0), (np.nan, 2.0, 2.0), 8, 2)
    edge("a_nan_all", (np.nan,) * 3, (np.nan,) * 3, 8, 2)
    edge("a_inf", (np.inf, 1.0, 1.0), (np.inf, 2.0, 2.0), 8, 2)
    edge("a_inf_all", (np.inf,) * 3, (np.inf,) * 3, 8, 2)
    edge("two_frames", (3.0, 2.0, 1.0), (5.0, 2.5, 0.75), 2, 2)
    edge("n_2p24_plus_1", (1.0e7, 2.0e7, 3.0e6), (6.5e6, 2.5e7, 6.0e5), 2 ** 24 + 1, 5)
    return np.stack(a_rows), np.stack(q_rows), np.array(n_rows, np.uint32), np.array(k_rows, np.uint32), edges


def test_rel_bits_equal_the_numpy_restatement(check, tmp_path):
    a, q, n, k, edges = _rel_table()
    got = _hex_rows(check, "rel", np.concatenate([_bits(a), _bits(q), n[:, None], k[:, None]], 1), tmp_path)[:, 0]
    want = np.array([R.rel_error(a[i], q[i], int(n[i]), int(k[i])) for i in range(len(n))], F)
    assert not np.isnan(want).any() and (want >= 0).all()  # never NaN, never negative: the bits order as uint32
    assert np.array_equal(got, _bits(want))
    rel = {name: float(want[i]) for name, i in edges.items()}
    assert rel["clamps"] == 0 and rel["a_zero"] == 0
    assert rel["one_channel_clamps"] > 0
    assert rel["a_nan"] == rel["a_nan_all"] == rel["a_inf"] == rel["a_inf_all"] == 0
    # at and below the floor the denominator is 2^-7 itself
    i = edges["at_floor"]
    m, v = R.variance(a[i], q[i], int(n[i]), int(k[i]))
    assert float((m[0] + m[1]) + m[2]) == 2.0 ** -7
    for name in ("below_floor", "at_floor"):
        i = edges[name]
        m, v = R.variance(a[i], q[i], int(n[i]), int(k[i]))
        err = np.sqrt(F(F(F(v[0] + v[1]) + v[2]) / F(n[i])))
        assert rel[name] == float(F(err / F(2.0 ** -7))) > 0, name
    assert rel["above_floor"] > 0 and rel["two_frames"] > 0 and rel["n_2p24_plus_1"] > 0
    assert np.count_nonzero(want[:3000] == 0) > 0 and np.count_nonzero(want[:3000] > 0) > 2000


def test_struct_layout_from_c(tmp_path, fr):
    import ctypes as C
    exe_path = str(tmp_path / "accum_error_abi")
    libdir = os.path.join(ROOT, "fo-rma_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "accum_error_abi.c"), "-L", libdir, "-lforma_rt",
                    f"-Wl,-rpath,{libdir}", "-o", exe_path], check=True)
    lay = json.loads(subprocess.run([exe_path], check=True, capture_output=True, text=True).stdout)
    assert lay["sizeof"] == 32 == C.sizeof(fr.FrAccumError)
    want = {"frames": [0, 4], "samples": [4, 4], "pixels": [8, 8], "converged": [16, 8], "max_rel": [24, 4],
            "threshold": [28, 4]}
    for name, (off, size) in want.items():
        assert lay[name] == [off, size], name
        field = getattr(fr.FrAccumError, name)
        assert (field.offset, field.size) == (off, size), name
    assert [f for f, _ in fr.FrAccumError._fields_] == list(want)
    assert lay["flag"] == 64 and lay["floor"] == 2.0 ** -7 and lay["abi_version"] == 6
    assert lay["null_rc"] == [FR_EARG] * 3


def test_python_mirror(fr):
    assert fr.FR_FLAG_ACCUM_ERROR == ACCUM_ERROR and fr.FR_ERR_FLOOR == 2.0 ** -7 and fr.FR_ABI_VERSION == 6
    assert fr.make_params(8, 8, 1).flags & (ACCUMULATE | ACCUM_ERROR) == 0
    assert fr.make_params(8, 8, 1, accumulate=True).flags & (ACCUMULATE | ACCUM_ERROR) == ACCUMULATE
    p = fr.make_params(8, 8, 1, accumulate="error", scene_jit="wait")
    assert p.flags == WRITE_U8 | SCENE_JIT | 8 | ACCUMULATE | ACCUM_ERROR
    hdr = open(os.path.join(ROOT, "include", "forma_rt.h")).read()
    assert "#define FR_FLAG_ACCUM_ERROR 64u" in hdr and "#define FR_ERR_FLOOR 0.0078125f" in hdr
    assert "#define FR_ABI_VERSION 6" in hdr
    for name in ("fr_ctx_accum_error", "fr_ctx_download_error", "fr_mctx_accum_error"):
        assert name in fr.EXPORTS and hasattr(fr.lib(), name)
    assert callable(fr.render_converged) and callable(fr.RenderContext.accum_error)
    assert callable(fr.MultiContext.accum_error)


# ---- the estimator, on oracle frames alone (this pins the definition, not the product) -------

@functools.lru_cache(maxsize=None)
def _oracle(key, w, h, spp, depth, seed):
    from oracle import oracle_py as O
    from oracle import scene_ref as S
    if key == "builtin0":
        prims, cam = S.BUILTIN[0](), O.camera_new(w, h)
    else:
        import forma_rt
        prims, (frm, at, vup, fov) = S.load_json(open(forma_rt.scene_path(key)).read())
        cam = O.camera_look(frm, at, vup, fov, 0.1, w, h)
    mean, _, _, rows = O.render(prims, cam, w, h, spp, depth, seed=seed, threads=8)
    assert rows == h and not np.isnan(mean).any()
    return mean


@pytest.mark.parametrize("key,w,h,depth,spps", [
    ("scene_08", 33, 17, 8, (16,) * 8),
    ("scene_08", 33, 17, 8, (1, 4, 16, 2, 8, 8)),
    ("builtin0", 32, 24, 50, (4,) * 8),
])
def test_the_estimate_predicts_the_real_squared_error(fr, key, w, h, depth, spps):
    """sum (mean - ref)^2 over sum v_c / n (1 + n / 4096), ref a 4096-spp frame of seed 999 (its
    own noise is the second term): within [0.5, 2]. Measured 0.92 to 1.08."""
    comp = R.ErrorComposite()
    for k, spp in enumerate(spps):
        mean = _oracle(key, w, h, spp, depth, 0xE220 + k)
        s = (mean * F(spp)).astype(F)  # exact: spp is a power of two
        assert np.array_equal(_bits((s / F(spp)).astype(F)), _bits(mean))
        got = comp.add(s, spp)
    ref = _oracle(key, w, h, 4096, depth, 999)
    _, v = R.variance(comp.a, comp.q, comp.n, comp.frames)
    actual = float(np.sum((got.astype(np.float64) - ref.astype(np.float64)) ** 2))
    predicted = float(np.sum(v.astype(np.float64) / comp.n * (1.0 + comp.n / 4096.0)))
    print(f"{key} {spps}: actual {actual:.6g} / predicted {predicted:.6g} = {actual / predicted:.3f}")
    assert 0.5 <= actual / predicted <= 2.0
