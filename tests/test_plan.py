"""The frame plan and the scene packer without a device (fo-rma_amd/csrc/plan.cpp, pack.cpp):
tests/c/plan_check.cpp links them into one CPU program, built with
-fsanitize=address,undefined -fno-sanitize-recover=all like tests/test_host_sanitizers.py's,
and prints what they decide; the expectations below restate the driver's formulas
 for a 256-CU device with 256 GiB (a 32 GiB sample-buffer budget)."""
import glob
import importlib.util
import json
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCENES = sorted(glob.glob(os.path.join(ROOT, "fo-rma_amd", "scenes", "*.min.json")))
FR_EARG = -1
SPHERE, PLANE, AABB, OBB, STUB, TRIANGLE = range(6)
MT_BANDS = 2
KNOBS = ("FR_BVH", "FR_DEFER", "FR_MAT", "FR_PIPELINE", "FR_SAMPLE_BUFFER_GB", "FR_FRAME_PIPE", "FR_FRAME_SLOTS",
         "FR_FRAME_PIPE_RESERVE", "FR_SCENE_JIT", "FR_BVH_STAGE", "FR_MAX_WGS")


def _build_plan_check(out, defs=()):
    srcs = [os.path.join(ROOT, "tests", "c", "plan_check.cpp")] + [
        os.path.join(ROOT, "fo-rma_amd", "csrc", f) for f in ("plan.cpp", "pack.cpp", "json_min.cpp", "scene.cpp", "bvh.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", *defs,
                    "-I", os.path.join(ROOT, "include"), *srcs, "-o", out], check=True, timeout=600)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "plan_check")
    _build_plan_check(out)
    return out


def _run(exe, *args, env=None):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    base.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", **(env or {}))
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=base)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return [json.loads(line) for line in p.stdout.splitlines() if line.strip()]


def _plan(exe, env=None, **kv):
    (r,) = _run(exe, "plan", *[f"{k}={v}" for k, v in kv.items()], env=env)
    return r


def _kernel(*t):
    b = lambda v: "true" if v else "false"
    return f"fr::trace_kernel<{t[0]}, {b(t[1])}, {t[2]}, {t[3]}, {b(t[4])}, {b(t[5])}, {t[6]}, {t[7]}>"


# the issue's cases: six diffuse boxes (the headline scene), a 40-primitive mixed scene with a
# plane and a metal, 10,000 diffuse spheres with a BVH, 100 diffuse spheres without one
BOXES = dict(n=6, kinds=1 << AABB, diffuse=1)
HEADLINE = dict(w=1920, h=1080, spp=256, depth=8, **BOXES)
SMALL = dict(w=64, h=36, depth=8, **BOXES)
MIXED = dict(w=64, h=36, spp=20, depth=12, n=40, kinds=(1 << SPHERE) | (1 << AABB) | (1 << PLANE), has_plane=1,
             diffuse=0)
SPHERES_10K = dict(w=64, h=36, spp=20, depth=8, n=10000, kinds=1 << SPHERE, diffuse=1, bvh_ok=1, bvh_levels=14,
                   n_aclass=1)
SPHERES_100 = dict(w=33, h=17, spp=17, depth=8, n=100, kinds=1 << SPHERE, diffuse=1, bvh_ok=0, shard="1/2")


def test_headline_plan(exe):
    r = _plan(exe, **HEADLINE)
    assert (r["P"], r["nblocks"], r["nibble"], r["wps"]) == (2073600, 16, 1, 2)
    assert (r["per_block"], r["cap_blocks"], r["passes"]) == (265420800, 129, 1)
    assert (r["nfs"], r["overlap"], r["lds"]) == (2, 0, 8688)
    assert r["pass"] == [[0, 16, 39398400, 31104000, 15]]
    assert r["kernel"] == _kernel(1, 0, 9, 8, 0, 0, 2, 1)


def test_headline_shard_of_eight_overlaps_its_traces(exe):
    r = _plan(exe, shard="0/8", **HEADLINE)
    assert (r["P"], r["nfs"], r["overlap"]) == (261120, 2, 1)
    assert r["pass"][0][2:4] == [4961280, 3916800]


@pytest.mark.parametrize("pipeline", [None, "2"])
def test_sample_buffer_budget_splits_the_frame_into_passes(exe, pipeline):
    env = {"FR_SAMPLE_BUFFER_GB": "0.001"}
    if pipeline:
        env["FR_PIPELINE"] = pipeline
    r = _plan(exe, env=env, spp=100, **SMALL)
    assert (r["P"], r["nblocks"], r["cap_blocks"], r["nb_pass"], r["passes"], r["nfs"]) == (2560, 7, 3, 1, 7, 0)
    assert r["pass"][-1] == [6, 1, 2560, 0, 6]


def test_short_frame_needs_only_its_own_sample_slots(exe):
    r = _plan(exe, spp=3, **SMALL)
    assert (r["ks"], r["nblocks"], r["per_block"], r["passes"], r["nfs"]) == (3, 1, 61440, 1, 2)
    assert r["pass"] == [[0, 1, 2560, 2560, 0]]


def test_general_scene_keeps_the_unwind_in_the_trace_kernel(exe):
    r = _plan(exe, **MIXED)
    assert (r["defer"], r["wps"], r["lds"]) == (0, 3, 27792)
    assert r["pass"] == [[0, 2, 5120, 2560, 1]]
    assert r["kernel"] == _kernel(0, 1, 4, 0, 0, 0, 0, 0)


def test_bvh_scene_with_attenuation_classes_stores_records(exe):
    r = _plan(exe, **SPHERES_10K)
    assert (r["use_bvh"], r["defer"], r["nibble"], r["wps"], r["lds"], r["stage_bytes"]) == (1, 1, 1, 2, 23552, 0)
    assert r["kernel"] == _kernel(2, 0, 2, 8, 1, 0, 2, 1)


def test_bvh_scene_without_classes_stores_colours(exe):
    r = _plan(exe, **dict(SPHERES_10K, n_aclass=0))
    assert (r["defer"], r["wps"], r["lds"], r["stage_bytes"]) == (0, 3, 19456, 6144)
    assert r["kernel"] == _kernel(2, 0, 4, 8, 1, 0, 0, 1)


def test_mid_size_list_scene_stores_12_byte_records(exe):
    r = _plan(exe, **SPHERES_100)
    assert (r["P"], r["defer"], r["nibble"], r["wps"], r["lds"]) == (320, 1, 0, 3, 15952)
    assert r["pass"] == [[0, 2, 640, 320, 1]]
    assert r["kernel"] == _kernel(2, 0, 4, 8, 0, 0, 1, 1)


def test_knobs(exe):
    r = _plan(exe, env={"FR_DEFER": "0"}, **HEADLINE)
    assert r["kernel"] == _kernel(1, 0, 4, 8, 0, 0, 0, 1) and r["wps"] == 3
    r = _plan(exe, env={"FR_DEFER": "1"}, **HEADLINE)
    assert r["targs"][6] == 1 and r["wps"] == 3
    assert _plan(exe, env={"FR_MAT": "0"}, **HEADLINE)["targs"][7] == 0
    r = _plan(exe, env={"FR_BVH": "0"}, **SPHERES_10K)
    assert r["use_bvh"] == 0 and r["targs"][4] == 0
    r = _plan(exe, **dict(MIXED, depth=8, flags=MT_BANDS))
    assert r["kernel"] == _kernel(0, 1, 4, 8, 0, 1, 0, 0) and (r["use_bvh"], r["defer"]) == (0, 0)
    assert _plan(exe, env={"FR_FRAME_PIPE": "0"}, **HEADLINE)["nfs"] == 0
    assert _plan(exe, env={"FR_FRAME_SLOTS": "3"}, spp=3, **SMALL)["nfs"] == 3
    # the grid's knobs travel with the plan; history decides the reserve
    r = _plan(exe, env={"FR_MAX_WGS": "5", "FR_BVH_STAGE": "2"}, **HEADLINE)
    assert (r["max_wgs"], r["bvh_stage"], r["reserve"]) == (5, 2, 0)
    assert _plan(exe, prev_in_flight=1, **HEADLINE)["reserve"] == 1
    assert _plan(exe, streaming=1, shard="0/8", **HEADLINE)["reserve"] == 4
    assert _plan(exe, env={"FR_FRAME_PIPE_RESERVE": "2"}, **HEADLINE)["reserve"] == 2


def test_select_kernel_reaches_exactly_the_sixty_compiled_specialisations(exe):
    res = _run(exe, "kernels")
    ids = res[:-1]
    assert res[-1]["distinct"] == len(ids) == 60 and res[-1]["inputs"] == 7 * 2 * 2 * 2 * 16
    pat = re.compile(r"^fr::trace_kernel<\d+, (true|false), \d+, \d+, (true|false), (true|false), \d+, \d+>$")
    for r in ids:
        assert pat.match(r["kernel"]), r
        assert r["kernel"] == _kernel(*r["targs"])
    assert len({tuple(r["targs"]) for r in ids}) == 60


def test_item_range(exe):
    """kItemLimit = 2^32 - 1 - 2^28 items per pass; a frame of more than one block runs its last
    block as up to 4 sub-blocks, so its shard may hold floor(kItemLimit / 4) pixel slots:
    3839 strips of a 32768-wide image (262,144 slots each), not 3840."""
    limit = 0xFFFFFFFF - (1 << 28)
    r = _plan(exe, w=32768, h=3840 * 8, spp=32, n=6)
    assert r["rc"] == FR_EARG
    assert r["error"] == ("shard of 1006632960 pixel slots exceeds the 32-bit work-item range at spp 32; "
                          "use more shards")
    r = _plan(exe, w=32768, h=3839 * 8, spp=32, n=6)
    assert r["rc"] == 0 and r["P"] == 3839 * 262144 and limit // r["P"] == 4
    assert max(p[2] for p in r["pass"]) == 4 * r["P"] <= limit
    # one block: no sub-blocks, every shard an image can have fits
    assert _plan(exe, w=32768, h=65528, spp=16, n=6)["rc"] == 0


@pytest.mark.parametrize("height", [1, 7, 8, 9, 17, 1080])
@pytest.mark.parametrize("count", [1, 2, 3, 8])
def test_strip_geometry(exe, height, count):
    res = _run(exe, "strips", str(height), str(count))
    assert len(res) == 2 * count
    owner = [(y // 8) % count for y in range(height)]  # strips of 8 rows, dealt round robin
    for r in res:
        rows = [y for y in range(height) if owner[y] == r["shard"]]
        strips = sorted({y // 8 for y in rows})
        assert r["strips"] == (height + 7) // 8 and r["count"] == len(strips) and r["rows"] == len(rows)
        mt_end = 4 * (height // 4) if r["mt"] else height
        assert r["traced_rows"] == sum(1 for y in rows if y < mt_end)
        full = [k for k in strips if (k + 1) * 8 <= height]
        assert r["full"] == len(full) and r["has_partial"] == (len(full) != len(strips))
        if r["has_partial"]:
            assert r["partial"] == strips[-1]
    for mt in (0, 1):
        assert sum(r["rows"] for r in res if r["mt"] == mt) == height  # the shards' rows partition [0, H)
    assert sum(r["traced_rows"] for r in res if r["mt"] == 1) == 4 * (height // 4)


def _facts(prims):
    """n_aclass, diffuse, att_nonneg from the primitive list [kind, material, colour bits]."""
    one = struct.unpack("<I", struct.pack("<f", 1.0))[0]
    classes, ok, diffuse, nonneg = [], True, True, True
    for kind, material, *col in prims:
        if kind == STUB:
            cls = "none"
        elif kind == PLANE:
            cls = "metal" if material == 1 else "lambert"
        else:
            cls = {1: "metal", 2: "dielectric", 3: "light"}.get(material, "lambert")
        diffuse &= cls not in ("metal", "dielectric")
        att = (one, one, one) if cls == "light" else tuple(col)
        if att not in classes:
            if len(classes) < 15:
                classes.append(att)
            else:
                ok = False
        nonneg &= all(b < 0x7F800000 for b in att)  # sign clear, finite
    return (len(classes) if ok and prims else 0), diffuse, nonneg


def test_packed_scenes(exe, tmp_path):
    spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(ROOT, "tools", "gen_scene.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    gen = tmp_path / "gen10k.json"
    gen.write_text(gs.dumps(gs.generator_scene(10000, "sphere")))
    res = _run(exe, "pack", *SCENES, "empty", str(gen))
    assert len(res) == len(SCENES) + 2
    unit = list(struct.unpack("<4I", struct.pack("<4f", 1.0, 1.0, 1.0, 0.0)))
    for r in res:
        offs = r["offsets"]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and r["bytes"] % 256 == 0, r["file"]
        assert all(a < b for a, b in zip(offs, offs[1:] + [r["bytes"]])), r["file"]
        assert r["n"] == len(r["prims"]) and r["att_n"] == unit, r["file"]
        assert r["rec_words"] == 16 * r["n"] and r["rec_words_equal_region"] == 1, r["file"]
        assert offs[4] - offs[3] >= 64 * max(r["n"], 1)  # the record region holds them
        n_aclass, diffuse, nonneg = _facts(r["prims"])
        assert (r["n_aclass"], r["diffuse"], r["att_nonneg"]) == (n_aclass, int(diffuse), int(nonneg)), r["file"]
        kinds = 0
        for p in r["prims"]:
            kinds |= 1 << (p[0] if p[0] <= TRIANGLE else STUB)
        assert r["kinds"] == kinds and r["has_plane"] == int(any(p[0] == PLANE for p in r["prims"])), r["file"]
    empty, gen10k = res[-2], res[-1]
    assert empty["n"] == 0 and empty["rec0_kind"] == STUB and empty["n_aclass"] == 0
    assert gen10k["n"] == 10000 and gen10k["bvh_ok"] == 1 and gen10k["n_segs"] >= 1 and gen10k["bvh_levels"] <= 16


# ---- the tuning table (fo-rma_amd/csrc/tuning.h) ------------------------------------------

CSRC = os.path.join(ROOT, "fo-rma_amd", "csrc")
# build macros and identifiers retired with the A/B alternatives they selected (profiles/AB_LOG.md
# keeps the measurements). FR_BVH_STAGE is not listed: the environment knob of that name stays.
RETIRED = ("FR_STAGE_SMAJOR FR_BVH_RSTAGE FR_TRACE_PRIO FR_CAM_RESIDENT FR_SPHERE_IEEE FR_SKY_IEEE FR_NO_UNROLL_NIB "
           "FR_BVH_SCALAR_NODES FR_BVH_SCALAR_LEAVES FR_JIT_PIN FR_JIT_GROUP FR_SKY_DEFER FR_STAGE FR_BLOCK_SAMPLES "
           "FR_FINE_SAMPLES FR_SUM_UNROLL_SKYD FR_SKY_SUM_IEEE FR_XOSHIRO_PLAIN FR_DIV_2STEP FR_BOX_FMA OR_BOX_FMA "
           "FR_SUM_PRIO FR_SUM_STUB FR_SUM_BUFLOAD FR_SUM_WAITFIX FR_SUM_DIRECT FR_SUM_THREADS FR_SUM_VGPRS "
           "FR_SETUP_ON_TRACE_STREAM FR_QUEUE_MEMSET FR_TAIL_PRIO FR_KLENS FR_KSCAT FR_OCCL_NEAR_FIRST kSkyDefer SKYD sky_dy RSTG SMAJ "
           "slot_at stage_base kStageSpansSub fine_item sum_kind jit_defines").split()
TEXT = (".h", ".hip", ".cpp", ".py", ".sh", ".md", ".txt", ".json", ".inc")


def _tuning_header():
    """tuning.h's defaults {name: value text} in file order, and FR_TUNING's names in list order."""
    text = open(os.path.join(CSRC, "tuning.h")).read()
    defaults = re.findall(r"^#ifndef (FR_\w+)\n#define \1 (\S+)[^\n]*\n#endif$", text, re.M)
    assert len(defaults) == len(re.findall(r"^#\s*ifndef\b", text, re.M)), "an #ifndef that is not a default"
    (body,) = re.findall(r"^#define FR_TUNING\(X\)((?:[^\n]*\\\n)*[^\n]*)$", text, re.M)
    return dict(defaults), [n for n, _ in defaults], re.findall(r"X\((\w+)\)", body)


def _default_value(defaults, name):
    v = defaults[name]
    return int(v) if re.fullmatch(r"\d+", v) else _default_value(defaults, v)  # (a default may name another knob)


def _source_files(*tops):
    for top in tops:
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("build", "_ref", "__pycache__", "sessions")]
            for f in files:
                if f.endswith(TEXT) or f == "Makefile":
                    yield os.path.join(d, f)


def test_tuning_table_names_every_default_once():
    defaults, order, listed = _tuning_header()
    assert len(order) == len(set(order))
    assert sorted(listed) == sorted(order) and len(listed) == len(set(listed))
    for path in _source_files(os.path.join("fo-rma_amd", "csrc")):
        if os.path.basename(path) != "tuning.h":
            assert "#ifndef FR_" not in open(path).read(), path


def test_retired_names_are_gone():
    pat = re.compile(r"\b(" + "|".join(RETIRED) + r")\b")
    for path in _source_files("fo-rma_amd", "oracle", "tools"):
        text = open(path, errors="replace").read()
        if path == os.path.join(CSRC, "plan.h"):  # FramePlan's one inert member (see its comment), nothing else
            text = text.replace("  int sum_kind = 0;\n", "", 1)
        m = pat.search(text)
        assert not m, (path, m.group(0))
    # ("pend" is also a word: only the kernel that held the variable is searched for it)
    assert not re.search(r"\bpend\b", open(os.path.join(CSRC, "trace_kernel.h")).read())


def _defines(exe):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    p = subprocess.run([exe, "tuning"], capture_output=True, text=True, timeout=600, env=base)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert all(re.fullmatch(r"#define FR_\w+ -?\d+", ln) for ln in lines), lines
    return [(ln.split()[1], int(ln.split()[2])) for ln in lines]


def test_tuning_defines_forward_every_default(exe):
    defaults, order, listed = _tuning_header()
    assert _defines(exe) == [(n, _default_value(defaults, n)) for n in listed]
    assert "sum_kind" not in _plan(exe, **HEADLINE)  # (left the printout with the 12-byte sky record)


def test_tuning_defines_forward_a_variant_builds_values(tmp_path):
    """One valued knob, one that was never forwarded, and the one that was a presence flag."""
    over = {"FR_KREJ_NIB": 7, "FR_BVH_WAVES": 6, "FR_MIN_WAVES": 5}
    out = str(tmp_path / "plan_check_variant")
    _build_plan_check(out, [f"-D{k}={v}" for k, v in over.items()])
    defaults, order, listed = _tuning_header()
    assert _defines(out) == [(n, over.get(n, _default_value(defaults, n))) for n in listed]

