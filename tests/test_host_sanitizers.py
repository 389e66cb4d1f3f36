"""Host sanitizer build: the product's JSON parser, scene builder, BVH builder
and scene-kernel cache reader (fo-rma_amd/csrc/json_min.cpp, scene.cpp, bvh.cpp,
jit_cache.cpp) and the oracle (oracle/oracle.cpp)
compiled with -fsanitize=address,undefined -fno-sanitize-recover=all into one CPU program
(tests/c/host_sanitize.cpp), then driven over every bundled scene, the generator's 10k-sphere
scene (BASELINE config C5), a malformed-JSON corpus and a 150k-sphere BVH build. Any
out-of-bounds access, use-after-free, leak or undefined behaviour aborts the program; every
malformed file must fail cleanly with FR_EPARSE (the reference unwrap()s and panics,
basics/scene_loader.rs:3-7)."""
import glob
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCENES = sorted(glob.glob(os.path.join(ROOT, "fo-rma_amd", "scenes", "*.min.json")))
FR_OK, FR_EARG, FR_EPARSE = 0, -1, -2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asan") / "host_sanitize")
    srcs = [os.path.join(ROOT, "tests", "c", "host_sanitize.cpp")] + [
        os.path.join(ROOT, "fo-rma_amd", "csrc", f) for f in ("json_min.cpp", "scene.cpp", "bvh.cpp", "jit_cache.cpp")] + [
        os.path.join(ROOT, "oracle", "oracle.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                    "-I", os.path.join(ROOT, "include"), *srcs, "-o", out], check=True, timeout=600)
    return out


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return [json.loads(line) for line in p.stdout.splitlines() if line.strip()]


def _malformed_corpus(dirpath):
    """Truncations, byte flips and hand-made bad documents around the bundled scenes."""
    base = open(os.path.join(ROOT, "fo-rma_amd", "scenes", "scene_01.min.json"), "rb").read()
    small = open(os.path.join(ROOT, "fo-rma_amd", "scenes", "scene_08.min.json"), "rb").read()
    docs = {}
    for k, cut in enumerate(sorted({1, 2, 10, 57, 200, len(base) // 3, len(base) // 2, len(base) - 2, len(base) - 1})):
        docs[f"trunc_{k}"] = base[:cut]
    rng = random.Random(5)
    for k in range(40):
        b = bytearray(small)
        for _ in range(1 + k % 4):
            b[rng.randrange(len(b))] = rng.choice(b'{}[],:"0-.eE+ \\tx\x00\xff')
        docs[f"flip_{k}"] = bytes(b)
    hand = {
        "empty": b"",
        "null": b"null",
        "number": b"42",
        "deep": b"[" * 300 + b"]" * 300,
        "deep_obj": b'{"a":' * 300 + b"1" + b"}" * 300,
        "huge_number": b'{"camera":{"position":[1e999,0,0],"rotation":[0,0,0,1],"fov":60},"objects":[]}',
        "bad_escape": b'{"camera":{"position":[0,0,0],"rotation":[0,0,0,1],"fov":60},"objects":[{"mesh":"\\uZZZZ"}]}',
        "string_pos": b'{"camera":{"position":"x","rotation":[0,0,0,1],"fov":60},"objects":[]}',
        "short_vec": b'{"camera":{"position":[0,0],"rotation":[0,0,0,1],"fov":60},"objects":[]}',
        "obj_not_list": b'{"camera":{"position":[0,0,0],"rotation":[0,0,0,1],"fov":60},"objects":7}',
        "missing_camera": b'{"objects":[]}',
        "unterminated": b'{"camera":{"position":[0,0,0',
        "trailing": small + b"}}}",
        "nul_inside": small[:40] + b"\x00" + small[41:],
        "long_string": b'{"camera":{"position":[0,0,0],"rotation":[0,0,0,1],"fov":60},"objects":[{"mesh":"'
                       + b"q" * 100000 + b'"}]}',
        "many_objects_bad_tail": b'{"camera":{"position":[0,0,0],"rotation":[0,0,0,1],"fov":60},"objects":['
                                 + b'{"mesh":"sphere","position":[0,0,0],"rotation":[0,0,0,1],"scale":[1,1,1]},' * 500
                                 + b"]",
    }
    docs.update(hand)
    paths = []
    for name, data in docs.items():
        p = os.path.join(dirpath, f"{name}.json")
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    return paths


def test_bundled_scenes_load_clean_and_match_the_product_library(exe, fr):
    res = _run(exe, "json", *SCENES)
    assert [r["rc"] for r in res] == [FR_OK] * len(SCENES)
    for r, path in zip(res, SCENES):
        assert r["prims"] == len(fr.Scene.from_file(path, 32, 18)), path  # the product library's own build
        assert r["oracle_rows"] == 18


def test_generator_scene_bvh_build_clean(exe, tmp_path):
    """BASELINE config C5's scene: tools/gen_scene.py's 10k spheres through the loader and the
    BVH builder (and a tiny oracle render over the brute-force list)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(ROOT, "tools", "gen_scene.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    p = tmp_path / "gen10k.json"
    p.write_text(gs.dumps(gs.generator_scene(10000, "sphere")))
    (r,) = _run(exe, "json", str(p))
    assert r["rc"] == FR_OK and r["prims"] == 10000
    assert r["bvh"]["ok"] == 1 and r["bvh"]["order"] == 10000
    # the full-sweep SAH tree (bvh.cpp): internal nodes below the stack's 16 levels (the
    # launch sizes its LDS stack to depth + 1 levels), leaves of at most 4 spheres
    assert r["bvh"]["depth"] < 16 and 10000 / 4 - 1 <= r["bvh"]["nodes"] < 10000
    # the tree the C5 timings were taken on (round 5's sort-per-node builder built the same
    # bytes: nodes, leaf order, segments); a builder change that moves it shows here. Re-pinned
    # (from 74bc9267b6b5e9e6) when spheres came to be bounded by bvh_sphere_bound: wider boxes, and
    # the splits that follow from them
    assert r["bvh"]["digest"] == "3ef837e2547dc637", r["bvh"]


# forced trees of the bundled scenes (fnv-1a over nodes, leaf order and segments), equal for
# round 5's builder (sorting every node's items per axis) and round 6's (presorted orders).
# scene_01 and scene_05, the two with spheres, were re-pinned (from db0be86289f89f8d and
# 8ee866288e39c8d0) when a sphere's bounds became bvh_sphere_bound's; the others did not move.
BUNDLED_TREE_DIGESTS = {
    "scene_01": "bca0bc7a13e0e1ba", "scene_02": "9402547a91b47399", "scene_03": "346a873c38c9159b",
    "scene_04": "51895897d1998ae2", "scene_05": "38c997c4c743a5c8", "scene_06": "191d4432c7c74f33",
    "scene_08": "3a4d7944ad02b602", "scene_09": "6f417d5af3a20a2f",
}


def test_bvh_trees_of_bundled_scenes_are_pinned(exe):
    res = _run(exe, "json", *[p for p in SCENES if os.path.basename(p)[:8] in BUNDLED_TREE_DIGESTS])
    assert len(res) == len(BUNDLED_TREE_DIGESTS)
    for r in res:
        name = os.path.basename(r["file"])[:8]
        assert r["bvh_forced"]["digest"] == BUNDLED_TREE_DIGESTS[name], (name, r["bvh_forced"])


def test_degenerate_bvh_inputs_build_clean(exe, tmp_path):
    """The full-sweep SAH builder on degenerate lists: 200 identical spheres (every centroid
    and box equal: no split separates, median splits by list order), and 200 spheres on one
    line (one axis with extent, two without). Builds clean, every primitive in the leaf
    order once, internal nodes below the 16 stack levels."""
    import copy
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_scene", os.path.join(ROOT, "tools", "gen_scene.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    base = json.loads(gs.dumps(gs.generator_scene(200, "sphere")))
    paths = []
    for name, pos in (("same", lambda i: (1.0, 2.0, 3.0)), ("line", lambda i: (0.25 * i, 0.0, 0.0))):
        d = copy.deepcopy(base)
        for i, o in enumerate(d["objects"]):
            o["position"] = dict(zip("xyz", pos(i)))
        p = tmp_path / f"{name}.json"
        p.write_text(json.dumps(d))
        paths.append(str(p))
    for r in _run(exe, "json", *paths):
        assert r["rc"] == FR_OK and r["prims"] == 200, r
        assert r["bvh"]["ok"] == 1 and r["bvh"]["order"] == 200 and r["bvh"]["depth"] < 16, r


def test_malformed_json_corpus_fails_cleanly(exe, tmp_path):
    paths = _malformed_corpus(str(tmp_path))
    res = _run(exe, "json", *paths)
    assert len(res) == len(paths)
    by = {os.path.basename(r["file"])[:-5]: r for r in res}
    for name in ("empty", "null", "number", "deep", "deep_obj", "unterminated", "trailing", "string_pos",
                 "short_vec", "obj_not_list", "many_objects_bad_tail", "bad_escape"):
        assert by[name]["rc"] == FR_EPARSE, (name, by[name])
    for r in res:
        assert r["rc"] in (FR_OK, FR_EPARSE), r


def test_150k_sphere_bvh_build_clean(exe):
    (r,) = _run(exe, "spheres", "150000")
    assert r["rc"] == FR_OK and r["bvh"]["ok"] == 1 and r["bvh"]["order"] == 150000


def test_cache_file_reader_rejects_damaged_files_cleanly(exe, tmp_path):
    """The scene kernel's disk-cache reader (jit_cache.cpp read_cached_code): the HIP loader
    aborts the process on a damaged code object, so nothing reaches it unless the 32-B
    header's magic, format, size and hash check out. A valid file round-trips; truncations,
    byte flips in header and body, a wrong size field (too small, too large, 2^63), a wrong
    magic or format, garbage, an empty file, a header alone, a directory and a missing file
    are refused without a sanitizer report, and a refused file is removed."""
    import struct
    good = tmp_path / "good.hsaco"
    subprocess.run([exe, "wrap", "5000", str(good)], check=True, timeout=60)
    raw = good.read_bytes()
    assert len(raw) == 5032
    bad = {
        "empty": b"",
        "header_only": raw[:32],
        "garbage": bytes(random.Random(3).randrange(256) for _ in range(4000)),
        "bad_magic": b"XRJC" + raw[4:],
        "bad_format": raw[:4] + struct.pack("<I", 2) + raw[8:],
        "size_small": raw[:8] + struct.pack("<Q", 4999) + raw[16:],
        "size_large": raw[:8] + struct.pack("<Q", 5001) + raw[16:],
        "size_huge": raw[:8] + struct.pack("<Q", 1 << 63) + raw[16:],
        "hash_flip": raw[:20] + bytes([raw[20] ^ 1]) + raw[21:],
        "body_flip": raw[:1000] + bytes([raw[1000] ^ 0x80]) + raw[1001:],
        "extra_byte": raw + b"\0",
    }
    for k, cut in enumerate((1, 31, 33, 100, len(raw) // 2, len(raw) - 1)):
        bad[f"trunc_{k}"] = raw[:cut]
    paths = []
    for name, data in bad.items():
        p = tmp_path / f"{name}.hsaco"
        p.write_bytes(data)
        paths.append(str(p))
    (tmp_path / "a_directory.hsaco").mkdir()
    paths += [str(tmp_path / "a_directory.hsaco"), str(tmp_path / "missing.hsaco")]
    res = _run(exe, "cache", str(good), *paths)
    assert res[0]["ok"] == 1 and res[0]["code_bytes"] == 5000 and res[0]["rewrap_equal"] == 1
    for r in res[1:]:
        assert r["ok"] == 0, r
    for name in bad:
        assert not (tmp_path / f"{name}.hsaco").exists(), name  # refused files are removed
    assert (tmp_path / "a_directory.hsaco").is_dir()  # (a directory is not a file to remove)
