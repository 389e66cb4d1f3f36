"""The segment's reciprocal guard and the box root selection without a device.

tests/c/guard_root_check.cpp, a CPU program built with -fsanitize=address,undefined
-fno-sanitize-recover=all -ffp-contract=off, compares rt_core.h's recip_box_ok3 and slab_root with
local copies of the per-component guard and of slab_root's expression over every combination of
the threshold values (its header lists them): the new guard never admits a segment the old one
refused, the fallback's clamped reciprocal has RN(1 / x)'s bits wherever the fast path is valid,
and the root selection's decision and t are those of the reference. It also counts where the
max(tn, t_min) < tf form of the geometric test, which was weighed and not taken, differs: exactly
the combinations with tn NaN and tf a number."""
import json
import os
import subprocess

import pytest

from tests.test_plan import ROOT


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("guard_root") / "guard_root_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math",
                    os.path.join(ROOT, "tests", "c", "guard_root_check.cpp"), "-o", out], check=True, timeout=600)
    return out


def _run(exe_path, args=()):
    """The stand-alone sanitizer program: it must end clean."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe_path, *args], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return p.stdout


def test_guard_is_conservative_and_root_selection_unchanged(check):
    got = json.loads(_run(check))
    print(got)
    assert got["triples"] == 28 ** 3 and got["roots"] == 12 ** 3
    # 10 of the 28 values pass the per-component guard; the sum test refuses some of their triples
    assert got["old_ok"] == 10 ** 3
    assert 0 < got["new_ok"] < got["old_ok"] and got["refused_more"] == got["old_ok"] - got["new_ok"]
    assert got["hits"] > 0
    # the form not taken: it hits where tn is NaN and tf lies in (t_min, t_max)
    assert got["max_form_differs"] > 0


def test_triples_listing_matches_numpy(check):
    """The program's triples and clamped reciprocals (what tests/test_recip_guard_gpu.py asks of the
    device) equal numpy's RN(1 / x) clamped to +-2^100."""
    import numpy as np

    from tests.recip_guard_fixtures import clamped_recip, triples
    rows = np.array([[int(t, 16) for t in ln.split()] for ln in _run(check, ["triples"]).splitlines()], np.uint32)
    d = triples()
    assert rows.shape == (len(d), 6)
    assert np.array_equal(rows[:, :3], d.view(np.uint32))
    assert np.array_equal(rows[:, 3:], clamped_recip(d).view(np.uint32))
