"""Instruction and register budget of the headline trace kernel (the scene_08 scene-specialised
build), from the listing tools/isa_sections.py cuts into lane-loop regions. No GPU: hipcc
cross-compiles.

The lane loop is bound by instruction issue, vector and scalar: a change that
adds a register copy at a join or a mask operation to a guard costs the step time without
changing a result. profiles/r09a_c3_static.json is this tree's own table (`python
tools/isa_sections.py isa`; r09a_c3_static_parent.json is the same command on the commit before);
no region may issue more VALU or SALU instructions than it records, and the kernel keeps the
registers that let a sum wave run beside seven trace waves (§4.6). Counts only: the test looks for
no particular instruction."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = "/opt/rocm/bin/hipcc"  # tools/isa_sections.py's compiler
TABLE = os.path.join(ROOT, "profiles", "r09a_c3_static.json")
PARENT = os.path.join(ROOT, "profiles", "r09a_c3_static_parent.json")
PARENT_SGPR_SPILLS = 3
# regions outside the lane loop's steady state: set-up and tear-down, and the IEEE fallbacks no
# ordinary frame enters
OUTSIDE = ("PROLOGUE", "EPILOGUE", "RARE")


@pytest.fixture(scope="module")
def listing():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc absent")
    env = dict(os.environ)
    env.pop("ISA_NOMARKS", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_sections.py"), "isa"], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def test_registers(listing, fr):
    meta = listing["meta"]
    print(meta)
    assert meta["vgpr_count"] <= 56
    assert meta["vgpr_spill_count"] == 0
    assert meta["sgpr_spill_count"] <= PARENT_SGPR_SPILLS


def test_no_region_above_the_recorded_table(listing, fr):
    want = json.load(open(TABLE))["regions"]
    got = listing["regions"]
    assert set(got) <= set(want), sorted(set(got) - set(want))
    over = {name: (r["valu"], r["salu"], want[name]["valu"], want[name]["salu"]) for name, r in got.items()
            if r["valu"] > want[name]["valu"] or r["salu"] > want[name]["salu"]}
    print({name: (r["valu"], r["salu"]) for name, r in got.items()})
    assert not over, f"(valu, salu, recorded valu, recorded salu): {over}"


def test_recorded_table_is_below_the_parents():
    """The committed pair: the lane loop's regions together issue fewer VALU and fewer SALU
    instructions than the parent's, with no more registers."""
    tree, parent = json.load(open(TABLE)), json.load(open(PARENT))
    loop = lambda t, k: sum(r[k] for name, r in t["regions"].items() if name not in OUTSIDE)  # noqa: E731
    assert loop(tree, "valu") < loop(parent, "valu") and loop(tree, "salu") < loop(parent, "salu")
    assert tree["meta"]["vgpr_count"] <= parent["meta"]["vgpr_count"]
    assert tree["meta"]["sgpr_spill_count"] <= parent["meta"]["sgpr_spill_count"] == PARENT_SGPR_SPILLS
