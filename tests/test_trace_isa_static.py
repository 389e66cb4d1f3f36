"""Static checks of the headline trace kernel (the scene_08 scene-specialised build), from the
ISA listing tools/isa_sections.py cuts into regions. No GPU: hipcc cross-compiles.

The box tests of the unrolled list land in the region after the hit marker (SC_POSTHIT, 94 VALU
before scene_08's three symmetric slab pairs lost their v_min_f32 / v_max_f32; SC_HIT, the
segment's reciprocals in front of them, 15). The camera's short form and the slab shortcut must
cost no registers: seven trace waves per SIMD need <= 72 VGPRs, and the sum runs beside the trace
only while the kernel stays far below that (<= 56)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = "/opt/rocm/bin/hipcc"  # tools/isa_sections.py's compiler
PARENT_POSTHIT, PARENT_HIT = 94, 15


def _isa(nomarks):
    env = dict(os.environ)
    env.pop("ISA_NOMARKS", None)
    if nomarks:
        env["ISA_NOMARKS"] = "1"
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_sections.py"), "isa"], env=env,
                          capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc absent")
def test_scene08_kernel_box_region_and_registers(fr):
    out = _isa(False)
    assert out.returncode == 0, out.stderr[-2000:]
    tab = json.loads(out.stdout)
    regions, meta = tab["regions"], tab["meta"]
    print("regions", {k: v["valu"] for k, v in regions.items()}, "meta", meta)
    assert regions["SC_POSTHIT"]["valu"] <= PARENT_POSTHIT - 4
    assert regions["SC_POSTHIT"]["valu"] + regions["SC_HIT"]["valu"] <= PARENT_POSTHIT + PARENT_HIT - 4
    assert meta["vgpr_count"] <= 56 and meta["vgpr_spill_count"] == 0
    # the product kernel's own registers: the listing without the region markers (their asm
    # statements can move the allocation). The tool has no regions to cut there, so it may stop
    # after writing the listing: the listing is what is read.
    _isa(True)
    asm = os.path.join(ROOT, "fo-rma_amd", "build", "isa_jit", "scene08_kernel.s")
    text = open(asm).read()
    assert "FRSEC" not in text
    got = {k: int(text.split("." + k + ":")[1].split()[0]) for k in ("vgpr_count", "vgpr_spill_count")}
    print("without markers", got)
    assert got["vgpr_count"] <= 56 and got["vgpr_spill_count"] == 0
