#!/usr/bin/env python3
"""The sweep behind fr_ctx_temporal's defaults: the numpy restatement
(tests/temporal_ref.py) over the quality rows of tests/test_temporal_host.py: two 4-spp frames of
V0, one of V1, against a 4096-spp frame of V1. Prints one line per option set: the score (the mean
over the rows of log(ratio at levels 0) + log(ratio at levels 4), unguided), the options and each
row's two ratios, then the sets sorted by score. No device is needed; the oracle library is.

    python3 tools/temporal_sweep.py [--quick]"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fo-rma_amd")]
from tests.test_temporal_host import quality  # noqa: E402

ROWS = ("spheres", "spheres_down", "boxes", "scene_01", "metal_near")
F = np.float32


def main():
    quick = "--quick" in sys.argv
    n_max = (32.0,) if quick else (8.0, 16.0, 32.0, 64.0)
    spec = (0.0, 2.0, 4.0, 8.0, 32.0)
    sigma_z = (2.0 ** -5,) if quick else (2.0 ** -7, 2.0 ** -5, 2.0 ** -3)
    normal_min = (float(F(0.9)),) if quick else (0.5, float(F(0.9)), float(F(0.98)))
    out = []
    print("score n_max n_max_specular sigma_z normal_min " + " ".join(ROWS))
    for a, b, c, d in itertools.product(n_max, spec, sigma_z, normal_min):
        opt = dict(n_max=a, n_max_specular=b, sigma_z=c, normal_min=d)
        rs = [quality(name, False, opt) for name in ROWS]
        score = float(np.mean([np.log(r[0]) + np.log(r[1]) for r in rs]))
        line = "%.4f %g %g %g %.2f " % (score, a, b, c, d) + " ".join("%.3f/%.3f" % tuple(r) for r in rs)
        out.append((score, line))
        print(line, flush=True)
    print("sorted:")
    for _, line in sorted(out)[:12]:
        print(line)


if __name__ == "__main__":
    main()
