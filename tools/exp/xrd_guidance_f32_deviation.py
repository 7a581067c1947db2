"""Measure what float32 does to the XRD-guidance gradient: the numpy restatement (arreau_amd/diffusion/xrd_guidance.py: reference)
in its float32 mode -- the kernel's split of precisions and operation kinds, numpy's sine, cosine and exp -- against the same run
in float64, over every batch of tests/xrd_guidance_cases.py, on the CPU.  Per batch the largest |g_32 - g_64| over the crystal's
scale (its largest |g_64| component; for a single atom, whose g vanishes identically, the largest component of g_terms) goes into
xrd_guidance.F32_DEVIATION by hand; the tests allow the device G_F32_BOUND = xrd.BOUND_FACTOR = 16 times the largest of them.

    python tools/exp/xrd_guidance_f32_deviation.py [BATCH ...]

One JSON line per batch (with the smallest float64 distance of a crystal to its target, which the tests require to be at least
MIN_TEST_DISTANCE, and whether the integers of the two runs agree) and a last one in the form of the constant."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from arreau_amd.diffusion import xrd_guidance as xg  # noqa: E402
from tests import xrd_guidance_cases as cases  # noqa: E402


def deviation(bt, r64, r32):
    """The largest |g_32 - g_64| / scale over the guided crystals."""
    first = cases.offsets(bt)
    worst = 0.0
    for b in range(len(bt.counts)):
        if r64.flags[b]:
            continue
        a, e = first[b], first[b + 1]
        err = np.abs(r32.g[a:e].astype(np.float64) - r64.g[a:e]).max()
        worst = max(worst, float(err / xg.g_scale(r64.g[a:e], r64.g_terms[a:e])))
    return worst


def main():
    table = {}
    for name in sys.argv[1:] or cases.BATCHES:
        bt, r64 = cases.reference(name)
        r32 = xg.reference(bt.frac, bt.lattice, bt.counts, bt.weights, bt.target, bt.params, dtype=np.float32)
        same = bool(np.array_equal(r64.reflections, r32.reflections) and np.array_equal(r64.flags, r32.flags))
        table[name] = float(f"{deviation(bt, r64, r32):.3g}")
        print(json.dumps({"batch": name, "crystals": len(bt.counts), "deviation": table[name], "same_integers": same,
                          "smallest_distance": float(np.nanmin(r64.distance)), "largest_distance": float(np.nanmax(r64.distance)),
                          "flagged": int((r64.flags != 0).sum())}), flush=True)
    print(json.dumps({"F32_DEVIATION": table, "largest": max(table.values()), "bound_factor": xg.BOUND_FACTOR}), flush=True)


if __name__ == "__main__":
    main()
