"""Measure what float32 does to the Ewald sum: the numpy restatement (arreau_amd/diffusion/ewald.py: ewald_reference) in its float32
mode -- the kernel's split of precisions: the pair displacement, d2 and its cut, the reduced phase and its sine and cosine in
float32, everything else float64 -- against the same run in float64, over every batch of tests/ewald_cases.py, on the CPU.  Per
batch the larger of the energies' deviation (relative to |E_self|) and the potentials' (relative to K 2 alpha max|q| / sqrt(pi))
goes into ewald.F32_DEVIATION by hand; the tests allow the device ewald.BOUND_FACTOR = 16 times the largest of them.

    python tools/exp/ewald_f32_deviation.py [BATCH ...]

One JSON line per batch (with its smallest margins to the two cuts and whether the integers of the two runs agree) and a last one
in the form of the constant."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from arreau_amd.diffusion import ewald  # noqa: E402
from tests import ewald_cases as cases  # noqa: E402


def main():
    table = {}
    for name in sys.argv[1:] or cases.BATCHES:
        bt, r64 = cases.reference(name)
        r32 = cases.reference32(name)
        e_err, p_err = cases.deviation(r64, r32, bt)
        same = bool(np.array_equal(r64.n_pairs, r32.n_pairs) and np.array_equal(r64.n_reciprocal, r32.n_reciprocal) and np.array_equal(r64.flags, r32.flags))
        table[name] = float(f"{max(e_err, p_err):.3g}")
        margin = lambda a: float(np.nanmin(a)) if np.isfinite(a).any() else None
        print(json.dumps({"batch": name, "crystals": len(bt.counts), "energies": float(f"{e_err:.3g}"), "potentials": float(f"{p_err:.3g}"),
                          "same_integers": same, "reciprocal_margin": margin(r64.reciprocal_margin), "pair_margin": margin(r64.pair_margin),
                          "rounds": [int(r64.rounds.min()), int(r64.rounds.max())], "flags": sorted(set(r64.flags.tolist()))}), flush=True)
    print(json.dumps({"F32_DEVIATION": table, "largest": max(table.values()), "bound_factor": ewald.BOUND_FACTOR}), flush=True)


if __name__ == "__main__":
    main()
