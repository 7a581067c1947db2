"""Time the structure match's launch (arreau_structure_match) with device events: the final state of a B x n sample of a synthetic
model matched, paired, against a copy of itself whose atoms are displaced by a few hundredths of an A, and against itself.

    python tools/time_structure_match.py [--shapes 256x20] [--reps 30] [--warmup 5] [--assignment nearest|optimal]

The windows include the wrapper's output allocations and ctypes call, so they bound the kernel from above.  Prints one JSON line
per input: median / min / p90 in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.diffusion import structure_match as sm  # noqa: E402
from tools.time_symmetrize import sampled  # noqa: E402
from tools.time_uniqueness import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100, help="denoising steps of the sampled input")
    ap.add_argument("--assignment", choices=tuple(sm.ASSIGNMENTS), default="nearest", help="StructureMatchParams.assignment (rule 6b)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        x = sampled(B, n, dev, args.steps)
        g = torch.Generator().manual_seed(11)
        moved = (x[0] + 0.004 * torch.randn(x[0].shape, generator=g).to(dev)).contiguous()
        pairs = torch.as_tensor(sm.paired(B), device=dev)
        for name, y in (("displaced copy", (moved,) + tuple(x[1:])), ("itself", x)):
            p = sm.StructureMatchParams(assignment=args.assignment)
            out = {"input": f"sampled {shape} against {name}", "assignment": p.assignment, "ltol": p.ltol, "angle_tol": p.angle_tol, "stol": p.stol,
                   "match": timed(lambda: sm.match(x, y, pairs, p, stride=n), args.reps, args.warmup)}
            r = sm.result_to_numpy(sm.match(x, y, pairs, p, stride=n))
            out["matched"], out["flagged"] = int(r["matched"].sum()), int((r["flags"] != 0).sum())
            out["n_mappings_mean"], out["n_candidates_mean"] = float(r["n_mappings"].mean()), float(r["n_candidates"].mean())
            out["n_permutations_mean"], out["assigned"] = float(r["n_permutations"].mean()), int(((r["flags"] & sm.ASSIGNED) != 0).sum())
            out["no_permutation"] = int(((r["flags"] & sm.NO_PERMUTATION) != 0).sum())
            ok = r["matched"] == 1
            out["rms_mean"] = float(r["rms"][ok].mean()) if ok.any() else None
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
