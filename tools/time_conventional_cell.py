"""Time the conventional-cell launch (arreau_crystal_conventional, the reduced batch and the search's result handed in) with device
events, beside the symmetry search's launch on the same reduced batch, the reduction's launch and the whole chain
(conventional_cell.conventional_cell: reduce, gather, search, conventional), and beside a sample(find_symmetry=True) call with and
without conventional_cell=True: the final state of a B x n sample of a synthetic model and the ragged batch of known crystals the
tests use.

    python tools/time_conventional_cell.py [--shapes 256x20] [--reps 30] [--warmup 5]

The windows include the wrappers' output allocations and ctypes calls, so they bound the kernels from above.  Prints one JSON
line per input: median / min / p90 in microseconds (the sample() calls: milliseconds of wall time, median of 5)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.diffusion import cell_reduction as cr  # noqa: E402
from arreau_amd.diffusion import conventional_cell as cc  # noqa: E402
from arreau_amd.diffusion import symmetry_search as ss  # noqa: E402
from tools.time_symmetrize import sampled  # noqa: E402
from tools.time_uniqueness import timed  # noqa: E402


def known(dev):
    from tests import conventional_cell_cases as cases
    frac, lattice, counts, types = cases.gpu_batch()[2]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return tuple(torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (frac, lattice, off, types.astype(np.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100, help="denoising steps of the sampled input")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    p = cc.ConventionalCellParams()
    inputs = [("known 67 ragged", known(dev))]
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        inputs.append((f"sampled {shape}", sampled(B, n, dev, args.steps)))
    for name, (frac, lattice, off, types) in inputs:
        reduced = cr.reduce_cells(frac, lattice, off, types, p.reduction())
        batch = cc.reduced_batch(reduced)
        found = ss.find_symmetry(*batch, p.search())
        out = {"input": name, "symprec": p.symprec, "max_ops": p.max_ops,
               "conventional": timed(lambda: cc.conventional_stage(*batch, found), args.reps, args.warmup),
               "symmetry": timed(lambda: ss.find_symmetry(*batch, p.search()), args.reps, args.warmup),
               "reduce": timed(lambda: cr.reduce_cells(frac, lattice, off, types, p.reduction()), args.reps, args.warmup),
               "chain": timed(lambda: cc.conventional_cell(frac, lattice, off, types, p), args.reps, args.warmup)}
        r = cc.result_to_numpy(cc.conventional_stage(*batch, found))
        out["bravais"] = {k: v for k, v in cc.stats_of(r)["bravais"].items() if v}
        out["flagged"] = int((r["flags"] != 0).sum())
        print(json.dumps(out), flush=True)
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=12, seed=4321, num_timesteps=100).to(dev)
    for kw in (dict(find_symmetry=True), dict(find_symmetry=True, conventional_cell=True)):
        wall = []
        for _ in range(6):
            torch.manual_seed(3)
            np.random.seed(3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.sample(20, 256, seed=777, max_steps=args.steps, **kw)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"sample 256x20": sorted(kw), "steps": args.steps, "ms_median": float(np.median(wall[1:])), "ms_min": min(wall[1:])}), flush=True)


if __name__ == "__main__":
    main()
