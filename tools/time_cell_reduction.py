"""Time the cell reduction's launch (arreau_crystal_reduce) with device events, beside the symmetry search's launch on the same
inputs: random crystals at the sampler's density, B crystals of n atoms each, and 64 copies of the 64-atom 2x2x2 NaCl supercell
(32 translations, the closure test and the class search at their widest).

    python tools/time_cell_reduction.py [--shapes 256x20] [--species 2] [--reps 30] [--warmup 5]

The windows include the wrappers' output allocations and ctypes calls, so they bound the kernels from above.  Prints one JSON
line per input: median / min / p90 in microseconds."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.diffusion import cell_reduction as cr  # noqa: E402
from arreau_amd.diffusion import symmetry_search as ss  # noqa: E402
from tools.time_symmetry_search import nacl_supercells  # noqa: E402
from tools.time_uniqueness import batch, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20")
    ap.add_argument("--species", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    inputs = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        inputs.append((f"random {shape}", batch(B, n, args.species)))
    inputs.append(("NaCl 2x2x2 64x64", nacl_supercells(64)))
    p, q = cr.CellReductionParams(), ss.SymmetrySearchParams()
    for name, arrays in inputs:
        frac, lattice, off, types = (torch.as_tensor(v, device=dev) for v in arrays)
        out = {"input": name, "symprec": p.symprec,
               "reduce": timed(lambda: cr.reduce_cells(frac, lattice, off, types, p), args.reps, args.warmup),
               "symmetry": timed(lambda: ss.find_symmetry(frac, lattice, off, types, q), args.reps, args.warmup)}
        r = cr.reduce_cells(frac, lattice, off, types, p)
        out["multiplicity_max"], out["flagged"] = int(r["multiplicity"].max()), int((r["flags"] != 0).sum())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
