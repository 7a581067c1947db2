"""Time the symmetry search's launch (arreau_crystal_symmetry) with device events, beside the structural screen's launch on the
same inputs: random crystals at the sampler's density, B crystals of n atoms each, and 64 copies of the 64-atom 2x2x2 NaCl
supercell (the worst case of rule 3: the rarest species holds half the atoms, 48 rotations x 32 translations are all accepted).

    python tools/time_symmetry_search.py [--shapes 256x20,1024x64] [--species 2] [--reps 30] [--warmup 5]

The windows include the wrappers' output allocations and ctypes calls, so they bound the kernels from above.  Prints one JSON
line per input: median / min / p90 in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.diffusion import screening as sc  # noqa: E402
from arreau_amd.diffusion import symmetry_search as ss  # noqa: E402
from tools.time_uniqueness import batch, timed  # noqa: E402


def nacl_supercells(B):
    fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    cell = np.concatenate([fcc, np.mod(fcc + 0.5, 1.0)])
    shifts = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    frac = ((cell[None] + shifts[:, None]) / 2.0).reshape(-1, 3)
    types = np.tile([0] * 4 + [1] * 4, 8)
    n = frac.shape[0]
    return (np.tile(frac, (B, 1)).astype(np.float32), np.tile(np.eye(3, dtype=np.float32)[None] * 11.28, (B, 1, 1)),
            (np.arange(B + 1) * n).astype(np.int32), np.tile(types, B).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20,1024x64")
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
    p = ss.SymmetrySearchParams()
    for name, arrays in inputs:
        frac, lattice, off, types = (torch.as_tensor(v, device=dev) for v in arrays)
        out = {"input": name, "symprec": p.symprec,
               "symmetry": timed(lambda: ss.find_symmetry(frac, lattice, off, types, p), args.reps, args.warmup),
               "screen": timed(lambda: sc.screen(frac, lattice, off, types), args.reps, args.warmup)}
        r = ss.find_symmetry(frac, lattice, off, types, p)
        out["n_ops_max"], out["flagged"] = int(r["n_ops"].max()), int((r["flags"] != 0).sum())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
