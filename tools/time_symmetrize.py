"""Time the symmetrization's launch (arreau_crystal_symmetrize, the search's result handed in) with device events, beside the
symmetry search's launch on the same inputs: the final state of a B x n sample of a synthetic model, random crystals at the
sampler's density, and 64 copies of the 64-atom 2x2x2 NaCl supercell with max_ops = 1536 (1536 operations each: the partner
search and the checks at their widest).

    python tools/time_symmetrize.py [--shapes 256x20] [--species 2] [--reps 30] [--warmup 5]

The windows include the wrappers' output allocations and ctypes calls, so they bound the kernels from above.  Prints one JSON
line per input: median / min / p90 in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.diffusion import crystal_batch as cb  # noqa: E402
from arreau_amd.diffusion import symmetrize as sz  # noqa: E402
from arreau_amd.diffusion import symmetry_search as ss  # noqa: E402
from tools.time_symmetry_search import nacl_supercells  # noqa: E402
from tools.time_uniqueness import batch, timed  # noqa: E402


def sampled(B, n, dev, steps):
    """The final state of a B x n sample of the synthetic model the tests use, as the device batch the instruments take."""
    from arreau_amd.checkpoint import make_synthetic_model
    torch.manual_seed(3)
    np.random.seed(3)
    res = make_synthetic_model(S=12, seed=4321, num_timesteps=100).to(dev).sample(n, B, seed=777, max_steps=steps)
    return cb.upload(res, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20")
    ap.add_argument("--species", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100, help="denoising steps of the sampled input")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    inputs = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        inputs.append((f"sampled {shape}", sampled(B, n, dev, args.steps), sz.SymmetrizeParams()))
        inputs.append((f"random {shape}", tuple(torch.as_tensor(v, device=dev) for v in batch(B, n, args.species)), sz.SymmetrizeParams()))
    inputs.append(("NaCl 2x2x2 64x64", tuple(torch.as_tensor(v, device=dev) for v in nacl_supercells(64)), sz.SymmetrizeParams(max_ops=1536)))
    for name, (frac, lattice, off, types), p in inputs:
        found = ss.find_symmetry(frac, lattice, off, types, p.search())
        out = {"input": name, "symprec": p.symprec, "max_ops": p.max_ops,
               "symmetrize": timed(lambda: sz.symmetrize(frac, lattice, off, types, p, found), args.reps, args.warmup),
               "symmetry": timed(lambda: ss.find_symmetry(frac, lattice, off, types, p.search()), args.reps, args.warmup)}
        r = sz.symmetrize(frac, lattice, off, types, p, found)
        out["n_ops_max"], out["flagged"] = int(found["n_ops"].max()), int((r["flags"] != 0).sum())
        out["max_displacement"] = float(r["max_displacement"].max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
