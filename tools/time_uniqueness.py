"""Time the two launches of duplicate detection with device events: arreau_crystal_fingerprint and arreau_fingerprint_match
(self mode) on random crystals at the sampler's density, B crystals of n atoms each.

    python tools/time_uniqueness.py [--shapes 256x20,8192x20] [--species 2] [--reps 30] [--warmup 5]

The windows include the wrappers' output allocations and ctypes calls, so they bound the kernels from above.  Prints one JSON
line per shape: median / min / p90 in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.diffusion import uniqueness as uq  # noqa: E402


def batch(B, n, species, seed=0, volume_per_atom=18.0):
    rng = np.random.RandomState(seed)
    a = (n * volume_per_atom) ** (1.0 / 3.0)
    lattice = (np.eye(3)[None] * a + rng.uniform(-0.1, 0.1, (B, 3, 3)) * a).astype(np.float32)
    types = np.tile(np.arange(n) % species, B).astype(np.int32)  # one formula: every pair of crystals is comparable
    return rng.uniform(0, 1, (B * n, 3)).astype(np.float32), lattice, (np.arange(B + 1) * n).astype(np.int32), types


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    t = np.sort(times)
    return {"median_us": float(np.median(t)), "min_us": float(t[0]), "p90_us": float(t[int(0.9 * (len(t) - 1))])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20,8192x20")
    ap.add_argument("--species", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        frac, lattice, off, types = (torch.as_tensor(v, device=dev) for v in batch(B, n, args.species))
        p = uq.FingerprintParams()
        fp = uq.fingerprint(frac, lattice, off, types, p)
        out = {"shape": shape, "species": args.species,
               "fingerprint": timed(lambda: uq.fingerprint(frac, lattice, off, types, p), args.reps, args.warmup),
               "match_self": timed(lambda: uq.match(fp, None, p.tolerance), args.reps, args.warmup)}
        m = uq.match(fp, None, p.tolerance)
        out["flagged"], out["duplicates"] = int((fp["flags"] != 0).sum()), int((m["duplicate_of"] >= 0).sum())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
