"""Time the Ewald launch (arreau_crystal_ewald) with device events beside the screen's launch (arreau_crystal_screen, at
search_radius 6 A) on the same batch in the same process: the screen is what every other per-crystal instrument's tool measures
against.  Inputs per shape B x n (the benchmark's 256 x 20), the two tools/time_xrd.py uses: the benchmark's sampler-start state
(tools/time_contact_guidance.py: BenchState, after `--state_steps` steps of the loop, which writes its cells: N(0, 1) A lengths,
so tiny cells, most of which need more images than max_shells allows) and random crystals at 18 A^3 per atom.  The charges
alternate +1, -1 along the atoms.

    python tools/time_ewald.py [--shapes 256x20] [--reps 20] [--inner 5] [--warmup 2] [--state_steps 5] [--accuracy 1e-8]

Both entry points are called directly with their outputs allocated once, so a window holds launches alone; a window is `inner`
back-to-back launches between two events, the two kernels' windows alternate, and the time per launch is reported as median / min
/ p90 over `reps` windows.  Also printed: the crystals with an energy, the real-space terms and the lattice points kept (summed
and per crystal with an energy), the mean alpha and the flags.  One JSON line per input."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd import _hip  # noqa: E402
from arreau_amd.diffusion import coordination as co  # noqa: E402
from arreau_amd.diffusion import ewald  # noqa: E402
from tools import time_coordination  # noqa: E402
from tools.time_contact_guidance import BenchState, T  # noqa: E402
from tools.time_coordination import spread, window  # noqa: E402
from tools.time_uniqueness import batch  # noqa: E402


def launcher(frac, lattice, off, charges, params):
    """A closure that launches the Ewald kernel into outputs allocated here, and those outputs."""
    dev, B, N = frac.device, int(lattice.shape[0]), int(frac.shape[0])
    out = ewald.ewald(frac, lattice, off, charges, params)
    work = torch.empty_like(out["potential"])
    par = _hip.EwaldParamsC(params.accuracy, params.alpha or 0.0, params.max_shells, params.max_index)
    res = _hip.EwaldResultC(*[_hip.ptr(out[k]).value for k in ewald.RESULT_KEYS], _hip.ptr(work).value)
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)
    a = (_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), _hip.ptr(charges))

    def sums():
        _hip.check(lib.arreau_crystal_ewald(a[0], a[1], a[2], a[3], B, N, ctypes.byref(par), ctypes.byref(res), stream), "arreau_crystal_ewald")
    return sums, (out, work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--state_steps", type=int, default=5, help="steps of the loop before the benchmark state is read")
    ap.add_argument("--accuracy", type=float, default=1e-8)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    params = ewald.EwaldParams(accuracy=args.accuracy)
    inputs = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        st = BenchState(B, n, dev)
        st.run(T - 1, args.state_steps)  # a state the loop has visited (and the cell arreau_sample_loop wrote)
        inputs.append((f"bench state {shape} after {args.state_steps} steps", (st.frac.clone(), st.lattice.clone(), st.off), n))
        inputs.append((f"random {shape}", tuple(torch.as_tensor(v, device=dev) for v in batch(B, n, 2)[:3]), n))
    for name, (frac, lattice, off), n in inputs:
        charges = torch.as_tensor(1.0 - 2.0 * (np.arange(int(frac.shape[0])) % 2), dtype=torch.float32, device=dev)
        screen = time_coordination.launchers(frac, lattice, off, co.CoordinationParams(cutoff=6.0))[0]
        sums, (out, _work) = launcher(frac, lattice, off, charges, params)
        for _ in range(args.warmup):
            window(screen, args.inner), window(sums, args.inner)
        ts, te = [], []
        for _ in range(args.reps):  # alternating windows: what else runs on the machine meets both alike
            ts.append(window(screen, args.inner))
            te.append(window(sums, args.inner))
        got = ewald.result_to_numpy(out)
        ok = (got["flags"] & ewald.INVALID_MASK) == 0
        k = max(int(ok.sum()), 1)
        print(json.dumps({"input": name, "accuracy": params.accuracy, "reps": args.reps, "inner": args.inner, "screen": spread(ts), "ewald": spread(te),
                          "time_ratio_median": float(np.median(te) / np.median(ts)), "energies": int(ok.sum()),
                          "n_pairs": int(got["n_pairs"][ok].sum()), "n_pairs_mean": float(got["n_pairs"][ok].sum() / k),
                          "n_reciprocal_mean": float(got["n_reciprocal"][ok].sum() / k), "alpha_mean": float(got["alpha"][ok].mean()) if ok.any() else None,
                          "flags": {flag: int(((got["flags"] & bit) != 0).sum()) for bit, flag in ewald.FLAG_NAMES if ((got["flags"] & bit) != 0).any()}}), flush=True)


if __name__ == "__main__":
    main()
