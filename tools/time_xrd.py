"""Time the powder-pattern launch (arreau_crystal_xrd) with device events beside the screen's launch (arreau_crystal_screen, at
search_radius 6 A) on the same batch in the same process: the screen is what every other per-crystal instrument's tool measures
against.  Inputs per shape B x n (the benchmark's 256 x 20), the two tools/time_voronoi.py uses: the benchmark's sampler-start
state (tools/time_contact_guidance.py: BenchState, after `--state_steps` steps of the loop, which writes its cells: N(0, 1) A
lengths, so tiny cells with few reflections in range) and random crystals at 18 A^3 per atom.

    python tools/time_xrd.py [--shapes 256x20] [--reps 20] [--inner 5] [--warmup 2] [--state_steps 5] [--points 1701] [--fwhm 0.2]

Both entry points are called directly with their outputs allocated once, so a window holds launches alone; a window is `inner`
back-to-back launches between two events, the two kernels' windows alternate, and the time per launch is reported as median / min
/ p90 over `reps` windows.  Also printed: the mean and largest number of box entries a crystal walks, the mean number of lattice
points kept, the atom-reflection pairs of the structure-factor sums (n times the half space's kept reflections, summed) and the
flags.  One JSON line per input."""
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
from arreau_amd.diffusion import xrd  # noqa: E402
from tools import time_coordination  # noqa: E402
from tools.time_contact_guidance import BenchState, T  # noqa: E402
from tools.time_coordination import spread, window  # noqa: E402
from tools.time_uniqueness import batch  # noqa: E402


def launcher(frac, lattice, off, weights, params):
    """A closure that launches the pattern kernel into outputs allocated here, and those outputs."""
    dev, B, N = frac.device, int(lattice.shape[0]), int(frac.shape[0])
    out = xrd.xrd(frac, lattice, off, weights, params)
    par = _hip.XrdParamsC(params.wavelength, params.two_theta_min, params.two_theta_max, params.fwhm, params.b_iso, params.n_points, params.max_index)
    res = _hip.XrdResultC(*[_hip.ptr(out[k]).value for k in xrd.RESULT_KEYS])
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)
    a = (_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), _hip.ptr(weights))

    def pattern():
        _hip.check(lib.arreau_crystal_xrd(a[0], a[1], a[2], a[3], B, N, ctypes.byref(par), ctypes.byref(res), stream), "arreau_crystal_xrd")
    return pattern, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--state_steps", type=int, default=5, help="steps of the loop before the benchmark state is read")
    ap.add_argument("--points", type=int, default=1701)
    ap.add_argument("--fwhm", type=float, default=0.2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    params = xrd.XrdParams(n_points=args.points, fwhm=args.fwhm, scattering="weights")
    inputs = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        st = BenchState(B, n, dev)
        st.run(T - 1, args.state_steps)  # a state the loop has visited (and the cell arreau_sample_loop wrote)
        inputs.append((f"bench state {shape} after {args.state_steps} steps", (st.frac.clone(), st.lattice.clone(), st.off), n))
        inputs.append((f"random {shape}", tuple(torch.as_tensor(v, device=dev) for v in batch(B, n, 2)[:3]), n))
    for name, (frac, lattice, off), n in inputs:
        weights = torch.as_tensor(1.0 + (np.arange(int(frac.shape[0])) % 83), dtype=torch.float32, device=dev)  # atomic numbers 1..83
        screen = time_coordination.launchers(frac, lattice, off, co.CoordinationParams(cutoff=6.0))[0]
        pattern, out = launcher(frac, lattice, off, weights, params)
        for _ in range(args.warmup):
            window(screen, args.inner), window(pattern, args.inner)
        ts, tx = [], []
        for _ in range(args.reps):  # alternating windows: what else runs on the machine meets both alike
            ts.append(window(screen, args.inner))
            tx.append(window(pattern, args.inner))
        got = xrd.result_to_numpy(out)
        ok = got["flags"] == 0
        cells = lattice.cpu().numpy()
        box = np.array([xrd.box_of(c, params) for c in cells[ok]]).reshape(-1, 3)
        entries = (box[:, 0] + 1) * (2 * box[:, 1] + 1) * (2 * box[:, 2] + 1)
        st = xrd.stats_of(xrd.sample_arrays(got, params))
        print(json.dumps({"input": name, "n_points": params.n_points, "fwhm": params.fwhm, "reps": args.reps, "inner": args.inner,
                          "screen": spread(ts), "xrd": spread(tx), "time_ratio_median": float(np.median(tx) / np.median(ts)),
                          "patterns": int(ok.sum()), "box_entries_mean": float(entries.mean()) if entries.size else None,
                          "box_entries_max": float(entries.max(initial=0)), "n_reflections_mean": st["n_reflections"] / max(st["patterns"], 1),
                          "atom_reflection_pairs": float(n * got["n_reflections"][ok].sum() / 2), "flags": {k: v for k, v in st["flags"].items() if v}}), flush=True)


if __name__ == "__main__":
    main()
