"""Time the bond-order launch (arreau_crystal_bond_order) with device events beside the coordination launch
(arreau_crystal_coordination) whose lists it reads, on the same batch in the same process.  Inputs per shape B x n (the benchmark's
256 x 20, and 1024 x 64): the final state of a sample of a synthetic model -- where its sampler comes out finite: the line says so
where it does not --, random crystals at 18 A^3 per atom (shells of one or two bonds) and, for shells that fill the pair loop, fcc
supercells of 32 atoms with a small seeded jitter: with the default parameters (12 bonds, 66 pairs per atom) and with tol = 1.4 and
max_neighbors = 64 (78 neighbours cut at 64 bonds: 2016 pairs per atom, the most the launch can meet).

    python tools/time_bond_order.py [--shapes 256x20,1024x64] [--reps 30] [--inner 20] [--warmup 3]

Both entry points are called directly with their outputs allocated once, so a window holds launches alone; a window is `inner`
back-to-back launches between two events, the two kernels' windows alternate, and the time per launch is reported as median / min /
p90 over `reps` windows.  Also printed: the pairs the new launch evaluates, the mean shell size and the ratio.  One JSON line per
input."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd import _hip  # noqa: E402
from arreau_amd.diffusion import bond_order as bo  # noqa: E402
from tools.time_coordination import launchers, spread, window  # noqa: E402
from tools.time_symmetrize import sampled  # noqa: E402
from tools.time_uniqueness import batch  # noqa: E402


def bond_order_launcher(frac, lattice, off, c_out, max_neighbors):
    """A closure that launches the new kernel on the coordination outputs `c_out` into outputs allocated here, and those outputs."""
    dev, B, N = frac.device, int(lattice.shape[0]), int(frac.shape[0])
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"mean_q": torch.empty((B, 4), **f32), "n_angles": torch.empty(B, **i32), "angle_hist": torch.empty((B, bo.ANGLE_BINS), **i32),
           "flags": torch.empty(B, **i32), "n_used": torch.empty(N, **i32), "q": torch.empty((N, 4), **f32), "q2": torch.empty((N, 4), **f32),
           "cos_min": torch.empty(N, **f32), "cos_max": torch.empty(N, **f32), "angles": torch.empty((N, bo.ANGLE_BINS), **i32)}
    par = _hip.BondOrderParamsC(max_neighbors, (ctypes.c_float * (bo.ANGLE_BINS - 1))(*[float(e) for e in bo.COS_EDGES]))
    res = _hip.BondOrderResultC(*[_hip.ptr(out[k]).value for k in bo.RESULT_KEYS])
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)
    a = (_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), _hip.ptr(c_out["cn"]), _hip.ptr(c_out["neighbors"]))

    def bond_order():
        _hip.check(lib.arreau_crystal_bond_order(a[0], a[1], a[2], B, N, a[3], a[4], ctypes.byref(par), ctypes.byref(res), stream),
                   "arreau_crystal_bond_order")
    return bond_order, out


def fcc_supercells(B, dev, a=3.61, jitter=0.002, seed=0):
    """B crystals of 2 x 2 x 2 conventional fcc cells (32 atoms), fractional coordinates jittered by up to `jitter`."""
    sites = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    cells = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    frac = ((cells + sites[None]) / 2.0).reshape(-1, 3)
    rng = np.random.RandomState(seed)
    frac = (frac[None] + rng.uniform(-jitter, jitter, (B,) + frac.shape)).astype(np.float32).reshape(-1, 3)
    lattice = np.broadcast_to(np.eye(3, dtype=np.float32) * np.float32(2 * a), (B, 3, 3)).copy()
    off = (np.arange(B + 1) * 32).astype(np.int32)
    return tuple(torch.as_tensor(v, device=dev) for v in (frac, lattice, off))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20,1024x64")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100, help="denoising steps of the sampled input")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    params = bo.BondOrderParams()
    inputs = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        try:
            inputs.append((f"sampled {shape}", sampled(B, n, dev, args.steps)[:3], params))
        except _hip.ArreauHipError as e:  # (a synthetic model's activations can leave every kernel's range at a large shape)
            print(json.dumps({"input": f"sampled {shape}", "error": str(e)[:160]}), flush=True)
        inputs.append((f"random {shape}", tuple(torch.as_tensor(v, device=dev) for v in batch(B, n, 2)[:3]), params))
        inputs.append((f"fcc {B}x32", fcc_supercells(B, dev), params))
        inputs.append((f"fcc {B}x32, tol 1.4, 64 bonds", fcc_supercells(B, dev), bo.BondOrderParams(tol=1.4, max_neighbors=64)))
    for name, (frac, lattice, off), params in inputs:
        _, coordination, c_out = launchers(frac, lattice, off, params.coordination())
        coordination()  # (the lists the new launch reads)
        bond_order, out = bond_order_launcher(frac, lattice, off, c_out, params.max_neighbors)
        for _ in range(args.warmup):
            window(coordination, args.inner), window(bond_order, args.inner)
        tc, tb = [], []
        for _ in range(args.reps):  # alternating windows: what else runs on the machine meets both alike
            tc.append(window(coordination, args.inner))
            tb.append(window(bond_order, args.inner))
        r = bo.result_to_numpy(out)
        flags = {n_: int(((r["flags"] & bit) != 0).sum()) for bit, n_ in bo.FLAG_NAMES}
        line = {"input": name, "steps": args.steps, "tol": params.tol, "cutoff": params.cutoff, "reps": args.reps, "inner": args.inner,
                "coordination": spread(tc), "bond_order": spread(tb), "time_ratio_median": float(np.median(tb) / np.median(tc)),
                "time_ratio_windows": spread(np.asarray(tb) / np.asarray(tc), ""), "pairs": int(r["n_angles"].sum()),
                "mean_shell": float(r["n_used"].mean()) if r["n_used"].size else None, "flags": {k: v for k, v in flags.items() if v}}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
