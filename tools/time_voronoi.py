"""Time the Voronoi launch (arreau_crystal_voronoi) with device events beside the coordination launch
(arreau_crystal_coordination) on the same batch in the same process at the same cutoff: the coordination search is the yardstick
because the candidates come from the same image walk.  Inputs per shape B x n (the benchmark's 256 x 20): the benchmark's
sampler-start state (tools/time_contact_guidance.py: BenchState, after `--state_steps` steps of the loop, which writes its cells:
N(0, 1) A lengths, so tiny cells with many images: what CELL and OVERFLOW make of them is printed) and random crystals at
18 A^3 per atom; with --sampled also the final state of a free sample of the tests' synthetic model.

    python tools/time_voronoi.py [--shapes 256x20] [--reps 20] [--inner 5] [--warmup 2] [--cutoff 6.0] [--state_steps 5] [--sampled]

Both entry points are called directly with their outputs allocated once, so a window holds launches alone; a window is `inner`
back-to-back launches between two events, the two kernels' windows alternate, and the time per launch is reported as median / min
/ p90 over `reps` windows.  Also printed: the mean number of candidates per atom (not an output: it is the cn of a coordination
search at a tolerance large enough to take everything within the cutoff), the plane-triple count C^3 / 2 summed over the atoms
that are built, mean cn and cn_eff, the atoms built, the OVERFLOW atoms, the share of OPEN atoms and the flags.  One JSON line
per input."""
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
from arreau_amd.diffusion import voronoi as vo  # noqa: E402
from tools.time_contact_guidance import BenchState, T  # noqa: E402
from tools.time_coordination import spread, window  # noqa: E402
from tools.time_symmetrize import sampled  # noqa: E402
from tools.time_uniqueness import batch  # noqa: E402


def launchers(frac, lattice, off, params, cparams):
    """(coordination, voronoi): closures that launch one kernel each into outputs allocated here, and both outputs."""
    dev, B, N = frac.device, int(lattice.shape[0]), int(frac.shape[0])
    c_out = co.coordination(frac, lattice, off, cparams)
    v_out = vo.voronoi(frac, lattice, off, params)
    c_par = _hip.CoordinationParamsC(cparams.tol, cparams.cutoff, cparams.max_neighbors, cparams.max_shells)
    c_res = _hip.CoordinationResultC(*[_hip.ptr(c_out[k]).value for k in co.RESULT_KEYS])
    v_par = _hip.VoronoiParamsC(params.tol, params.cutoff, params.max_faces, params.max_candidates, params.max_shells)
    v_res = _hip.VoronoiResultC(*[_hip.ptr(v_out[k]).value for k in vo.RESULT_KEYS])
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)
    a = (_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off))

    def coordination():
        _hip.check(lib.arreau_crystal_coordination(a[0], a[1], a[2], B, N, ctypes.byref(c_par), ctypes.byref(c_res), stream), "arreau_crystal_coordination")

    def voronoi():
        _hip.check(lib.arreau_crystal_voronoi(a[0], a[1], a[2], B, N, ctypes.byref(v_par), ctypes.byref(v_res), stream), "arreau_crystal_voronoi")
    return coordination, voronoi, c_out, v_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cutoff", type=float, default=6.0)
    ap.add_argument("--steps", type=int, default=100, help="--sampled: denoising steps of the sampled input")
    ap.add_argument("--state_steps", type=int, default=5, help="steps of the loop before the benchmark state is read")
    ap.add_argument("--sampled", action="store_true", help="also time the final state of a free sample of the tests' synthetic model")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    params = vo.VoronoiParams(cutoff=args.cutoff)
    cparams = co.CoordinationParams(cutoff=args.cutoff)
    inputs = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        st = BenchState(B, n, dev)
        st.run(T - 1, args.state_steps)  # a state the loop has visited (and the cell arreau_sample_loop wrote)
        inputs.append((f"bench state {shape} after {args.state_steps} steps", (st.frac.clone(), st.lattice.clone(), st.off)))
        if args.sampled:
            try:
                inputs.append((f"sampled {shape}", sampled(B, n, dev, args.steps)[:3]))
            except _hip.ArreauHipError as e:  # (a synthetic model's activations can leave every kernel's range at a large shape)
                print(json.dumps({"input": f"sampled {shape}", "error": str(e)[:160]}), flush=True)
        inputs.append((f"random {shape}", tuple(torch.as_tensor(v, device=dev) for v in batch(B, n, 2)[:3])))
    for name, (frac, lattice, off) in inputs:
        coordination, voronoi, _, v_out = launchers(frac, lattice, off, params, cparams)
        for _ in range(args.warmup):
            window(coordination, args.inner), window(voronoi, args.inner)
        tc, tv = [], []
        for _ in range(args.reps):  # alternating windows: what else runs on the machine meets both alike
            tc.append(window(coordination, args.inner))
            tv.append(window(voronoi, args.inner))
        # the candidates per atom: everything the coordination rule finds within the cutoff at a tolerance that takes it all
        wide = co.result_to_numpy(co.coordination(frac, lattice, off, co.CoordinationParams(tol=1e6, cutoff=args.cutoff, max_neighbors=1)))
        cand = wide["cn"].astype(np.float64)
        got = vo.result_to_numpy(v_out)
        st = vo.stats_of(dict(got, species=None))
        over = (got["atom_flags"] & vo.OVERFLOW) != 0
        out = {"input": name, "steps": args.steps, "tol": params.tol, "cutoff": params.cutoff, "reps": args.reps, "inner": args.inner,
               "coordination": spread(tc), "voronoi": spread(tv), "time_ratio_median": float(np.median(tv) / np.median(tc)),
               "candidates_mean": float(cand.mean()) if cand.size else None, "candidates_max": float(cand.max(initial=0)),
               "plane_triples": float((cand[~over] ** 3 / 2).sum()), "overflow_atoms": int(over.sum()),
               "mean_cn": st["n_faces"] / max(st["atoms"], 1), "mean_cn_eff": st["cn_eff"] / max(st["atoms"], 1),
               "atoms_built": st["atoms"], "open_share": st["open"] / max(st["atoms"], 1), "flags": {k: v for k, v in st["flags"].items() if v}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
