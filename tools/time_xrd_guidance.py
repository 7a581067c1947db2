"""Time XRD guidance (arreau_xrd_guidance_step, arreau_sample_loop_xrd_guided; rules in include/arreau_hip.h, "XRD guidance") with
device events, in tools/time_xrd.py's form.

  launch   the guidance launch beside the pattern launch (arreau_crystal_xrd) on the same state in the same process, windows
           alternating, on the two 256 x 20 inputs tools/time_xrd.py uses: the benchmark's sampler-start state after
           `--state_steps` steps of the loop (N(0, 1) A lengths: tiny cells with few reflections in range) and random crystals at
           18 A^3 per atom.  The amplitudes are atomic numbers 1..83 by atom; the targets are the patterns of the same cells with
           other positions.
  step     the guided step against the unguided one on the benchmark's state, eager and with graph replay, windows alternating;
           every class weighs its index + 1 (the benchmark's state is all mask, which would not scatter).

    python tools/time_xrd_guidance.py [--parts launch,step] [--shape 256x20] [--reps 20] [--inner 5] [--warmup 2] [--k 20]

One JSON line per input and part: median / min / p90 per launch or per step in microseconds, the reflections, distances and flags
of the guided state."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd import _hip  # noqa: E402
from arreau_amd.diffusion import xrd, xrd_guidance as xg  # noqa: E402
from tools.time_contact_guidance import BenchState, S, T  # noqa: E402
from tools.time_coordination import spread, window  # noqa: E402
from tools.time_uniqueness import batch  # noqa: E402
from tools.time_xrd import launcher  # noqa: E402


def targets(frac, lattice, off, weights, params, seed=5):
    """The patterns of the same cells and amplitudes with other positions; a crystal without one (flagged) gets a flat row."""
    other = torch.as_tensor(np.random.RandomState(seed).uniform(size=tuple(frac.shape)).astype(np.float32), device=frac.device)
    rows = xrd.xrd(other, lattice, off, weights, params)["pattern"]
    flat = ~torch.isfinite(rows).all(dim=1) | (rows.sum(dim=1) <= 0)
    rows[flat] = 1.0
    return rows.contiguous()


def part_launch(name, frac, lattice, off, t_c, eng, args):
    dev, B, N = frac.device, int(lattice.shape[0]), int(frac.shape[0])
    params = xrd.XrdParams(n_points=args.points, fwhm=args.fwhm, scattering="weights")
    weights = torch.as_tensor(1.0 + (np.arange(N) % 83), dtype=torch.float32, device=dev)
    pattern, _ = launcher(frac, lattice, off, weights, params)
    guide = xg.DeviceGuidance(params, args.weight, targets(frac, lattice, off, weights, params), atom_weights=weights, info=xg.allocate_info(B, dev))
    struct = eng._xrd_guidance_struct(guide, B, N, step=True)
    eps = torch.randn(N, 3, device=dev)
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def guidance():
        _hip.check(lib.arreau_xrd_guidance_step(eng._handle, _hip.ptr(frac), None, _hip.ptr(lattice), _hip.ptr(t_c), _hip.ptr(off), B, N,
                                                _hip.ptr(eps), ctypes.byref(struct), None, stream), "arreau_xrd_guidance_step")
    for _ in range(args.warmup):
        window(pattern, args.inner), window(guidance, args.inner)
    tx, tg = [], []
    for _ in range(args.reps):  # alternating windows: what else runs on the machine meets both alike
        tx.append(window(pattern, args.inner))
        tg.append(window(guidance, args.inner))
    st = xg.stats_of(xg.info_to_numpy(guide.info))
    return {"part": "launch", "input": name, "n_points": params.n_points, "fwhm": params.fwhm, "reps": args.reps, "inner": args.inner,
            "xrd": spread(tx), "guidance": spread(tg), "time_ratio_median": float(np.median(tg) / np.median(tx)), "guided": st["guided"],
            "n_reflections_mean": float(guide.info["reflections"].float().mean()), "distance_mean": st["distance_sum"] / max(st["guided"], 1),
            "flags": {k: v for k, v in st["flags"].items() if v}}


def part_step(st, args):
    """Per-step microseconds of k steps in one call: unguided and guided, eager and graph replay, the windows alternating."""
    dev = st.dev
    params = xrd.XrdParams(n_points=args.points, fwhm=args.fwhm)
    table = torch.arange(1, S + 1, device=dev, dtype=torch.float32)
    st.fresh()
    st.run(T - 1, args.state_steps)
    rows = targets(st.frac, st.lattice, st.off, table[st.types.long()].contiguous(), xrd.for_weights(xrd.XrdParams(n_points=args.points, fwhm=args.fwhm, scattering="weights")))
    guide = xg.DeviceGuidance(params, args.weight, rows, class_weights=table, info=xg.allocate_info(st.B, dev))

    def one(guided, use_graph):
        st.fresh()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        st.eng.sample_loop(st.frac, st.types, st.lengths, st.angles, st.off, T - 1, args.k, 77, None, st.lattice, use_graph=use_graph,
                           fixed_lengths=st.lengths0, xrd_guidance=guide if guided else None)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.k
    variants = [("unguided_eager", False, False), ("guided_eager", True, False), ("unguided_graph", False, True), ("guided_graph", True, True)]
    times = {name: [] for name, _, _ in variants}
    for rep in range(args.warmup + args.reps):
        for name, guided, use_graph in variants:
            v = one(guided, use_graph)
            if rep >= args.warmup:
                times[name].append(v)
    stats = xg.stats_of(xg.info_to_numpy(guide.info))
    out = {"part": "step", "shape": f"{st.B}x{st.n}", "k": args.k, "reps": args.reps, **{name: spread(v) for name, v in times.items()},
           "guided_crystals_last_evaluation": stats["guided"], "flags": {k: v for k, v in stats["flags"].items() if v}}
    for mode in ("eager", "graph"):
        out[f"guidance_cost_{mode}_us"] = float(np.median(times[f"guided_{mode}"]) - np.median(times[f"unguided_{mode}"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="launch,step")
    ap.add_argument("--shape", default="256x20")
    ap.add_argument("--weight", type=float, default=xg.DEFAULT_WEIGHT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=20, help="step: steps per window")
    ap.add_argument("--state_steps", type=int, default=5, help="steps of the unguided loop before the timed state")
    ap.add_argument("--points", type=int, default=1701)
    ap.add_argument("--fwhm", type=float, default=0.2)
    args = ap.parse_args()
    B, n = (int(v) for v in args.shape.split("x"))
    dev = torch.device("cuda", 0)
    st = BenchState(B, n, dev)
    parts = args.parts.split(",")
    if "launch" in parts:
        st.run(T - 1, args.state_steps)  # a state the loop has visited (and the cell arreau_sample_loop wrote)
        t_c = torch.full((B,), T - 1 - args.state_steps, device=dev, dtype=torch.int32)
        inputs = [(f"bench state {args.shape} after {args.state_steps} steps", (st.frac.clone(), st.lattice.clone(), st.off)),
                  (f"random {args.shape}", tuple(torch.as_tensor(v, device=dev) for v in batch(B, n, 2)[:3]))]
        for name, (frac, lattice, off) in inputs:
            print(json.dumps(part_launch(name, frac, lattice, off, t_c, st.eng, args)), flush=True)
    if "step" in parts:
        print(json.dumps(part_step(st, args)), flush=True)


if __name__ == "__main__":
    main()
