"""Time contact guidance (arreau_launch_contact_guide; rules in include/arreau_hip.h, "contact guidance") on the benchmark's
configuration (256 crystals x 20 atoms, S = 90, T = 1000, the sampler-start state at fixed cell lengths, bench.py):

  launch   the guidance launch alone with device events, beside the screen's launch on the same state at search_radius =
           min_distance (the same image walk): windows of `inner` back-to-back launches, alternating, median / min / p90;
  step     the sampling step with and without guidance: windows of `k` steps of Engine.sample_loop (eager and graph replay),
           alternating; with --parent_lib the unguided step of that library too (another build of libarreau_hip.so, e.g. the
           parent commit's: a fresh process with ARREAU_HIP_LIB, started after this one's windows), on the same box;
  close    the screen's CLOSE crystals and contacts below min_distance after --num_steps steps from one seed, with and without
           guidance.  A measurement: with a synthetic model nothing is promised about it.

    python tools/time_contact_guidance.py [--parts launch,step,close] [--parent_lib tools/exp/ab/lib_prev.so] [--num_steps 50]

One JSON line per part."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd import _hip  # noqa: E402
from arreau_amd.diffusion import contact_guidance as cg  # noqa: E402
from arreau_amd.diffusion import screening as sc  # noqa: E402
from tools.time_coordination import spread, window  # noqa: E402

S, T = 90, 1000


class BenchState:
    """bench.py's sampler-start state of B x n (rank 0) and its model."""

    def __init__(self, B, n, dev):
        from arreau_amd.checkpoint import make_synthetic_model
        from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
        self.B, self.n, self.N, self.dev = B, n, B * n, dev
        self.model = make_synthetic_model(S=S, seed=1234, num_timesteps=T).to(dev)
        self.eng = self.model.engine()
        torch.manual_seed(1000)
        rng = np.random.RandomState(1000)
        f32 = dict(device=dev, dtype=torch.float32)
        self.angles = torch.tensor(np.stack([np.full(B, 90.0), rng.uniform(90, 180, B), np.full(B, 90.0)], 1), dtype=torch.float32).to(**f32)
        self.lengths0 = torch.randn(B, 3).to(**f32)
        self.frac0 = torch.randn(self.N, 3).to(**f32)
        self.off = crystal_offsets(torch.full((B,), n), dev)
        self.fresh()

    def fresh(self):
        self.frac, self.lengths = self.frac0.clone(), self.lengths0.clone()
        self.types = torch.full((self.N,), S - 1, device=self.dev, dtype=torch.int32)
        self.lattice = torch.zeros(self.B, 3, 3, device=self.dev)

    def run(self, t, k, guidance=None, use_graph=False, seed=77):
        self.eng.sample_loop(self.frac, self.types, self.lengths, self.angles, self.off, t, k, seed, None, self.lattice, use_graph=use_graph,
                             fixed_lengths=self.lengths0, guidance=guidance)


def part_launch(st, params, args, random_state=False):
    """The launch on the benchmark's state after a few steps (its cells are the sampler-start draws N(0, 1) A: tiny, many images
    per axis, many flagged CELL), or, random_state, on random crystals at 18 A^3 per atom (27 images: what a compact cell costs)."""
    st.fresh()
    st.run(T - 1, args.state_steps)  # a state the loop has visited (and the cell arreau_sample_loop wrote)
    dev, B, N = st.dev, st.B, st.N
    if random_state:
        from tools.time_uniqueness import batch
        frac, lattice = (torch.as_tensor(v, device=dev) for v in batch(B, st.n, 2)[:2])
        st.frac.copy_(frac), st.lattice.copy_(lattice)
    info = cg.allocate_info(B, dev)
    eps = torch.randn(N, 3, device=dev)
    t_c = torch.full((B,), T - 1 - args.state_steps, device=dev, dtype=torch.int32)
    guide = _hip.ContactGuidanceC(params.min_distance, params.weight, params.max_shells, *[_hip.ptr(info[q]).value for q in cg.INFO_KEYS])
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    s_out = {"min_distance": torch.empty(B, **f32), "pair": torch.empty((B, 5), **i32), "n_close": torch.empty(B, **i32),
             "volume": torch.empty(B, **f32), "number_density": torch.empty(B, **f32), "flags": torch.empty(B, **i32)}
    crit = _hip.ScreenCriteriaC(params.min_distance, 0.0, params.min_distance, -1, params.max_shells)
    s_res = _hip.ScreenResultC(*[_hip.ptr(s_out[k]).value for k in sc.METRIC_KEYS])
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)

    def guide_launch():
        _hip.check(lib.arreau_contact_guidance_step(st.eng._handle, _hip.ptr(st.frac), _hip.ptr(st.lattice), _hip.ptr(t_c), _hip.ptr(st.off), B, N,
                                                    _hip.ptr(eps), ctypes.byref(guide), stream), "arreau_contact_guidance_step")

    def screen_launch():
        _hip.check(lib.arreau_crystal_screen(_hip.ptr(st.frac), None, _hip.ptr(st.lattice), _hip.ptr(st.off), B, N, ctypes.byref(crit),
                                             ctypes.byref(s_res), stream), "arreau_crystal_screen")
    for _ in range(args.warmup):
        window(guide_launch, args.inner), window(screen_launch, args.inner)
    tg, ts = [], []
    for _ in range(args.reps):
        tg.append(window(guide_launch, args.inner))
        ts.append(window(screen_launch, args.inner))
    r = cg.info_to_numpy(info)
    return {"part": "launch", "input": "random, 18 A^3 per atom" if random_state else f"bench state after {args.state_steps} steps", "shape": f"{B}x{st.n}", "min_distance": params.min_distance, "reps": args.reps, "inner": args.inner,
            "guidance": spread(tg), "screen": spread(ts), "contacts": int(r["contacts"].sum()), "crystals_with_contacts": int((r["contacts"] > 0).sum()),
            "flags": {k: v for k, v in cg.stats_of(r)["flags"].items() if v}}


def step_windows(st, variants, args):
    """{name: per-step microseconds of every window}, the variants' windows alternating; a window is k steps in one call."""
    k, t0 = args.k, T - 1

    def one(guidance, use_graph):
        st.fresh()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        st.run(t0, k, guidance, use_graph)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / k
    times = {name: [] for name, _, _ in variants}
    for rep in range(args.warmup + args.reps):
        for name, guidance, use_graph in variants:
            v = one(guidance, use_graph)
            if rep >= args.warmup:
                times[name].append(v)
    return times


def part_step(st, params, args):
    info = cg.allocate_info(st.B, st.dev)
    variants = [("unguided_eager", None, False), ("guided_eager", (params, info), False), ("unguided_graph", None, True),
                ("guided_graph", (params, info), True)]
    if args.unguided_only:  # (another build of the library: it has no guided export)
        variants = [v for v in variants if v[1] is None]
    times = step_windows(st, variants, args)
    out = {"part": "step", "lib": os.environ.get("ARREAU_HIP_LIB", "in-tree"), "shape": f"{st.B}x{st.n}", "k": args.k, "reps": args.reps,
           **{name: spread(v) for name, v in times.items()}}
    for mode in ("eager", "graph"):
        if f"guided_{mode}" in times:
            out[f"guidance_cost_{mode}_us"] = float(np.median(times[f"guided_{mode}"]) - np.median(times[f"unguided_{mode}"]))
    return out


def part_close(st, params, args):
    out = {"part": "close", "shape": f"{st.B}x{st.n}", "num_steps": args.num_steps, "seed": 77, "min_distance": params.min_distance, "weight": params.weight}
    for name, guidance in (("unguided", None), ("guided", (params, cg.allocate_info(st.B, st.dev)))):
        st.fresh()
        st.run(T - 1, args.num_steps, guidance)
        st.eng.check_status()
        m = sc.metrics_to_numpy(st.eng.screen(st.frac, st.lattice, st.off, None, sc.ScreenCriteria(min_distance=params.min_distance, mask_type=-1)))
        out[name] = {"close_crystals": int(((m["flags"] & sc.CLOSE) != 0).sum()), "contacts_below_min_distance": int(m["n_close"].sum()),
                     "cell_flagged": int(((m["flags"] & sc.CELL) != 0).sum()), "nonfinite": int(((m["flags"] & sc.NONFINITE) != 0).sum()),
                     "median_shortest_contact": float(np.nanmedian(m["min_distance"]))}
        if guidance is not None:
            r = cg.info_to_numpy(guidance[1])
            out[name]["last_evaluation"] = {"contacts": int(r["contacts"].sum()), "flags": {k: v for k, v in cg.stats_of(r)["flags"].items() if v}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="launch,step,close")
    ap.add_argument("--shape", default="256x20")
    ap.add_argument("--min_distance", type=float, default=0.5)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=20, help="step: steps per window")
    ap.add_argument("--state_steps", type=int, default=5, help="launch: steps of the unguided loop before the timed state")
    ap.add_argument("--num_steps", type=int, default=50, help="close: steps from the sampler-start state")
    ap.add_argument("--parent_lib", default=None, help="step: also time the unguided step of this build of the library")
    ap.add_argument("--unguided_only", action="store_true", help="step: the unguided variants alone (set for --parent_lib's process)")
    args = ap.parse_args()
    B, n = (int(v) for v in args.shape.split("x"))
    params = cg.ContactGuidance(min_distance=args.min_distance, weight=args.weight)
    st = BenchState(B, n, torch.device("cuda", 0))
    parts = args.parts.split(",")
    for name, fn in (("launch", part_launch), ("step", part_step), ("close", part_close)):
        if name in parts:
            print(json.dumps(fn(st, params, args)), flush=True)
            if name == "launch":
                print(json.dumps(part_launch(st, params, args, random_state=True)), flush=True)
    if "step" in parts and args.parent_lib:
        env = dict(os.environ, ARREAU_HIP_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--parts", "step", "--unguided_only", "--shape", args.shape, "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--k", str(args.k)]
        subprocess.run(cmd, env=env, check=True, timeout=600)


if __name__ == "__main__":
    main()
