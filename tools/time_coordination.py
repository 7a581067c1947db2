"""Time the coordination launch (arreau_crystal_coordination) with device events beside the screen's launch
(arreau_crystal_screen) on the same batch in the same process, at search_radius = cutoff: the screen is the yardstick because the
image walk is the same.  Inputs per shape B x n (the benchmark's 256 x 20, and 1024 x 64): the final state of a sample of a synthetic
model -- where its sampler comes out finite: the line says so where it does not -- and random crystals at 18 A^3 per atom.

    python tools/time_coordination.py [--shapes 256x20,1024x64] [--reps 30] [--inner 20] [--warmup 3]

Both entry points are called directly with their outputs allocated once, so a window holds launches alone; a window is `inner`
back-to-back launches between two events (a single launch of some tens of microseconds would measure the events), the two kernels'
windows alternate, and the time per launch is reported as median / min / p90 over `reps` windows.  Also printed: the contacts each
kernel evaluates, counted from the cells (screen: n (n + 1) / 2 M per crystal; coordination: 2 n^2 M, two walks over all j), and the
two ratios.  One JSON line per input."""
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
from arreau_amd.diffusion import crystal_batch as cb  # noqa: E402
from arreau_amd.diffusion import screening as sc  # noqa: E402
from tools.time_symmetrize import sampled  # noqa: E402
from tools.time_uniqueness import batch  # noqa: E402


def launchers(frac, lattice, off, params):
    """(screen, coordination): closures that launch one kernel each into outputs allocated here, and the coordination's outputs."""
    dev, B, N = frac.device, int(lattice.shape[0]), int(frac.shape[0])
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    s_out = {"min_distance": torch.empty(B, **f32), "pair": torch.empty((B, 5), **i32), "n_close": torch.empty(B, **i32),
             "volume": torch.empty(B, **f32), "number_density": torch.empty(B, **f32), "flags": torch.empty(B, **i32)}
    c_out = {k: torch.empty(B, **(f32 if k == "mean_cn" else i32)) for k in co.COORD_KEYS}
    c_out.update({"cn": torch.empty(N, **i32), "neighbors": torch.empty((N, params.max_neighbors, 4), **i32), "nearest": torch.empty(N, **f32),
                  "farthest": torch.empty(N, **f32), "mutual": torch.empty(N, **i32), "nearest_d2": torch.empty(N, **f32)})
    crit = _hip.ScreenCriteriaC(0.0, 0.0, params.cutoff, -1, params.max_shells)
    s_res = _hip.ScreenResultC(*[_hip.ptr(s_out[k]).value for k in sc.METRIC_KEYS])
    c_par = _hip.CoordinationParamsC(params.tol, params.cutoff, params.max_neighbors, params.max_shells)
    c_res = _hip.CoordinationResultC(*[_hip.ptr(c_out[k]).value for k in co.RESULT_KEYS])
    lib, stream = _hip.lib(), _hip.stream_ptr(dev)
    a = (_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off))

    def screen():
        _hip.check(lib.arreau_crystal_screen(a[0], None, a[1], a[2], B, N, ctypes.byref(crit), ctypes.byref(s_res), stream), "arreau_crystal_screen")

    def coordination():
        _hip.check(lib.arreau_crystal_coordination(a[0], a[1], a[2], B, N, ctypes.byref(c_par), ctypes.byref(c_res), stream), "arreau_crystal_coordination")
    return screen, coordination, c_out


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def spread(times, unit="_us"):
    t = np.sort(times)
    return {"median" + unit: float(np.median(t)), "min" + unit: float(t[0]), "p90" + unit: float(t[int(0.9 * (len(t) - 1))])}


def contact_counts(lattice, counts, params):
    """(screen, coordination) contacts of the crystals both kernels search, from the float32 cells."""
    s = c = 0
    for L, n in zip(lattice, counts):
        _, q, bad = cb.cell_f32(L, params.cutoff, 0.0, params.max_shells)
        if not bad and np.isfinite(L).all():
            M = int(np.prod([2 * max(1, int(np.ceil(qk))) + 1 for qk in q]))
            s, c = s + n * (n + 1) // 2 * M, c + 2 * n * n * M
    return s, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20,1024x64")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100, help="denoising steps of the sampled input")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    params = co.CoordinationParams()
    inputs = []
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.split("x"))
        try:
            inputs.append((f"sampled {shape}", sampled(B, n, dev, args.steps)[:3]))
        except _hip.ArreauHipError as e:  # (a synthetic model's activations can leave every kernel's range at a large shape)
            print(json.dumps({"input": f"sampled {shape}", "error": str(e)[:160]}), flush=True)
        inputs.append((f"random {shape}", tuple(torch.as_tensor(v, device=dev) for v in batch(B, n, 2)[:3])))
    for name, (frac, lattice, off) in inputs:
        screen, coordination, c_out = launchers(frac, lattice, off, params)
        for _ in range(args.warmup):
            window(screen, args.inner), window(coordination, args.inner)
        ts, tc = [], []
        for _ in range(args.reps):  # alternating windows: what else runs on the machine meets both alike
            ts.append(window(screen, args.inner))
            tc.append(window(coordination, args.inner))
        ns, nc = contact_counts(lattice.cpu().numpy(), np.diff(off.cpu().numpy()).tolist(), params)
        r = co.result_to_numpy(c_out)
        st = co.stats_of(dict(r, species=None))
        out = {"input": name, "steps": args.steps, "tol": params.tol, "cutoff": params.cutoff, "reps": args.reps, "inner": args.inner,
               "screen": spread(ts), "coordination": spread(tc), "time_ratio_median": float(np.median(tc) / np.median(ts)),
               "time_ratio_windows": spread(np.asarray(tc) / np.asarray(ts), ""), "contacts_screen": ns, "contacts_coordination": nc,
               "contact_ratio": nc / ns if ns else None, "mean_cn": st["n_bonds"] / max(st["atoms"], 1), "flags": {k: v for k, v in st["flags"].items() if v}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
