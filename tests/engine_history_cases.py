"""Batches and schedules of calls shared by tests/test_engine_history_cpu.py and tests/test_gpu_engine_history.py: what one engine
is handed, call after call, when the question is whether a step depends on what its engine ran before.  CPU only; the float64
oracle's neighbour list (oracle/geometry.py) states the facts the GPU tests rely on (`graph_facts`)."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import geometry as OG
from oracle import training as TR

S, T = 12, 100
RADIUS, K = 5.0, 8
F64 = torch.float64

# the two models, both make_synthetic_model(S=12, seed=1234, num_timesteps=100, **arguments)
MODELS = {
    "fused": {},   # the training forward is the fused ConvNext launch of node_f16m.hip at k = 8
    "narrow": dict(hidden_dim=12, basis_dim=20, widening_factor=3, layers=2),   # general kernels; one context trains, scores and samples
}


def make_batch(num_atoms, cells, timesteps, seed):
    """(batch, lattice0, timestep, noise): the body of tests/test_gpu_training.py: make_setup (S = 12, T = 100) for any number of
    crystals, with every draw injected.  `cells`: one (shortest, longest) range of cell lengths in angstrom per crystal;
    `timesteps`: one per crystal; `seed` seeds the crystals (numpy) and the noise (torch) alike."""
    rng = np.random.RandomState(seed)
    num_atoms = list(num_atoms)
    B, N = len(num_atoms), sum(num_atoms)
    assert len(cells) == B and len(timesteps) == B
    lo, hi = np.array(cells, dtype=np.float64).T
    lengths = torch.tensor(rng.uniform(lo[:, None], hi[:, None], size=(B, 3)), dtype=torch.float32)
    angles = torch.tensor(np.deg2rad(rng.uniform(75, 105, size=(B, 3))), dtype=torch.float32)
    lattice0 = OG.lattice_from_params(lengths, angles)
    frac0 = torch.tensor(rng.uniform(0, 1, size=(N, 3)), dtype=torch.float32)
    types0 = torch.tensor(rng.randint(0, S - 1, size=N))
    timestep = torch.tensor(list(timesteps))
    g = torch.Generator().manual_seed(seed)
    noise = (torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g), torch.randn(B, 3, generator=g))
    batch = SimpleNamespace(X0=frac0, A0=types0, L0=lattice0.reshape(-1, 3), num_atoms=torch.tensor(num_atoms))
    return batch, lattice0, timestep, noise


# How arreau_amd/csrc/train_net.hip: ensure_ctx sizes the one context of a model: the first call gets exactly (N, B); a call that
# does not fit regrows it to max(N, capN) * 5 / 4 and max(B, capB) * 5 / 4 (integer division of the quarter) in BOTH dimensions.
def capacity_after(sizes):
    """(capN, capB) of a context after calls of the given (N, B), by today's rule of ensure_ctx"""
    cap = None
    for n, b in sizes:
        if cap is None:
            cap = (n, b)
        elif n > cap[0] or b > cap[1]:
            cap = tuple(max(x, c) + max(x, c) // 4 for x, c in ((n, cap[0]), (b, cap[1])))
    return cap


_DENSE, _LOOSE, _ALONE = (3.5, 5.0), (3.5, 7.0), (12.0, 14.0)
# name -> make_batch arguments.  Seeds and timesteps were found by search on the CPU so that conditions 1-4 of
# tests/test_engine_history_cpu.py hold (as RADIUS_STATES of tests/test_gpu_model_shapes.py was found).
#   A      17 atoms; the 1-atom crystal alone in a 12-14 A cell (degree 0), the others in 3.5-7 A cells
#   BIG    50 atoms in dense cells: N grows and B does not
#   WIDE   10 atoms in 8 crystals: B grows and N does not
#   FULL   77 atoms and OVER 78, in three crystals: A (17, 5) -> BIG (50, 3) regrows to (62, 6); WIDE (10, 8) regrows to
#          (62 + 15, 8 + 2) = (77, 10) (capacity_after; asserted in the CPU test), so FULL lands exactly on the capacity and OVER
#          is one atom beyond it.  Should the rule change, the tests still pass and cover less.
#   GROW   84 atoms in 7 crystals: more atoms and more crystals than the 5 x 6-atom sample of test 3, and beyond the capacity in
#          both dimensions at that point of its schedule
BATCHES = {
    "A": dict(num_atoms=(3, 5, 2, 1, 6), cells=(_LOOSE, _LOOSE, _LOOSE, _ALONE, _LOOSE), timesteps=(1, 50, 20, 2, 77), seed=0),
    "BIG": dict(num_atoms=(3, 40, 7), cells=(_DENSE,) * 3, timesteps=(3, 60, 30), seed=6),
    "WIDE": dict(num_atoms=(1, 1, 2, 1, 1, 1, 1, 2), cells=(_LOOSE,) * 8, timesteps=(1, 12, 40, 7, 25, 33, 2, 18), seed=0),
    "FULL": dict(num_atoms=(30, 40, 7), cells=((5.0, 7.0), (5.5, 7.5), _DENSE), timesteps=(5, 45, 80), seed=1),
    "OVER": dict(num_atoms=(30, 41, 7), cells=((5.0, 7.0), (5.5, 7.5), _DENSE), timesteps=(70, 9, 35), seed=2),
    "GROW": dict(num_atoms=(12, 11, 13, 12, 10, 14, 12), cells=((4.5, 6.5),) * 7, timesteps=(1, 15, 30, 45, 60, 75, 100), seed=2),
}
SCHEDULE = ("A", "BIG", "A", "WIDE", "A", "FULL", "OVER", "A")   # test 1: one engine runs these in turn
SCORED_PAIR = (4, 6)             # test 3: the state random_state(12, [4, 6], 1) that is scored between training steps
SAMPLED = (6,) * 5               # test 3: the crystals of the sample
SCORED_FIRST = (12,) * 5         # test 4: the 60-atom state scored before the calibrating step; as many crystals as A, so A fits


def batch(name):
    return make_batch(**BATCHES[name])


def size_of(name):
    na = BATCHES[name]["num_atoms"]
    return sum(na), len(na)


def graph_facts(om64, om32, case):
    """What the float64 oracle `om64` makes of a make_batch result: the graph of the NOISED state (TR.noise_inputs) through
    OG.radius_graph_pbc(..., 5.0, 8).  Returns deg [N]; same_in_float32, whether the float32 oracle `om32` selects the same
    edges; off_radius, the smallest distance of any candidate pair from the radius; cut_gap, the smallest gap between the last neighbour kept and the first one dropped at a receiver with more than 8
    candidates; near_pairs, how many pairs of candidates of one receiver lie within 1e-4 A of each other, and mirror_pairs, how
    many of those are an atom's own two images at +c and -c (equal distances by symmetry, whatever the arithmetic)."""
    b, lattice0, timestep, noise = case
    nz = TR.noise_inputs(om64, b.X0.to(F64), b.A0, lattice0.to(F64), b.num_atoms, timestep, *(z.to(F64) for z in noise))
    lat = OG.lattice_from_params(nz["noisy_lengths"].to(F64), nz["angles"].to(F64))
    cart = OG.frac_to_cart_coords(nz["noisy_frac"].to(F64), lat, b.num_atoms)
    N = cart.shape[0]
    ei, cells = OG.radius_graph_pbc(cart, lat, b.num_atoms, RADIUS, K)[:2]
    # the same list in float32, on the float32 noising of the same draws: the set the library's float32 kernel has to find
    nz32 = TR.noise_inputs(om32, b.X0, b.A0, lattice0, b.num_atoms, timestep, *noise)
    lat32 = OG.lattice_from_params(nz32["noisy_lengths"], nz32["angles"])
    ei32, cells32 = OG.radius_graph_pbc(OG.frac_to_cart_coords(nz32["noisy_frac"], lat32, b.num_atoms), lat32, b.num_atoms, RADIUS, K)[:2]
    same = ei.shape == ei32.shape and torch.equal(ei, ei32) and torch.equal(cells.long(), cells32.long())
    ei_all, cell_all, _n, d_all, _d = OG.radius_graph_pbc(cart, lat, b.num_atoms, RADIUS + 0.5, 0)  # every candidate, uncapped
    gap, near, mirror = float("inf"), 0, 0
    for r in range(N):
        mine = (ei_all[1] == r) & (d_all <= RADIUS)
        d, order = d_all[mine].sort()
        if len(d) > K:
            gap = min(gap, float(d[K] - d[K - 1]))
        close = torch.nonzero(d[1:] - d[:-1] < 1e-4).flatten()
        near += len(close)
        snd, cel = ei_all[0][mine][order], cell_all[mine][order]
        mirror += sum(int(snd[i] == r and snd[i + 1] == r and bool((cel[i] == -cel[i + 1]).all())) for i in close.tolist())
    return SimpleNamespace(deg=torch.bincount(ei[1], minlength=N), off_radius=float((d_all - RADIUS).abs().min()) if len(d_all) else float("inf"),
                           cut_gap=gap, near_pairs=near, mirror_pairs=mirror, same_in_float32=same)
