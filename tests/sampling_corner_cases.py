"""The cases of the sampling-step corner tests (test_sampling_corners_cpu.py, test_gpu_sampling_corners.py): one ragged batch of 67
crystals on which every crystal holds its own pair of timesteps, models with S = 124, 2 and 12 classes and T = 2, caller-made
scores, and the float64 references of every step entry point.  Built and guarded on the CPU; torch and numpy only.

What the batch reaches that the 4-to-6-crystal scaffolding of tests/sampling_helpers.py does not:

    per-crystal pairs   the atom part finds each atom's crystal by a wave-wide 64-ary search of the offsets; with one (t, s) for
                        all crystals a wrong crystal gives the same sigma, Qbar rows and t == 1 branch.  Here neighbouring
                        crystals always differ (PAIRS dealt round-robin), and one-atom crystals put boundaries on adjacent atoms.
    67 crystals         the stand-alone lattice part deals four lanes per crystal, 64 crystals per workgroup: a second workgroup
                        with three live crystals, a partly live group of four, waves 1-3, two levels of the crystal search.
    tie codes           0, 1, 2 cycling with period 3 (coprime to the pair periods), so tied crystals sit past lane 23 and past
                        crystal 64.
    S = 124             two classes per lane (lane + 64): the mask class sits in the second class of lane 59.
    130 atoms           the last crystal keeps the large-crystal pooling in.

A reference is a float64 restatement evaluated once per distinct pair on the whole batch and gathered per crystal (a step
treats crystals independently); `gather` with another crystal index per atom gives what a wrong lookup would have computed.
"""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import torch

from arreau_amd.diffusion import corrector as pc
from arreau_amd.diffusion import inversion as iv
from arreau_amd.diffusion import lattice_systems as ls
from arreau_amd.diffusion import resampling as rs
from oracle import geometry as OG
from oracle import sampler as OS
from tests.helpers import random_state
from tests.symmetry_cases import MODELS as _SYM_MODELS

T = 100
MODEL_SEED = 4321
# make_synthetic_model arguments: only the diffusion tables matter to a step, so S = 124 takes the small accepted network of
# symmetry_cases.MODELS; the others are fused shapes test_gpu_model_shapes.py accepts (fused-S2, the default, fused-T2)
MODELS = {"S124": dict(_SYM_MODELS["S124"], num_timesteps=T), "S2": dict(S=2, num_timesteps=T), "S12": dict(S=12, num_timesteps=T),
          "S12-T2": dict(S=12, num_timesteps=2)}

COUNTS = [(1, 2, 3, 5, 4)[b % 5] for b in range(66)] + [130]
B, N = len(COUNTS), sum(COUNTS)
assert (B, N) == (67, 326)
FIRST = np.concatenate([[0], np.cumsum(COUNTS)])
CRYSTAL = np.repeat(np.arange(B), COUNTS)
CODES = [b % 3 for b in range(B)]
CLIP = 0.999
SNR = 0.16
MARGIN = 1e-3  # 10 x symmetry_cases.MARGIN: no atom of any case is closer to a Gumbel tie in float64, so the device's classes must be equal

# (t, s) of the reverse steps; read as (s, t) climbs by the inversion (s >= 1) and the jump
REVERSE = [(99, 98), (99, 80), (50, 10), (7, 1), (2, 1), (1, 0), (60, 59), (100, 99)]
KINDS = ("plain", "reverse", "invert", "jump", "corrector")
# the GPU bound on positions of each kind (wrapped), from the kind's own restatement test
POS_TOL = {"plain": 1e-5, "reverse": 1e-5, "invert": 1e-5, "jump": 1e-6, "corrector": 1e-5}


def pair_list(model, kind):
    """The distinct pairs of a kind on a model, in dealing order: (t, s) for plain (s = t - 1) and reverse, (s, t) for invert and
    jump, (t, t) for the corrector (one timestep)."""
    if MODELS[model]["num_timesteps"] == 2:
        return {"plain": [(2, 1), (1, 0)], "reverse": [(2, 1), (1, 0)], "invert": [(1, 2)],
                "jump": [(0, 1), (0, 2), (1, 2), (0, 2)], "corrector": [(2, 2), (1, 1)]}[kind]
    ts = [99, 50, 7, 2, 1, 60, 100]  # the timesteps of REVERSE, each once: neighbours differ at stride 1 too
    return {"plain": [(t, t - 1) for t in ts], "reverse": list(REVERSE), "invert": [(s, t) for t, s in REVERSE if s > 0],
            "jump": [(s, t) for t, s in REVERSE], "corrector": [(t, t) for t in ts]}[kind]


def pair_index(model, kind):
    """The index into pair_list of every crystal: round-robin, turned so that the 130-atom crystal holds the list's first pair
    (a high level, where a wrong lookup moves an atom by more than the bound; at levels below 10 sigma is about 0.001)."""
    n = len(pair_list(model, kind))
    return (np.arange(B) - (B - 1)) % n


def pairs_per_crystal(model, kind):
    """(first [B], second [B]) int64 arrays of the pairs the crystals hold."""
    p = np.asarray(pair_list(model, kind), dtype=np.int64)[pair_index(model, kind)]
    return p[:, 0], p[:, 1]


@functools.lru_cache(maxsize=None)
def model_and_oracle(name):
    """(module on the CPU, oracle model with float32 tables) of a name of MODELS."""
    from arreau_amd.checkpoint import make_synthetic_model
    from tests.helpers import oracle_from_module
    m = make_synthetic_model(seed=MODEL_SEED, **MODELS[name])
    return m, oracle_from_module(m, torch.float32)


def in_float64(om):
    """The oracle model with its tables as float64 tensors (the float32 values, exactly)."""
    return dataclasses.replace(om, **{k: getattr(om, k).double() for k in
                                      ("ve_sigmas", "vp_alpha_bars", "vp_betas", "q_one_step_transposed", "q_mats")})


def inputs(model, kind, seed=0):
    """The state, scores and draws of one launch, on the host in float32 (as _inputs of test_gpu_ddim_sampling.py; with seed 0
    every case's float64 margins reach MARGIN, which test_sampling_corners_cpu.py asserts):
    eps ~ 0.3 N(0,1), logits ~ 2 N(0,1), len0 ~ U(0.5, 1.5), standard draws z_l [B,3], z_f [N,3], u [N,S]; x_t uniform over the
    classes with every third atom on the mask class S - 1.  plain / reverse / jump: a sampler-like state (positions and lengths
    ~ N(0,1), as the step tests' Case); invert / corrector: positions in the cell, some at the wrap, lengths in 2..6 (as
    test_gpu_inversion.py).  corrector: eps of the size the network is trained to, sigma of the crystal's timestep, zero on
    crystal 65; `known` marks 40 % of the atoms and every atom of crystal 64."""
    S = MODELS[model]["S"]
    g = torch.Generator().manual_seed(7919 * seed + 1000 + KINDS.index(kind))
    frac, _, lengths, angles, na = random_state(S, COUNTS, 50 + seed, sampler_like=True)
    v = SimpleNamespace(S=S, seed=seed, na=na, angles=angles)
    v.eps = torch.randn(N, 3, generator=g) * 0.3
    v.logits = torch.randn(N, S, generator=g) * 2.0
    v.len0 = torch.rand(B, 3, generator=g) + 0.5
    v.z_l, v.z_f, v.u = torch.randn(B, 3, generator=g), torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g)
    v.x_t = torch.randint(0, S, (N,), generator=g)
    v.x_t[::3] = S - 1
    if kind in ("invert", "corrector"):
        frac = torch.rand(N, 3, generator=g)
        edge = torch.tensor([[0.0, 1e-7, 1 - 6e-8], [1 - 1e-6, 5e-7, 0.999999], [1e-5, 0.5, 1 - 1e-5]])
        frac[:3], frac[-2:] = edge, edge[:2]
        lengths = torch.rand(B, 3, generator=g) * 4 + 2
    if kind == "corrector":
        sig = model_and_oracle(model)[1].ve_sigmas[torch.as_tensor(pairs_per_crystal(model, kind)[0])]
        v.eps = torch.randn(N, 3, generator=g) * sig[torch.as_tensor(CRYSTAL)].unsqueeze(-1).float()
        v.eps[CRYSTAL == 65] = 0.0
        v.known = torch.rand(N, generator=g) < 0.4
        v.known[torch.as_tensor(CRYSTAL == 64)] = True
    v.frac, v.lengths = frac, lengths
    return v


# ---- the float64 references, each on the whole batch at one pair ------------------------------------------------------------
def _np(v):
    return v.double().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)


def reverse_at(om, v, t, s, variant, eta=None, codes=None):
    """One reverse step of the whole batch from t to s: dict(frac [N,3], types [N], margin [N], lengths [B,3]) in float64.
    variant "plain": oracle.sampler.reverse_step (s = t - 1); "sched": the respaced step's restatement, its lengths by
    lattice_systems.tied_update when `codes` are given; "eta": the eta step's restatement (ddim.ve_step / length_step)."""
    from tests.test_gpu_ddim_sampling import _d3pm_post, _step_cpu as eta_step
    from tests.test_gpu_respaced_sampling import _step_cpu as sched_step
    scores = (v.eps, v.logits, v.len0)
    if variant == "eta":
        fr, ty, le, _, margin = eta_step(om, v.frac, v.x_t, v.lengths, v.angles, v.na, scores, t, s, v.z_l, v.z_f, v.u, eta, codes)
        return dict(frac=_np(fr), types=ty.numpy(), margin=_np(margin), lengths=_np(le))
    fr, ty, le, _, margin = sched_step(om, v.frac, v.x_t, v.lengths, v.angles, v.na, scores, t, s, v.z_l, v.z_f, v.u)
    if variant == "plain":
        assert s == t - 1
        d = lambda a: a.double()
        fr, ty2, le, _ = OS.reverse_step(in_float64(om), d(v.frac), v.x_t, d(v.lengths), d(v.angles), v.na, tuple(d(a) for a in scores),
                                         t, OS.StepNoise(d(v.z_l), d(v.z_f), d(v.u)))
        assert torch.equal(ty, ty2), "the two float64 restatements of the species rule disagree"
    elif codes is not None:
        ab, betas = _np(om.vp_alpha_bars), _np(om.vp_betas)
        x0 = _np(v.len0) * v.na.numpy()[:, None]
        le = ls.tied_update(_np(v.lengths), x0, _np(v.z_l), np.full(B, t), np.full(B, s), ab, betas, codes, clipmax=CLIP)
    return dict(frac=_np(fr), types=ty.numpy(), margin=_np(margin), lengths=_np(le))


def invert_at(om, v, s, t):
    """One inversion step from s up to t: positions, lengths and the derived float32 bound of the length move."""
    sig, ab = _np(om.ve_sigmas), _np(om.vp_alpha_bars)
    x0 = _np(v.len0) * v.na.numpy()[:, None]
    return dict(frac=iv.invert_positions(sig, _np(v.frac), _np(v.eps), s, t), lengths=iv.invert_lengths(ab, _np(v.lengths), x0, s, t),
                bound=iv.length_error_bound(ab, _np(v.lengths), x0, s, t))


def jump_margin(om, types, s, t, u):
    """The top-two margin of resampling.jump_species' arg-max, per atom."""
    rows = _np(om.q_mats)[t - s - 1, np.asarray(types, np.int64)]
    val = np.log(rows + rs.D3PM_EPS) - np.log(-np.log(np.clip(_np(u), rs.D3PM_EPS, 1.0)))
    top = np.sort(val, axis=1)
    return top[:, -1] - top[:, -2]


def jump_at(om, v, s, t, codes=None):
    """One jump from s up to t (resampling.jump; the lengths by lattice_systems.tied_jump when `codes` are given)."""
    sig, ab, qm = _np(om.ve_sigmas), _np(om.vp_alpha_bars), _np(om.q_mats)
    f, ty, le = rs.jump(_np(v.frac), v.x_t.numpy(), _np(v.lengths), np.full(B, s), np.full(B, t), v.na.numpy(), sig, ab, qm,
                        _np(v.z_f), _np(v.z_l), _np(v.u))
    if codes is not None:
        le = ls.tied_jump(_np(v.lengths), _np(v.z_l), np.full(B, s), np.full(B, t), ab, codes)
    return dict(frac=f, types=ty, margin=jump_margin(om, v.x_t.numpy(), s, t, v.u), lengths=le)


def corrector_at(om, v, t, masked):
    return dict(frac=pc.corrector_move(_np(v.frac), _np(v.eps), _np(v.z_f), float(om.ve_sigmas[t]), SNR, v.na.numpy(),
                                       known=v.known.numpy() if masked else None))


def per_pair(model, kind, fn):
    """fn(first, second) at every distinct pair of the kind: a list in pair_list's order (equal pairs evaluated once)."""
    done = {}
    return [done.setdefault(p, fn(*p)) if p not in done else done[p] for p in pair_list(model, kind)]


def gather(results, model, kind, crystal_of_atom=None):
    """The per-pair results (per_pair) gathered per crystal: rows of [N, ...] arrays by the pair of each atom's crystal, rows of
    [B, ...] arrays by the crystal's own pair.  `crystal_of_atom` [N]: the crystal whose pair each atom takes (default: its own;
    another crystal's restates a wrong lookup)."""
    idx_c = pair_index(model, kind)
    idx_a = idx_c[CRYSTAL if crystal_of_atom is None else np.asarray(crystal_of_atom)]
    out = {}
    for key in results[0]:
        stack = np.stack([np.asarray(r[key]) for r in results])
        out[key] = stack[idx_a, np.arange(N)] if stack.shape[1] == N else stack[idx_c, np.arange(B)]
    return out


def cell_of(lengths, angles):
    """The float64 cell of lengths [B,3] (numpy) and the case's angles."""
    return OG.lattice_from_params(torch.as_tensor(lengths), angles.double()).numpy()


def wrapped(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    d = d - np.floor(d)
    return np.minimum(d, 1 - d)


def neighbour_holds_another_pair(model, kind, shift):
    """Per atom: whether crystal (own + shift) mod B holds another pair than the atom's own crystal."""
    pl, idx = pair_list(model, kind), pair_index(model, kind)
    other = (CRYSTAL + shift) % B
    return np.array([pl[idx[a]] != pl[idx[b]] for a, b in zip(CRYSTAL, other)]), other
