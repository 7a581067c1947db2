"""The corners of the model shapes arreau_model_create accepts (include/arreau_hip.h) against the float64 oracle: where the
kernels switch to other code -- the vector read-out (readout_nodes_kernel) for S + 4 > 96 and both of its eps branches,
the register conv and the k < 8 edge tiles, a single layer (no calibration, no basis form, a one-wave MFMA read-out), the
shortest schedule, and the shape-general fp32 path at C = 4, C = 12 and C = 1024 -- plus the values just past each edge,
which must be refused before anything launches.  Two settings that are free rather than bounded, on both paths: layer_scale
present (every other shape) and absent (`-noLS`: a plane of ones in the node kernels, a backward pass with other launches), and
the radius, 5 everywhere else, at 3.5 and 7 (`-R3.5`, `-R7`) on states chosen so that the cut-off decides degrees and the
window's steep end is reached (RADIUS_STATES, _assert_cutoff_bites).  Every shape: scores (teacher-forced and own neighbour list), the kernel
families the library reports, one reverse step at t = 1 and t = T, one training step against oracle autograd, and a
short sample eager against graph replay.  Every fused shape runs twice: on the default kernels (fp16x3) and on the
full-range ones (bf16x6: `set_variant(3, 1)`, what the library falls back to when a model outgrows fp16), which are
documented as fp32-grade and so are held to the same bounds.  Needs an MI355X: run with `-m gpu`.

Measured on an MI355X when the -noLS and -R shapes were added (worst over t = 1 / t = T, given / own edges and both kernel sets;
in brackets the float32 oracle's own distance from float64 on the same inputs):
  shape               eps       logits    len0                gradient / its largest entry   families (default; full range)
  fused-noLS          2.8e-7    2.6e-6    1.7e-5 (9.2e-6)     3.6e-6 (2.9e-6)                fp16x3, fp16x3-16x16x32, conv 1 (2 at 256 atoms); bf16x6, bf16x6, conv 1
  fused-k5-noLS       3.2e-7    3.5e-6    2.3e-5 (2.7e-5)     2.7e-6 (2.9e-6)                fp16x3, fp16x3-16x16x32, conv 0; bf16x6, bf16x6, conv 0
  fused-L1-noLS       6.4e-7    6.2e-6    3.7e-5 (3.4e-5)     4.7e-6 (4.5e-6)                fp16x3, fp16x3-16x16x32, conv 1; bf16x6, bf16x6, conv 1
  general-C12-noLS    2.1e-7    2.4e-6    2.1e-5 (2.2e-5)     2.0e-5 (2.1e-5)                general-fp32-gemm throughout
  fused-R3.5          2.5e-7    3.4e-6    9.8e-6 (6.2e-6)     9.1e-6 (1.1e-5)                as fused-noLS
  fused-R7            2.7e-7    3.2e-6    1.8e-5 (1.1e-5)     3.4e-6 (3.3e-6)                as fused-noLS; edge_activation_bound 343
  general-C12-R3.5    1.4e-7    2.5e-6    3.0e-5 (2.3e-5)     7.0e-6 (9.3e-6)                general-fp32-gemm throughout"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import diffusion as OD
from oracle import geometry as OG
from oracle import sampler as OS
from oracle import training as TR
from tests.helpers import oracle_from_module, random_state, slots_from_edges
from tests.test_gpu_parity import TOL, _oracle_scores, _to_dev, pooled_bound
from tests.test_gpu_training import GRAD_TOL

pytestmark = pytest.mark.gpu

F64 = torch.float64

# id -> make_synthetic_model arguments (T = 20, L = 5, k = 8 and the fused C128 / D256 / W4 unless given)
SHAPES = {
    "fused-S2": dict(S=2),                                          # species loops: almost every lane idle; RO = 6
    "fused-S92-L8": dict(S=92, layers=8),                           # largest MFMA read-out: three full tiles, 512 threads
    "fused-S93": dict(S=93),                                        # first vector read-out shape; eps on idle columns
    "fused-S124-L8": dict(S=124, layers=8),                         # RO = 128, one thread walks the tile's eps, 1,024 threads, 64 KiB LDS
    "fused-L1": dict(S=12, layers=1),                               # one-wave MFMA read-out, no calibration, no basis form
    "fused-k1": dict(S=12, max_neighbors=1),                        # one slot per edge tile; register conv
    "fused-k5": dict(S=12, layers=3, max_neighbors=5),              # register conv at k < 8; training without the fused ConvNext
    "fused-T2": dict(S=12, num_timesteps=2),                        # the shortest schedule
    "general-C4": dict(S=12, hidden_dim=4, basis_dim=4, widening_factor=1, layers=2),     # one float4 per row; K = N = 4
    "general-C12-S124": dict(S=124, hidden_dim=12, basis_dim=20, widening_factor=3, layers=3, max_neighbors=3),  # C/4 = 3; RO = 128
    "general-C1024": dict(S=12, hidden_dim=1024, basis_dim=1024, widening_factor=1, layers=2),  # 64 KiB LDS launches; H = 1024
    # layer_scale absent (the reference's --layer_scale 0: no such parameter, no such state_dict key)
    "fused-noLS": dict(S=12, layer_scale=0.0),                      # a plane of ones in the node kernels; backward without d(out) written ahead
    "fused-k5-noLS": dict(S=12, layers=3, max_neighbors=5, layer_scale=0.0),   # register conv; training without the fused ConvNext
    "fused-L1-noLS": dict(S=12, layers=1, layer_scale=0.0),         # top-layer-only column sums
    "general-C12-noLS": dict(S=12, hidden_dim=12, basis_dim=20, widening_factor=3, layers=3, layer_scale=0.0),  # general forward / backward
    # a radius other than 5 (the states are chosen per radius: RADIUS_STATES)
    "fused-R3.5": dict(S=12, radius=3.5),                           # a cut-off window that bites; degree-starved receivers
    # edges longer than 5 A.  The range bound of arreau_model_create takes R^(powers of dist) = 7^3 for the largest monomial, where
    # radius 5 has 5^3.  For this checkpoint that monomial is the edge chain's largest bound, 343 (hidden units 53, basis 330;
    # at radius 5: 125, 27, 170) -- inside the fp16 range itself, far below the 64 x 65504 up to which a model starts on fp16x3 --
    # so the default case runs fp16x3 here too, and _assert_families checks that the library arrived at 343
    "fused-R7": dict(S=12, radius=7.0),
    "general-C12-R3.5": dict(S=12, hidden_dim=12, basis_dim=20, widening_factor=3, layers=3, radius=3.5),  # edge_rows_kernel; general forward
}


# (shape, arithmetic): the fused shapes on both kernel sets (a full-range case's id carries "-full-range"; the default
# cases keep the shape's id), the general shapes, which have no bf16x6 form, on their one path
CASES = [(name, arith) for name in SHAPES for arith in ("default", "full range") if arith == "default" or name.startswith("fused")]
CASE_IDS = [name if arith == "default" else name + "-full-range" for name, arith in CASES]


def _shape(name):
    kw = dict(SHAPES[name])
    kw.setdefault("num_timesteps", 20)
    S = kw.pop("S")
    hp = dict(S=S, T=kw["num_timesteps"], L=kw.get("layers", 5), k=kw.get("max_neighbors", 8), C=kw.get("hidden_dim", 128),
              radius=float(kw.get("radius", 5.0)), layer_scale=kw.get("layer_scale", 1e-6) != 0.0)
    hp["fused"] = hp["C"] == 128 and kw.get("basis_dim", 256) == 256 and kw.get("widening_factor", 4) == 4
    return S, kw, hp


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", params=CASES, ids=CASE_IDS)
def shape_model(dev, request):
    from arreau_amd.checkpoint import make_synthetic_model
    name, arith = request.param
    S, kw, hp = _shape(name)
    m = make_synthetic_model(S=S, seed=2024, trained_like=True, **kw).to(dev)
    full_range = arith == "full range"
    if full_range:
        m.engine().set_variant(3, 1)
    return SimpleNamespace(m=m, om=oracle_from_module(m, F64), om32=oracle_from_module(m, torch.float32),
                           name=name + (" full range" if full_range else ""), full_range=full_range, **hp)


def _concat(*states):
    frac, types, lengths, angles, na = zip(*states)
    return torch.cat(frac), torch.cat(types), torch.cat(lengths), torch.cat(angles), torch.cat(na)


# radius -> the cells and seeds of _ragged_state for a model of that radius, found on the CPU so that the cut-off matters and
# conditions a-e of _assert_cutoff_bites hold on the float64 oracle's own neighbour list.  "cells": the length ranges of the 33-,
# 1-, 5- and 3-atom crystals; "seeds": the state of the t = 1 and of the t = T test.
RADIUS_STATES = {
    3.5: dict(cells=((8.0, 10.0), (12.0, 14.0), (5.0, 8.0), (6.0, 8.0)), seeds={"t=1": 101, "t=T": 106}),
    7.0: dict(cells=((16.0, 20.0), (12.0, 14.0), (9.0, 12.0), (10.0, 12.0)), seeds={"t=1": 103, "t=T": 100}),
}


def _ragged_state(S, seed, radius=5.0):
    """Physical cells (no exact image ties, so both neighbour lists choose the same set): a crystal of 33 atoms (two
    32-atom read-out tiles, five 8-atom vector read-out tiles), a 1-atom crystal in a 12-14 A cell (no neighbour within the
    radius: fewer than k for every k), a 5-atom crystal and a sparse 3-atom crystal in a 10-12 A cell.  42 atoms: not a
    multiple of the 8 nodes per workgroup of the bf16x6 MLP kernel.  For a radius other than 5 the same four crystals in the
    cells of RADIUS_STATES (`seed` is then "t=1" or "t=T")."""
    if radius != 5.0:
        rs = RADIUS_STATES[radius]
        seed = rs["seeds"][seed]
        return _concat(*(random_state(S, [n], seed + i, cell=cell) for i, (n, cell) in enumerate(zip((33, 1, 5, 3), rs["cells"]))))
    return _concat(random_state(S, [33], seed), random_state(S, [1], seed + 1, cell=(12.0, 14.0)),
                   random_state(S, [5], seed + 2), random_state(S, [3], seed + 3, cell=(10.0, 12.0)))


def _cutoff_facts(state, radius, k):
    """What the float64 oracle's neighbour list makes of `state` at `radius` and k (no GPU): the degrees, the selected
    distances, the degrees a radius of 5 would give, the smallest distance of a candidate pair from the radius, the smallest gap
    between the last neighbour kept and the first one dropped at a receiver with more than k candidates, and the smallest spacing
    of lattice planes of any cell."""
    frac, _types, lengths, angles, na = state
    lat = OG.lattice_from_params(lengths.to(F64), angles.to(F64))
    cart = OG.frac_to_cart_coords(frac.to(F64), lat, na)
    N = frac.shape[0]
    ei, _c, _n, dist, _d = OG.radius_graph_pbc(cart, lat, na, radius, k)
    ei5 = OG.radius_graph_pbc(cart, lat, na, 5.0, k)[0]
    # every candidate pair out to beyond the larger radius, uncapped (max_neighbors = 0)
    ei_all, _c, _n, d_all, _d = OG.radius_graph_pbc(cart, lat, na, max(radius, 5.0) + 0.5, 0)
    gap = float("inf")
    for r in range(N):
        d = d_all[(ei_all[1] == r) & (d_all <= radius)].sort().values
        if len(d) > k:
            gap = min(gap, float(d[k] - d[k - 1]))
    cross = torch.stack([torch.linalg.cross(lat[:, (i + 1) % 3], lat[:, (i + 2) % 3]) for i in range(3)], 1)
    spacing = torch.linalg.det(lat).abs()[:, None] / cross.norm(dim=-1)
    return SimpleNamespace(deg=torch.bincount(ei[1], minlength=N), dist=dist, deg5=torch.bincount(ei5[1], minlength=N),
                           off_radius=float((d_all - radius).abs().min()), cut_gap=gap, spacing=float(spacing.min()))


def _assert_cutoff_bites(state, radius, k, tag):
    """The conditions on a state for a model whose radius is not 5, on the float64 oracle's list alone, before anything is
    compared: a. a receiver with 1 <= degree < k and one with degree k; b. a selected edge with dist / radius >= 0.9, where
    the window 1 - 28 u^6 + 48 u^7 - 21 u^8 is a difference of large terms; c. below 5: a receiver that a radius of 5 would
    give more neighbours (a pair in (radius, 5] selected in place of nothing), above 5: a selected edge longer than 5 A; d. no
    candidate pair within 1e-3 A of the radius and none within 1e-4 A of the last neighbour kept at the cut of the k nearest,
    so that the float32 and the float64 list agree; e. every cell's three plane spacings at least the radius: the 27 images the
    list looks at then hold every pair in range."""
    f = _cutoff_facts(state, radius, k)
    assert bool(((f.deg >= 1) & (f.deg < k)).any()) and bool((f.deg == k).any()), (tag, "a", f.deg.tolist())
    assert float(f.dist.max()) / radius >= 0.9, (tag, "b", float(f.dist.max()))
    if radius < 5.0:
        assert bool((f.deg5 > f.deg).any()), (tag, "c", f.deg.tolist(), f.deg5.tolist())
    else:
        assert float(f.dist.max()) > 5.0, (tag, "c", float(f.dist.max()))
    assert f.off_radius >= 1e-3 and f.cut_gap >= 1e-4, (tag, "d", f.off_radius, f.cut_gap)
    assert f.spacing >= radius, (tag, "e", f.spacing)
    return f


def _engine_scores(sm, dev, state, t, teacher_forced):
    """(HIP scores, float64 oracle scores, float32 oracle scores on the same edges, degrees of the oracle's neighbour list)"""
    eps_o, logits_o, len0_o, (ei, dists, direction, _c, _l) = _oracle_scores(sm.om, *state, t, dtype=F64)
    want32 = _oracle_scores(sm.om32, *state, t, edges=(ei, dists.float(), direction.float()))[:3]
    N, B = state[0].shape[0], len(state[4])
    f, ty, le, an, off = _to_dev(dev, *state)
    t_c = torch.full((B,), t, device=dev, dtype=torch.int32)
    deg, src, sdir, sdist = slots_from_edges(ei, dists, direction, N, sm.k)
    edges = tuple(x.to(dev).contiguous() for x in (deg, src, sdir, sdist)) if teacher_forced else None
    got = sm.m.engine().predict_scores(f, ty, le, an, t_c, off, edges=edges)
    return got, (eps_o, logits_o, len0_o), want32, deg


def _assert_scores_close_to_float64(got, want64, want32, tag, atoms_per_crystal=20):
    """Against float64: eps and logits within assert_scores_close's 1e-5 bounds; len0, a sum over the crystal's atoms, within
    pooled_bound plus twice the float32 oracle's own distance to float64 (the idiom of test_gpu_training.py at the bench size).  That distance is what a 33-atom crystal at t = T
    costs any float32 evaluation: measured 1.4e-5 .. 7.5e-5 for the float32 oracle at |len0| = 5 .. 51 (C = 4 the most),
    1.0e-5 .. 8.5e-5 for the library (C = 4 the most); at t = 1 the float32 oracle stays below 1e-5.  Returns the errors against float64."""
    (eps, logits, len0), (eps_o, logits_o, len0_o) = got, want64
    e = float((eps.detach().cpu().double() - eps_o).abs().max())
    l = float((logits.detach().cpu().double() - logits_o).abs().max())
    g = float((len0.detach().cpu().double() - len0_o).abs().max())
    g32 = float((want32[2].double() - len0_o).abs().max())
    assert e <= TOL * max(1.0, float(eps_o.abs().max())), (tag, "eps", e)
    assert l <= TOL * max(1.0, float(logits_o.abs().max()) / 8.0), (tag, "logits", l, float(logits_o.abs().max()))
    assert g <= pooled_bound(len0_o, atoms_per_crystal) + 2 * g32, (tag, "len0", g, g32, float(len0_o.abs().max()))
    return e, l, g


def _expected_families(sm, basis_form=False):
    if not sm.fused:
        return dict(edge_kernel="general-fp32-gemm", mlp_kernel="general-fp32-gemm", conv_variant=5, readout_kernel=5)
    if sm.full_range:  # no basis form without the fp16x3 edge kernel (score_plan.h: basis_form): K pair at k = 8, else register
        return dict(edge_kernel="bf16x6", mlp_kernel="bf16x6", conv_variant=1 if sm.k == 8 else 0,
                    readout_kernel=1 if sm.S + 4 <= 96 else 0)
    # conv: 2 basis form (k = 8, L >= 2, enough receivers), 1 streamed K pair (k = 8), 0 register form (any k)
    conv = (2 if basis_form and sm.L >= 2 else 1) if sm.k == 8 else 0
    return dict(edge_kernel="fp16x3", mlp_kernel="fp16x3-16x16x32", conv_variant=conv,
                readout_kernel=1 if sm.S + 4 <= 96 else 0)


def _assert_families(sm, basis_form=False):
    st = sm.m.engine().status()
    want = _expected_families(sm, basis_form)
    assert {k: st[k] for k in want} == want, (sm.name, st)
    assert st["flags"] == 0, (sm.name, st)
    if sm.fused and sm.radius == 7.0:  # the radius has reached the range bound (arreau_model_create: R^(powers of dist)): see SHAPES
        assert st["edge_activation_bound"] == 343.0, (sm.name, st)


# ------------------------------------------------------------------------------------------- a. scores, b. kernel families
@pytest.mark.parametrize("t_end", ["t=1", "t=T"])
def test_scores_match_float64_oracle(dev, shape_model, t_end):
    sm = shape_model
    t = 1 if t_end == "t=1" else sm.T
    if sm.radius == 5.0:
        state = _ragged_state(sm.S, 10 if t == 1 else 20)
    else:  # a state in which this radius cuts: checked on the float64 oracle's list before anything runs
        state = _ragged_state(sm.S, t_end, sm.radius)
        facts = _assert_cutoff_bites(state, sm.radius, sm.k, (sm.name, t_end))
    worst, worst32 = np.zeros(3), np.zeros(3)
    for teacher_forced in (True, False):
        got, want, want32, deg = _engine_scores(sm, dev, state, t, teacher_forced)
        assert int(deg.min()) == 0 and bool((deg < sm.k).any())  # the isolated atom, and atoms short of k neighbours
        assert len(deg) % 8 != 0
        if sm.radius != 5.0:
            assert torch.equal(deg.long(), facts.deg)
        worst32 = np.maximum(worst32, [float((a.double() - b).abs().max()) for a, b in zip(want32, want)])
        errs = _assert_scores_close_to_float64(got, want, want32, (sm.name, t, "given edges" if teacher_forced else "own edges"),
                                               atoms_per_crystal=33)
        worst = np.maximum(worst, errs)
        _assert_families(sm)
    # sampler-start state (lengths ~ N(0, 1), frac ~ N(0, 1)): tiny cells whose images tie exactly, so teacher-forced only
    state = random_state(sm.S, [9, 2, 17], 30 + t, sampler_like=True)
    got, want, want32, _ = _engine_scores(sm, dev, state, t, True)
    worst = np.maximum(worst, _assert_scores_close_to_float64(got, want, want32, (sm.name, t, "sampler-like")))
    _assert_families(sm)
    print(f"\n[{sm.name} {t_end}] worst against float64: eps {worst[0]:.2e} logits {worst[1]:.2e} len0 {worst[2]:.2e}; the float32 "
          f"oracle's own on the ragged state: eps {worst32[0]:.2e} logits {worst32[1]:.2e} len0 {worst32[2]:.2e}")


def test_basis_form_when_enough_receivers(dev, shape_model, monkeypatch):
    """With the receiver threshold at its floor (240) a batch of 256 atoms takes the basis form of the message path where
    the shape has it (fused, k = 8, L >= 2) and keeps the K pair / register conv elsewhere; scores against float64 either way."""
    sm = shape_model
    monkeypatch.setenv("ARREAU_BASIS_MIN_RECEIVERS", "0")
    state = random_state(sm.S, [32] * 8, 40)
    got, want, want32, _ = _engine_scores(sm, dev, state, max(1, sm.T // 2), True)
    errs = _assert_scores_close_to_float64(got, want, want32, (sm.name, "256 atoms"), atoms_per_crystal=32)
    _assert_families(sm, basis_form=True)
    print(f"\n[{sm.name} 256 atoms] families {_expected_families(sm, True)}; worst against float64: "
          f"eps {errs[0]:.2e} logits {errs[1]:.2e} len0 {errs[2]:.2e}")


# ------------------------------------------------------------------------------------------- c. one reverse step
@pytest.mark.parametrize("t_end", ["t=1", "t=T"])
def test_reverse_step_matches_float64_oracle(dev, shape_model, t_end):
    """test_gpu_parity.py: test_reverse_step_matches_oracle at this shape's S and T, against the float64 oracle."""
    _check_reverse_step(shape_model, dev, 1 if t_end == "t=1" else shape_model.T)


def _check_reverse_step(sm, dev, t):
    """One reverse step of the model `sm` (attributes m, om = float64 oracle, S) at timestep t against the float64 oracle."""
    S = sm.S
    frac, types, lengths, angles, na = random_state(S, [4, 7, 1, 33], 50 + t, sampler_like=True)
    frac = frac % 1
    N, B = frac.shape[0], len(na)
    g = torch.Generator().manual_seed(t)
    eps = torch.randn(N, 3, generator=g)
    logits = torch.randn(N, S, generator=g) * 2
    len0 = torch.randn(B, 3, generator=g)
    noise = OS.StepNoise(torch.randn(B, 3, generator=g), torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g))
    d64 = lambda v: v.to(F64)
    noise64 = OS.StepNoise(*(d64(z) for z in (noise.z_lattice, noise.z_frac, noise.u_types)))
    f_o, ty_o, len_o, lat_o = OS.reverse_step(sm.om, d64(frac), types, d64(lengths), d64(angles), na,
                                              (d64(eps), d64(logits), d64(len0)), t, noise64)
    post_o = OD.d3pm_q_posterior_logits(sm.om.q_one_step_transposed, sm.om.q_mats, d64(logits), types, torch.full((N,), t))
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    d = lambda v: v.to(dev).contiguous()
    f, ty, le, an = d(frac.clone()), d(types.to(torch.int32)), d(lengths.clone()), d(angles)
    lat = torch.zeros(B, 3, 3, device=dev)
    t_c = torch.full((B,), t, device=dev, dtype=torch.int32)
    sm.m.engine().reverse_step(f, ty, le, an, t_c, crystal_offsets(na, dev), d(eps), d(logits), d(len0),
                               d(noise.z_lattice), d(noise.z_frac), d(noise.u_types), lat)
    np.testing.assert_allclose(le.cpu().double().numpy(), len_o.numpy(), atol=TOL * max(1.0, float(len_o.abs().max())), rtol=0)
    np.testing.assert_allclose(lat.cpu().double().numpy(), lat_o.numpy(), atol=TOL * max(1.0, float(lat_o.abs().max())), rtol=0)
    df = (f.cpu().double() - f_o).abs()
    df = torch.minimum(df, 1 - df)  # a value within rounding of 0 or 1 may land on the other side of the seam
    assert df.max() <= TOL
    # discrete update: identical unless the two best classes are closer than the float32 noise floor
    scale = 0.2 if t == 1 else 1.0
    u = torch.clip(d64(noise.u_types), 1e-6, 1.0)
    top2 = (post_o + (-torch.log(-torch.log(u))) * scale).topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert decided.float().mean() > 0.9
    assert torch.equal(ty.cpu().long()[decided], ty_o[decided])
    assert sm.m.engine().status()["flags"] == 0


# ------------------------------------------------------------------------------------------- d. one training step
def _training_inputs(S, T, radius=5.0):
    """(batch, lattice0, timestep, noise) of a 4-crystal training step of 15 atoms, every random draw injected.  For a radius
    above 5 the cells (and the draw that becomes the cell at t = T) grow by (radius + 1) / 6: see the comment on the lengths."""
    grow = max(1.0, (radius + 1.0) / 6.0)
    rng = np.random.RandomState(8)
    num_atoms = [3, 5, 1, 6]
    B, N = len(num_atoms), sum(num_atoms)
    # cells of 6-8 A (no lattice vector shorter than the 5 A radius): no atom sees its own images, which come in pairs at
    # exactly equal distances -- at k < 8 such a tie at the cut decides the graph by rounding, differently in float32 and float64
    lengths = torch.tensor(rng.uniform(6.0, 8.0, size=(B, 3)), dtype=torch.float32) * grow
    angles = torch.tensor(np.deg2rad(rng.uniform(75, 105, size=(B, 3))), dtype=torch.float32)
    lattice0 = OG.lattice_from_params(lengths, angles)
    batch = SimpleNamespace(X0=torch.tensor(rng.uniform(0, 1, size=(N, 3)), dtype=torch.float32),
                            A0=torch.tensor(rng.randint(0, S - 1, size=N)), L0=lattice0.reshape(-1, 3),
                            num_atoms=torch.tensor(num_atoms))
    timestep = torch.tensor([1, T, max(1, T // 2), T][:B])
    g = torch.Generator().manual_seed(4)
    # z_lengths: at t = T the noised cell IS this draw (alpha_bar ~ 0), so it is drawn as cell lengths of 6-8 A rather than N(0, 1),
    # which would give sub-angstrom cells full of exactly tied periodic images
    noise = (torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g), (6.0 + 2.0 * torch.rand(B, 3, generator=g)) * grow)
    return batch, lattice0, timestep, noise


def _assert_cutoff_bites_in_training(sm, batch, lattice0, timestep, noise):
    """The training step of a model whose radius is not 5 builds its graph on the noised batch: on the float64 oracle's noising
    of it, a receiver short of k neighbours, conditions b to e of _assert_cutoff_bites, and how many edges the list has."""
    nz = TR.noise_inputs(sm.om, batch.X0.to(F64), batch.A0, lattice0.to(F64), batch.num_atoms, timestep, *(z.to(F64) for z in noise))
    state = (nz["noisy_frac"], nz["noisy_types"], nz["noisy_lengths"], nz["angles"], batch.num_atoms)
    f = _cutoff_facts(state, sm.radius, sm.k)
    assert bool(((f.deg >= 1) & (f.deg < sm.k)).any()), (sm.name, "a", f.deg.tolist())
    assert float(f.dist.max()) / sm.radius >= 0.9, (sm.name, "b", float(f.dist.max()))
    assert bool((f.deg5 > f.deg).any()) if sm.radius < 5.0 else float(f.dist.max()) > 5.0, (sm.name, "c", f.deg.tolist(), f.deg5.tolist())
    assert f.off_radius >= 1e-3 and f.cut_gap >= 1e-4, (sm.name, "d", f.off_radius, f.cut_gap)
    assert f.spacing >= sm.radius, (sm.name, "e", f.spacing)
    return int(f.deg.sum())


def _oracle_autograd(om, dtype, batch, lattice0, timestep, noise):
    """(loss, {parameter name: gradient}) of torch autograd through the oracle `om`'s loss in `dtype`; `om` is left as it was"""
    for v in om.sd.values():
        if v.is_floating_point() and v.numel() > 0:
            v.requires_grad_(True)
            v.grad = None
    try:
        loss_o = TR.diffusion_loss(om, batch.X0.to(dtype), batch.A0, lattice0.to(dtype), batch.num_atoms, timestep,
                                   *(z.to(dtype) for z in noise))
        loss_o.backward()
        want = {"model." + k: v.grad.clone() for k, v in om.sd.items() if v.requires_grad and v.grad is not None}
    finally:
        for v in om.sd.values():
            v.requires_grad_(False)
            v.grad = None
    return loss_o.detach(), want


def test_training_step_matches_float64_oracle_autograd(dev, shape_model):
    """Under "full range" the training forward leaves the fused ConvNext launch for bf16x6 products (train_net.hip: fwd_mode 2)."""
    sm = shape_model
    batch, lattice0, timestep, noise = _training_inputs(sm.S, sm.T, sm.radius)
    if sm.radius != 5.0:
        _assert_cutoff_bites_in_training(sm, batch, lattice0, timestep, noise)
    mm = copy.deepcopy(sm.m)  # (the copy packs its own engine: the arithmetic is chosen on it)
    for layer in mm.model.interaction_layers:
        layer.conv.callibrated.fill_(True)
    if sm.full_range:
        mm.engine(for_training=True).set_variant(3, 1)
    loss = mm.training_step(batch, timestep=timestep, noise=noise)
    loss_o, want = _oracle_autograd(sm.om, F64, batch, lattice0, timestep, noise)
    loss32, want32 = _oracle_autograd(sm.om32, torch.float32, batch, lattice0, timestep, noise)  # (printed, not part of any bound)
    loss_err = abs(float(loss.detach()) - float(loss_o))
    assert loss_err <= TOL * max(1.0, abs(float(loss_o))), (sm.name, float(loss), float(loss_o))
    got = {n: p.grad for n, p in mm.named_parameters() if p.grad is not None}
    params = {n for n, p in mm.named_parameters() if p.requires_grad and p.numel() > 0}
    checked, worst = set(), (0.0, 0.0, "")
    for name, w in want.items():
        if w.numel() == 0:
            continue
        err = float((got[name].cpu().double() - w).abs().max())
        scale = max(float(w.abs().max()), 1e-7)
        assert err <= GRAD_TOL * scale + 1e-7, (sm.name, name, err, scale)
        worst = max(worst, (err / scale, float((want32[name].double() - w).abs().max()) / scale, name))
        checked.add(name)
    assert checked == params, (sm.name, sorted(params ^ checked))
    # 9 tensors in front of the layers, two read-out tensors per layer, and per layer ten with layer_scale, nine without it
    assert len(checked) == 9 + sm.L * (2 + 9 + int(sm.layer_scale)), (sm.name, len(checked))
    assert sm.layer_scale == any(n.endswith("layer_scale") for n in got), (sm.name, sorted(got))
    assert mm._engine.status()["flags"] == 0
    print(f"\n[{sm.name} training] loss {float(loss_o):.4f}, error {loss_err:.2e} (float32 oracle {abs(float(loss32) - float(loss_o)):.2e}); "
          f"worst gradient error relative to its largest entry {worst[0]:.2e}, float32 oracle autograd {worst[1]:.2e} ({worst[2]}), "
          f"{len(checked)} tensors")


# ------------------------------------------------------------------------------------------- e. a short sample
def test_sample_eager_and_graph_replay_agree(dev, shape_model):
    """The whole sampling loop, eager and as hipGraph replay: the same bits, finite, no flags.  (At T = 2 the loop has two
    steps, fewer than the three arreau_sample_loop captures a graph for: both runs are eager there.)"""
    sm = shape_model
    from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(11); np.random.seed(11)
        runs.append(sm.m.sample(6, 5, VisualizationSetting.NONE, False, use_graph=use_graph, seed=123))
        st = sm.m.engine().status()
        assert st["flags"] == 0 and st["edge_kernel"] == _expected_families(sm)["edge_kernel"], (sm.name, st)
    a, b = runs
    assert np.isfinite(a.frac_x).all() and np.isfinite(a.lattice).all()
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.atomic_numbers, b.atomic_numbers)
    assert np.array_equal(a.lattice, b.lattice)


# ------------------------------------------------------------------------------------------- the edges of the contract
@pytest.mark.parametrize("kw,message", [
    (dict(hidden_dim=6), "hidden_dim must be a multiple of 4 in 4..1024"),
    (dict(hidden_dim=1028, widening_factor=1), "hidden_dim must be a multiple of 4 in 4..1024"),
    (dict(basis_dim=1028), "basis_dim must be a multiple of 4 in 4..1024"),
    (dict(hidden_dim=520, widening_factor=2), "widening_factor \\* hidden_dim must be at most 1024"),
    (dict(S=125), "num_atomic_states must be in 2..124"),
    (dict(layers=9), "bad num_layers"),
    (dict(max_neighbors=0), "max_neighbors must be in 1..8"),
    (dict(max_neighbors=9), "max_neighbors must be in 1..8"),
    (dict(num_timesteps=1), "num_timesteps"),
], ids=["C6", "C1028", "D1028", "C520-W2", "S125", "L9", "k0", "k9", "T1"])
def test_shapes_just_past_each_edge_are_refused(dev, kw, message):
    """arreau_model_create refuses the value just past each edge of the accepted range with its message, before it allocates
    or launches anything (its checks come first)."""
    from arreau_amd import _hip
    from arreau_amd.checkpoint import make_synthetic_model
    from arreau_amd.engine import HipEngine
    kw = dict(kw)
    S = kw.pop("S", 12)
    kw.setdefault("num_timesteps", 20)
    try:
        m = make_synthetic_model(S=S, seed=1, trained_like=False, **kw)
    except ValueError:
        return  # refused by the Python side before any engine exists
    with pytest.raises(_hip.ArreauHipError, match=message):
        HipEngine(m, dev)
