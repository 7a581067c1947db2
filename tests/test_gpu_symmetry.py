"""Space-group symmetry on the device: the symmetric step (arreau_reverse_step_sym) on a ragged batch that mixes specs with
unconstrained crystals, against the float64 restatement of arreau_amd/diffusion/symmetry.py and bitwise against the tied step
for the unconstrained crystals; sample(symmetry=...) symmetric in every frame of every sampler mode it supports; eager = graph
replay; `None` as today's sampler; bad tables flagged; generate.py --symops.

The step's VALUES (section 5 on): positions and species against the float64 restatements (step_positions, step_species) with
caller-made scores that are not symmetric, on the cases with reach of tests/symmetry_cases.py -- orbits of 96 and 192 atoms (the
second and third trip of the lane-strided loops of sym_orbit_ok and of the write-back), S = 124 (the second class of a lane, s1 =
lane + 64), 70 crystals (the second level of sym_atom_crystal's 64-ary search), stabilizers of order 1, 2, 4, 6, 8, 24 and 48, the
last step t = 1 -> 0; the members' draws unread, bit for bit; a P1 spec against the plain step; the loop (sym_philox_normal's
draws, the batch[i] form of the crystal index) against its steps one by one, bit for bit; bad tables at reach.
Needs an MI355X: `-m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import lattice_systems as ls
from arreau_amd.diffusion import symmetry as sy
from tests import symmetry_cases as C
from tests.sampling_helpers import S, T, any_model, assert_same_bits, dev, fused_model, full_i32, model_seed  # noqa: F401
from tests.symmetry_cases import GENS, PNMA_4C, R3M_3A_3B, ROCK_SALT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _specs():
    return {
        "p21c": sy.SymmetrySpec.general_positions(GENS["P21/c"], 2, "monoclinic"),
        "rocksalt": sy.SymmetrySpec.from_template(ROCK_SALT, GENS["Fm-3m"], "cubic"),
        "r3m-general": sy.SymmetrySpec.general_positions(GENS["R-3m"], 1, "hexagonal"),
        "r3m-3a3b": sy.SymmetrySpec.from_template(R3M_3A_3B, GENS["R-3m"], "hexagonal"),
        "pnma4c": sy.SymmetrySpec.from_template(PNMA_4C, GENS["Pnma"], "orthorhombic"),
    }


def _wrapped(d):
    d = np.abs(np.asarray(d, dtype=np.float64))
    d = d - np.floor(d)
    return np.minimum(d, 1 - d)


def assert_symmetric(specs, counts, frac, types, what="", tol=1e-6):
    """Every op g_m maps every atom j onto an atom within tol (wrapped); species constant per orbit, bitwise."""
    x = np.asarray(frac, dtype=np.float64)
    ty = np.asarray(types)
    first = np.concatenate([[0], np.cumsum(counts)])
    for b, spec in enumerate(specs):
        if spec is None:
            continue
        xb, tb = x[first[b]:first[b + 1]], ty[first[b]:first[b + 1]]
        for m in range(spec.order):
            gx = xb @ spec.R[m].T + spec.t[m]
            d = _wrapped(gx[:, None, :] - xb[None, :, :]).max(axis=2).min(axis=1)
            assert d.max() <= tol, (what, b, m, sy.format_symop(spec.R[m], spec.t[m]), d.max())
        for members in spec.orbits:
            assert np.all(tb[members] == tb[members[0]]), (what, b, tb[members])


def assert_cells(specs, lengths, angles, what=""):
    """Tied lengths bitwise equal, and the angles the system's."""
    le, an = np.asarray(lengths), np.asarray(angles, dtype=np.float64)
    for b, spec in enumerate(specs):
        if spec is None:
            continue
        code = ls.TIE_CODES[spec.lattice_system]
        if code:
            assert np.all(le[b, :code + 1] == le[b, 0]), (what, b, le[b])
        want = {"cubic": (90, 90, 90), "orthorhombic": (90, 90, 90), "hexagonal": (90, 90, 120)}.get(spec.lattice_system)
        if want is not None:
            assert np.allclose(an[b], np.deg2rad(want), atol=1e-6), (what, b, an[b])
        elif spec.lattice_system == "monoclinic":
            assert abs(an[b, 0] - np.pi / 2) < 1e-6 and abs(an[b, 2] - np.pi / 2) < 1e-6, (what, b, an[b])


class Frames:
    """Records (frac, types, lengths, angles) after every loop segment (sample_loop) of the engine."""

    def __init__(self, eng, monkeypatch):
        self.states = []

        def wrapped(*a, _orig=eng.sample_loop, **k):
            out = _orig(*a, **k)
            self.states.append(tuple(v.detach().cpu().clone() for v in a[:4]))
            return out
        monkeypatch.setattr(eng, "sample_loop", wrapped)

    def check(self, specs, counts):
        assert self.states
        for j, (f, ty, le, an) in enumerate(self.states):
            assert np.isfinite(f.numpy()).all() and ((f >= 0) & (f <= 1)).all(), j
            assert_symmetric(specs, counts, f.numpy(), ty.numpy(), j)
            assert_cells(specs, le.numpy(), an.numpy(), j)


# -------------------------------------------------------------------------------------------------------------- 1
def test_step_against_the_restatement(dev, fused_model):
    """Three steps (stride 1, then respaced) through arreau_reverse_step_sym with the caller's noise on a ragged batch of P2_1/c
    general positions, Fm-3m rock salt, R-3m general positions and Pnma 4c with unconstrained crystals: positions against the
    float64 restatement, members' species their leader's, unconstrained crystals and every cell bitwise the tied step's."""
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    m, _ = fused_model
    eng = m.engine()
    sp = _specs()
    specs = [sp["p21c"], None, sp["rocksalt"], sp["r3m-general"], None, sp["pnma4c"]]
    counts = [8, 5, 8, 36, 3, 4]
    B, N = len(specs), sum(counts)
    first = np.concatenate([[0], np.cumsum(counts)])
    rng = np.random.RandomState(7)
    frac = rng.uniform(0, 1, (N, 3))
    for b, s in enumerate(specs):
        if s is not None:
            frac[first[b]:first[b + 1]] = s.initial_positions(frac[first[b]:first[b + 1]]) % 1
    types = rng.randint(0, S, N)
    for b, s in enumerate(specs):  # species constant per orbit, as the sampler keeps them
        if s is not None:
            for members in s.orbits:
                types[first[b] + members] = types[first[b] + members[0]]
    names = [None if s is None else s.lattice_system for s in specs]
    np.random.seed(3)
    angles, codes = ls.resolve(names, B)
    lengths = ls.tie_lengths(rng.uniform(4, 8, (B, 3)), codes)
    d = lambda v, dt=torch.float32: torch.as_tensor(v, dtype=dt).to(dev).contiguous()
    f, ty, le, an = d(frac), d(types, torch.int32), d(lengths), d(angles)
    lat = torch.zeros(B, 3, 3, device=dev)
    off = crystal_offsets(torch.tensor(counts), dev)
    tie = d(codes, torch.int32)
    tables = sy.device_arrays(specs, off, dev)
    sig = m.state_dict()["diffusion_loss.pos_diffusion.sigmas"].float().cpu().double().numpy()
    g = torch.Generator().manual_seed(11)
    eng.status(reset=True)
    t = T - 1
    for s_next in (T - 2, T - 3, T - 12):
        t_c, s_c = full_i32(B, t, dev), full_i32(B, s_next, dev)
        eps, logits, len0 = eng.predict_scores(f, ty, le, an, t_c, off)
        z_l, z_f, u = d(torch.randn(B, 3, generator=g)), d(torch.randn(N, 3, generator=g)), d(torch.rand(N, S, generator=g))
        ref = [v.clone() for v in (f, ty, le, lat)]
        eng.reverse_step_tied(*ref[:3], an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, ref[3], tie)
        x_before = f.cpu().double().numpy()
        eng.reverse_step_sym(f, ty, le, an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, lat, tie, tables)
        got, got_t = f.cpu().double().numpy(), ty.cpu().numpy()
        e_np, z_np = eps.cpu().double().numpy(), z_f.cpu().double().numpy()
        for b, s in enumerate(specs):
            a0, a1 = first[b], first[b + 1]
            if s is None:
                assert_same_bits((f[a0:a1], ty[a0:a1]), (ref[0][a0:a1], ref[1][a0:a1]), f"unconstrained crystal {b}")
                continue
            want = s.step_positions(x_before[a0:a1], e_np[a0:a1], z_np[a0:a1], sig[t], sig[s_next])
            err = _wrapped(got[a0:a1] - want).max()
            assert err <= 1e-5, (t, b, err)
            for members in s.orbits:
                assert np.all(got_t[a0 + members] == got_t[a0 + members[0]]), (t, b)
        assert_same_bits((le, lat), (ref[2], ref[3]), "cells are the tied step's")
        assert_symmetric(specs, counts, got, got_t, t)
        t = s_next
    eng.check_status()


def test_bad_tables_are_flagged(dev, fused_model):
    """A leader out of range and an orbit member outside its crystal set ARREAU_STATUS_BAD_SYMMETRY; nothing is read out of
    bounds (every index is checked before it is followed) and the step completes."""
    from arreau_amd import _hip
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    m, _ = fused_model
    eng = m.engine()
    sp = _specs()
    specs, counts = [sp["p21c"], sp["pnma4c"]], [8, 4]
    B, N = 2, 12
    off = crystal_offsets(torch.tensor(counts), dev)
    g = torch.Generator().manual_seed(2)
    d = lambda v: v.to(dev).contiguous()
    for corrupt in ("leader", "member"):
        tables = sy.device_arrays(specs, off, dev)
        if corrupt == "leader":
            tables["leader"][3] = N + 100
        else:
            tables["orbit_atoms"][9] = 1  # an atom of crystal 0 in crystal 1's orbit
        f, ty = d(torch.rand(N, 3, generator=g)), torch.zeros(N, dtype=torch.int32, device=dev)
        le, an = d(torch.full((B, 3), 5.0)), d(torch.full((B, 3), float(np.pi / 2)))
        t_c, s_c = full_i32(B, 40, dev), full_i32(B, 39, dev)
        eps, logits, len0 = eng.predict_scores(f, ty, le, an, t_c, off)
        z_l, z_f, u = d(torch.randn(B, 3, generator=g)), d(torch.randn(N, 3, generator=g)), d(torch.rand(N, S, generator=g))
        eng.status(reset=True)
        eng.reverse_step_sym(f, ty, le, an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, torch.zeros(B, 3, 3, device=dev), None,
                             tables)
        assert eng.status(reset=True)["flags"] == _hip.STATUS_BAD_SYMMETRY, corrupt
        assert torch.isfinite(f).all()


# -------------------------------------------------------------------------------------------------------------- 2
MODES = {
    "eager": dict(use_graph=False, max_steps=12),
    "graph": dict(use_graph=True, max_steps=12),
    "respaced": dict(num_steps=20),
    "fixed_cell": dict(fixed_cell=True, max_steps=10),
    "frames": dict(max_steps=6, frames=True),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_frame_is_symmetric(dev, fused_model, monkeypatch, tmp_path, mode):
    from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting
    m, _ = fused_model
    sp = _specs()
    specs = [sp["p21c"], sp["rocksalt"], None, sp["r3m-3a3b"], sp["pnma4c"]]
    counts = [8, 8, 5, 6, 4]
    kw = dict(MODES[mode])
    if kw.pop("frames", False):
        kw.update(visualization_setting=VisualizationSetting.ALL_DETAILED, vis_name=str(tmp_path / "f"))
    frames = Frames(m.engine(), monkeypatch)
    res = m.sample(counts, len(counts), symmetry=specs, seed=21, **kw)  # (sample raises on a status flag)
    if mode == "frames":
        assert len(frames.states) == 5  # one loop segment per frame
    frames.check(specs, counts)
    assert_symmetric(specs, counts, res.frac_x, res.atomic_numbers, "result")


def test_one_spec_for_the_batch_and_constant_species(dev, fused_model, monkeypatch):
    m, _ = fused_model
    spec = _specs()["rocksalt"]
    frames = Frames(m.engine(), monkeypatch)
    from arreau_amd.diffusion.tools.atomic_number_table import SYMBOL_TO_Z
    symbol = {z: name for name, z in SYMBOL_TO_Z.items()}
    zs = [int(z) for z in m.z_table_zs.tolist()]
    res = m.sample(8, 3, symmetry=spec, seed=5, num_steps=15, use_constant_atomic_symbols=[symbol[zs[1]]] * 4 + [symbol[zs[2]]] * 4)
    frames.check([spec] * 3, [8] * 3)
    assert res.atomic_numbers.tolist() == ([zs[1]] * 4 + [zs[2]] * 4) * 3


def test_eager_and_graph_are_the_same_trajectory(dev, fused_model):
    m, _ = fused_model
    sp = _specs()
    specs, counts = [sp["p21c"], None, sp["rocksalt"], sp["pnma4c"]], [8, 5, 8, 4]
    out = []
    for use_graph in (False, True):
        torch.manual_seed(4)
        np.random.seed(4)
        out.append(m.sample(counts, 4, symmetry=specs, seed=77, max_steps=9, use_graph=use_graph))
    a, b = out
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.atomic_numbers, b.atomic_numbers)
    assert np.array_equal(a.lattice, b.lattice)


# -------------------------------------------------------------------------------------------------------------- 3
def test_none_is_todays_sampler(dev, fused_model):
    m, _ = fused_model
    for noise in ("philox", "reference"):
        out = []
        for kw in ({}, dict(symmetry=None), dict(symmetry=[None] * 3)):
            torch.manual_seed(3)
            np.random.seed(3)
            r = m.sample([4, 7, 1], 3, seed=777, noise=noise, max_steps=6, **kw)
            out.append((r, torch.random.get_rng_state(), np.random.uniform()))
        for r, rng, after in out[1:]:
            a = out[0][0]
            assert np.array_equal(a.frac_x, r.frac_x) and np.array_equal(a.atomic_numbers, r.atomic_numbers)
            assert np.array_equal(a.lattice, r.lattice) and torch.equal(out[0][1], rng) and out[0][2] == after


# -------------------------------------------------------------------------------------------------------------- 4
def test_generate_rock_salt(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    from arreau_amd.generate import save_sample_results
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    ops = tmp_path / "fm3m.txt"
    ops.write_text("# Fm-3m generators\n" + "\n".join(GENS["Fm-3m"]) + "\n")
    na = np.array([8])
    tmpl = save_sample_results(SampleResult(frac_x=ROCK_SALT.copy(), atomic_numbers=np.array([11.0] * 4 + [17.0] * 4),
                                            lattice=np.eye(3)[None] * 5.64, num_atoms=na, idx_start=np.zeros(1, dtype=np.int64)),
                               str(tmp_path / "tmpl.npz"))
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--num_crystals", "5", "--batch", "4", "--num_steps", "20", "--symops", str(ops), "--lattice_system", "cubic",
                        "--symmetry_template", tmpl, "--seed", "5", "--out", out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == [8] * 5
    spec = sy.SymmetrySpec.from_template(ROCK_SALT, GENS["Fm-3m"], "cubic")
    assert_symmetric([spec] * 5, [8] * 5, res.frac_x, res.atomic_numbers, "generate")


# -------------------------------------------------------------------------------------------------------------- 5
@pytest.fixture(scope="module", params=sorted(C.MODELS))
def value_model(dev, request, fused_model, model_seed):
    """(S, module, oracle model): fused_model (S = 12, one class per lane) and an S = 124 model, where lanes 0..59 hold a second
    class (the v1 path)."""
    if request.param == "S12":
        assert C.MODELS["S12"] == dict(S=S) and C.T == T
        return (S,) + tuple(fused_model)
    from arreau_amd.checkpoint import make_synthetic_model
    from tests.helpers import oracle_from_module
    kw = dict(C.MODELS[request.param])
    m = make_synthetic_model(seed=model_seed, num_timesteps=C.T, **kw).to(dev)
    return kw["S"], m, oracle_from_module(m, torch.float32)


def _on_device(dev, specs, counts, n_species, seed, cell=(5.0, 9.0)):
    """The on-site state of symmetry_cases.state on the device: (frac, types, lengths, lattice), angles, offsets, tie, tables."""
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    frac, types, lengths, angles, codes = C.state(specs, counts, n_species, seed, cell)
    d = lambda v, dt=torch.float32: torch.as_tensor(v, dtype=dt).to(dev).contiguous()
    off = crystal_offsets(torch.tensor(counts), dev)
    bufs = (d(frac), d(types, torch.int32), d(lengths), torch.zeros(len(counts), 3, 3, device=dev))
    return bufs, d(angles), off, d(codes, torch.int32), sy.device_arrays(specs, off, dev)


def _member_rows(tables):
    """The atoms that are members but not leaders of an orbit."""
    lead = tables["leader"].long()
    return (lead >= 0) & (lead != torch.arange(lead.numel(), device=lead.device))


@pytest.mark.parametrize("t,s", C.PAIRS)
@pytest.mark.parametrize("batch_name", ["wide", "deep"])
def test_step_values_against_the_restatements(dev, value_model, batch_name, t, s):
    """Three consecutive steps from t to s through arreau_reverse_step_sym with caller-made scores (symmetry_cases.scores: eps and
    logits random per atom, not symmetric) from an on-site state whose species include the mask class.  wide: orbits of 192 and
    96 atoms (three and two trips of the lane-strided loops), stabilizers of order 1, 2, 4, 6, 8, 24 and 48; deep: 70 crystals
    (the two-level crystal search).  S = 124: the second class per lane.  (1, 0): the last step, t = 1.
    Positions: SymmetrySpec.step_positions, 1e-5 wrapped.  Species: SymmetrySpec.step_species; a class may differ only where the
    float64 margin is below 1e-4, in at most one orbit of a step -- and the inputs hold no such orbit (asserted), so none may.
    The comparison's power is asserted on the same inputs: R for R^-1 and the leader's eps alone move every orbit that can
    show them (symmetry_cases.can_tell) by more than 10 x the bound; the leader's own logits and a member's uniforms change
    classes (counted over the steps; test_symmetry_cpu.py::test_the_step_cases_tell_the_rules_apart holds the counts).
    Bitwise: the members' rows of z_frac and u_types are not read (rules 2 and 5); unconstrained crystals and every cell are
    the tied step's (rule 7).
    (T-1, T-2) does NOT tell rule 5 apart: there the D3PM posterior keeps x_t (the mask class, or the class once taken) by a
    margin of about 3 whatever the logits, so leader-only logits or a member's uniforms change the class of 0 to 2 orbits only
    (printed, not asserted); the species rule is pinned by the other four pairs, which each assert at least 3 such orbits.  The
    positions (rules 1-4) are told apart at every pair.
    Measured on an MI355X: largest wrapped position error 4.79e-07 over the 20 cases (S = 124, deep, (1, 0)); no class differs."""
    n_species, m, om = value_model
    eng = m.engine()
    sig, q1t, qm = C.model_tables(om)
    specs, counts = C.batch(C.WIDE if batch_name == "wide" else C.DEEP)
    first = C.first_atoms(counts)
    B, N = len(counts), int(first[-1])
    tells = {b: C.can_tell(sp) for b, sp in enumerate(specs) if sp is not None}
    (f, ty, le, lat), an, off, tie, tables = _on_device(dev, specs, counts, n_species, C.step_seed(batch_name, t))
    members = _member_rows(tables)
    t_c, s_c = full_i32(B, t, dev), full_i32(B, s, dev)
    rng = np.random.RandomState(1000 + t)
    d = lambda v: torch.as_tensor(v).to(dev).contiguous()
    worst = by_logits = by_uniforms = left = 0
    eng.status(reset=True)
    for step in range(C.STEPS):
        sc = C.scores(rng, specs, counts, n_species, sigma_t=sig[t], sigma_s=sig[s])
        eps, logits, len0, z_l, z_f, u = (d(a) for a in sc)
        x_before, ty_before = f.cpu().double().numpy(), ty.cpu().numpy()
        tied = [v.clone() for v in (f, ty, le, lat)]
        eng.reverse_step_tied(*tied[:3], an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, tied[3], tie)
        other = [v.clone() for v in (f, ty, le, lat)]
        z2, u2 = z_f.clone(), u.clone()
        z2[members], u2[members] = 7.5, 0.125
        eng.reverse_step_sym(*other[:3], an, t_c, s_c, off, eps, logits, len0, z_l, z2, u2, other[3], tie, tables)
        eng.reverse_step_sym(f, ty, le, an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, lat, tie, tables)
        assert_same_bits((f, ty, le, lat), other, "the members' rows of z_frac and u_types are not read")
        assert_same_bits((le, lat), (tied[2], tied[3]), "cells are the tied step's")
        got, got_t = f.cpu().double().numpy(), ty.cpu().numpy()
        r = C.reference_step(specs, counts, x_before, ty_before, sc, t, s, sig, q1t, qm)
        excused = 0
        for b, sp in enumerate(specs):
            a0, a1 = first[b], first[b + 1]
            if sp is None:
                assert_same_bits((f[a0:a1], ty[a0:a1]), (tied[0][a0:a1], tied[1][a0:a1]), f"unconstrained crystal {b}")
                continue
            err = C.wrapped(got[a0:a1] - r.frac[b]).max()
            worst = max(worst, err)
            assert err <= C.TOL, (t, s, step, b, err)
            assert (r.rot[b][tells[b][0]] > C.TELL).all() and (r.lead[b][tells[b][1]] > C.TELL).all(), (step, b, r.rot[b], r.lead[b])
            assert (r.margins[b] >= C.MARGIN).all(), (step, b, r.margins[b].min())  # (the seeds hold no near-tie)
            for o, orbit in enumerate(sp.orbits):
                assert np.all(got_t[a0 + orbit] == got_t[a0 + orbit[0]]), (step, b, o)
                if got_t[a0 + orbit[0]] != r.classes[b][orbit[0]]:
                    assert r.margins[b][o] < C.MARGIN, ("a species differs away from a Gumbel near-tie", step, b, o, r.margins[b][o])
                    excused += 1
        assert excused == 0, (step, excused)
        by_logits, by_uniforms, left = by_logits + r.logit_orbits, by_uniforms + r.uniform_orbits, left + r.left
        assert_symmetric(specs, counts, got, got_t, (t, step))
    print(f"S={n_species} {batch_name} ({t},{s}): largest wrapped position error {worst:.3g}; classes the leader's own logits "
          f"would change {by_logits}, a member's uniforms {by_uniforms}; special-position leaders that left the cell {left}")
    assert left >= 3
    if t < C.T - 1:
        assert by_logits >= 3 and by_uniforms >= 3, (by_logits, by_uniforms)
    eng.check_status()


@pytest.mark.parametrize("t,s", C.PAIRS)
def test_p1_spec_is_the_plain_step(dev, value_model, t, s):
    """Orbits of one atom (P1, |G| = 1) next to unconstrained crystals (4 and 70 atoms): the species and cells are the tied
    step's bit for bit; the unconstrained crystals' positions too (rule 7: reverse_one_atom itself); the P1 crystals' positions
    are within 2^-22 wrapped -- the same fp32 expression in two inlined copies, which may contract one multiply-add
    differently.  Measured on an MI355X: 0 in all ten cases."""
    n_species, m, om = value_model
    eng = m.engine()
    sig = C.model_tables(om)[0]
    specs, counts = C.batch(["p1-5", 4, "p1-5", 70, "p1-5"])
    B, N = len(counts), sum(counts)
    (f, ty, le, lat), an, off, tie, tables = _on_device(dev, specs, counts, n_species, 40 + t)
    sc = C.scores(np.random.RandomState(50 + t), specs, counts, n_species, sigma_t=sig[t], sigma_s=sig[s])
    eps, logits, len0, z_l, z_f, u = (torch.as_tensor(a).to(dev).contiguous() for a in sc)
    t_c, s_c = full_i32(B, t, dev), full_i32(B, s, dev)
    tied = [v.clone() for v in (f, ty, le, lat)]
    start = f.clone()
    eng.status(reset=True)
    eng.reverse_step_tied(*tied[:3], an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, tied[3], tie)
    eng.reverse_step_sym(f, ty, le, an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, lat, tie, tables)
    assert_same_bits((ty, le, lat), tied[1:], "P1: species and cells")
    first = C.first_atoms(counts)
    p1 = np.zeros(N, dtype=bool)
    for b, sp in enumerate(specs):
        sl = slice(int(first[b]), int(first[b + 1]))
        if sp is None:
            assert_same_bits((f[sl],), (tied[0][sl],), f"unconstrained crystal {b}")
        else:
            p1[sl] = True
    assert p1.sum() == 15
    err = float(C.wrapped(f.cpu().double().numpy()[p1] - tied[0].cpu().double().numpy()[p1]).max())
    print(f"S={n_species} ({t},{s}): P1 against the plain step, largest wrapped difference {err:.3g}")
    assert err <= 2.0 ** -22
    assert not torch.equal(tied[0], start), "the step moved nothing"
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 6
SCHEDULES = {"stride-1": [5, 4, 3, 2, 1], "respaced": [99, 98, 80, 61, 40, 39, 12, 3, 2, 1]}  # both end with t = 1 -> 0


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_symmetric_loop_is_its_steps_one_by_one(dev, any_model, loop_prep, schedule, monkeypatch):
    """predict_scores + arreau_reverse_step_sym with arreau_philox_fill's draws (kinds 0, 1, 2), step by step, against
    arreau_sample_loop_sym over the same seed and timesteps: bit for bit in frac, types, lengths and lattice, eager and replayed
    as a hipGraph, at stride 1 and on a respaced schedule, both ending with the last step t = 1 -> 0, in both loop forms
    (ARREAU_LOOP_PREP=1 keeps the prep launch per step; the loop hands the kernel batch[i], the step searches the offsets).  The
    loop's leaders draw through sym_philox_normal: a wrong element index or kind there would show here.  Ragged batch with a
    crystal of 96 atoms (two trips of the lane-strided loops), cubic (a = b = c), hexagonal (a = b) and untied systems and
    unconstrained crystals."""
    from arreau_amd.diffusion import respacing
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    specs, counts = C.batch(C.LOOP)
    B, N = len(counts), sum(counts)
    seed, clip = 9988776655, 0.999
    sched = SCHEDULES[schedule]
    nxt = respacing.next_table(T, sched).to(dev) if schedule == "respaced" else None
    start, an, off, tie, tables = _on_device(dev, specs, counts, S, 61, cell=(7.0, 11.0))
    assert set(tie.tolist()) == {0, 1, 2}
    eng.status(reset=True)
    f, ty, le, lat = (v.clone() for v in start)
    for t, s in zip(sched, sched[1:] + [0]):
        t_c = full_i32(B, t, dev)
        eps, logits, len0 = eng.predict_scores(f, ty, le, an, t_c, off)
        eng.reverse_step_sym(f, ty, le, an, t_c, full_i32(B, s, dev), off, eps, logits, len0,
                             eng.philox_fill(seed, t, 0, 3 * B).view(B, 3), eng.philox_fill(seed, t, 1, 3 * N).view(N, 3),
                             eng.philox_fill(seed, t, 2, N * S).view(N, S), lat, tie, tables, clip)
    want = (f, ty, le, lat)
    assert not torch.equal(f, start[0]) and not torch.equal(ty, start[1])
    for use_graph in (False, True):
        got = [v.clone() for v in start]
        eng.sample_loop(*got[:3], an, off, sched[0], len(sched), seed, None, got[3], use_graph=use_graph, next_table=nxt,
                        lattice_clipmax=clip, length_tie=tie, symmetry=tables)
        assert_same_bits(got, want, ("one call", "graph" if use_graph else "eager"))
    got = [v.clone() for v in start]
    cuts = ((0, 2), (2, 5)) if schedule == "stride-1" else ((0, 3), (3, 4), (4, 10))  # (segments start at scheduled timesteps)
    for lo, hi in cuts:
        eng.sample_loop(*got[:3], an, off, sched[lo], hi - lo, seed, None, got[3], use_graph=hi - lo >= 3, next_table=nxt,
                        lattice_clipmax=clip, length_tie=tie, symmetry=tables)
    assert_same_bits(got, want, "segments")
    assert_symmetric(specs, counts, f.cpu().numpy(), ty.cpu().numpy(), "the loop's end")
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("corrupt", ["member 70 of 192", "member 150 of 192", "stabilizer row 40 of 48", "stabilizer row 1 of 2"])
def test_bad_tables_at_reach_are_flagged(dev, fused_model, corrupt):
    """A corrupt member in the second (index 70) and third (index 150) trip of sym_orbit_ok's lane-strided loop over a 192-atom
    orbit, and a corrupt stabilizer row (beyond the operations; negative), set ARREAU_STATUS_BAD_SYMMETRY; every other crystal
    comes out bit for bit as without the corruption.  Table validation: every index is checked before it is followed."""
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    names = ["fm3m-192l", 5, "fm3m-96k", "rocksalt", "p21c"]
    specs, counts = C.batch(names)
    first = C.first_atoms(counts)
    B, N = len(counts), int(first[-1])
    start, an, off, tie, tables = _on_device(dev, specs, counts, S, 71)
    bad = {k: v.clone() for k, v in tables.items()}
    n_ops = tables["rot"].shape[0]
    if corrupt.startswith("member"):
        where, hit = int(corrupt.split()[1]), 0
        assert tables["orbit_ptr"][:2].tolist() == [0, 192]
        bad["orbit_atoms"][where] = int(first[1])  # an atom of the unconstrained crystal 1
    else:
        hit = 3 if "48" in corrupt else 2
        o = int(tables["orbit"][first[hit]])
        h0, h1 = tables["stab_ptr"][o:o + 2].tolist()
        assert h1 - h0 == (48 if hit == 3 else 2)
        bad["stab_ops"][h0 + (40 if hit == 3 else 1)] = n_ops + 7 if hit == 3 else -1
    sc = C.scores(np.random.RandomState(72), specs, counts, S, sigma_t=0.05, sigma_s=0.04)
    eps, logits, len0, z_l, z_f, u = (torch.as_tensor(a).to(dev).contiguous() for a in sc)
    t_c, s_c = full_i32(B, 40, dev), full_i32(B, 39, dev)
    out = {}
    for name, tb in (("clean", tables), ("corrupt", bad)):
        f, ty, le, lat = (v.clone() for v in start)
        eng.status(reset=True)
        eng.reverse_step_sym(f, ty, le, an, t_c, s_c, off, eps, logits, len0, z_l, z_f, u, lat, tie, tb)
        out[name] = (f, ty, le, lat, eng.status(reset=True)["flags"])
    assert out["clean"][4] == 0 and out["corrupt"][4] == _hip.STATUS_BAD_SYMMETRY, corrupt
    assert torch.isfinite(out["corrupt"][0]).all()
    for b in range(B):
        if b != hit:
            sl = slice(int(first[b]), int(first[b + 1]))
            assert_same_bits([v[sl] for v in out["corrupt"][:2]], [v[sl] for v in out["clean"][:2]], (corrupt, "crystal", b))
    assert_same_bits(out["corrupt"][2:4], out["clean"][2:4], (corrupt, "cells"))
    sl = slice(int(first[hit]), int(first[hit + 1]))
    assert not torch.equal(out["corrupt"][0][sl], out["clean"][0][sl]), "a rejected orbit is not stepped as an orbit"
