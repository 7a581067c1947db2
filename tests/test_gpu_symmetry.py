"""Space-group symmetry on the device: the symmetric step (arreau_reverse_step_sym) on a ragged batch that mixes specs with
unconstrained crystals, against the float64 restatement of arreau_amd/diffusion/symmetry.py and bitwise against the tied step
for the unconstrained crystals; sample(symmetry=...) symmetric in every frame of every sampler mode it supports; eager = graph
replay; `None` as today's sampler; bad tables flagged; generate.py --symops.  Needs an MI355X: `-m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import lattice_systems as ls
from arreau_amd.diffusion import symmetry as sy
from tests.sampling_helpers import S, T, assert_same_bits, dev, fused_model, full_i32, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENS = {
    "P21/c": ["-x,y+1/2,-z+1/2", "-x,-y,-z"],
    "Pnma": ["-x+1/2,-y,z+1/2", "-x,y+1/2,-z", "-x,-y,-z"],
    "R-3m": ["-y,x-y,z", "y,x,-z", "-x,-y,-z", "x+2/3,y+1/3,z+1/3"],
    "Fm-3m": ["z,x,y", "-y,x,z", "-x,-y,-z", "x,y+1/2,z+1/2", "x+1/2,y,z+1/2"],
}
FCC = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
ROCK_SALT = np.concatenate([FCC, (FCC + 0.5) % 1])
PNMA_4C = np.array([[0.1377, 0.25, 0.3141], [0.3623, 0.75, 0.8141], [0.8623, 0.75, 0.6859], [0.6377, 0.25, 0.1859]])
R3M_3A_3B = np.array([[0, 0, 0], [2 / 3, 1 / 3, 1 / 3], [1 / 3, 2 / 3, 2 / 3],
                      [0, 0, 0.5], [2 / 3, 1 / 3, 5 / 6], [1 / 3, 2 / 3, 1 / 6]])


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
