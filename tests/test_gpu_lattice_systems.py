"""Lattice systems on the device: the tied length update and jump (arreau_reverse_step_tied, arreau_resample_jump_tied) against
the float64 restatements of arreau_amd/diffusion/lattice_systems.py and bitwise against the untied entry points for code 0; the
tied loop (arreau_sample_loop_tied) bitwise against arreau_sample_loop_resampled for an all-zero tie array, in eager, graph,
segment and prep-per-step forms; sample(lattice_system=...) with exact ties at every step in every sampler mode, the cells'
geometry, `None` as today's sampler, and generate.py.  Needs an MI355X: `-m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import lattice_systems as ls
from tests.sampling_helpers import (Case as _Case, S, T, any_model, assert_same_bits, dev, full_i32, fused_model,  # noqa: F401
                                     model_seed)

pytestmark = pytest.mark.gpu
TOL = 1e-5
COUNTS = [4, 7, 2, 150, 1, 5]  # ragged, one crystal above 128 atoms, one single atom
CODES = [0, 1, 2, 1, 2, 0]
# whole runs with free cells: the untrained synthetic model drives a 150-atom cell to non-finite values, tied or not (the
# resampled sampler's whole-run tests hold such a batch's cells fixed)
FREE_COUNTS = [4, 7, 2, 9, 1, 5]
MIXED = ["orthorhombic", "hexagonal", "cubic", "tetragonal", "rhombohedral", "triclinic"]  # tie codes CODES
SNR = 0.16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(_Case):
    COUNTS = COUNTS


assert [ls.TIE_CODES[name] for name in MIXED] == CODES


def _codes(dev, codes=CODES):
    return torch.as_tensor(codes, dtype=torch.int32, device=dev).contiguous()


def assert_tied(lengths, codes, what=""):
    """Tied axes bitwise equal: a = b for code 1, a = b = c for code 2."""
    le = lengths.detach().cpu()
    for b, code in enumerate(codes):
        if code is not None and code > 0:
            assert torch.equal(le[b, :code + 1], le[b, :1].expand(code + 1)), (what, b, le[b])


def _tables(om):
    return om.vp_alpha_bars.double().numpy(), om.vp_betas.double().numpy()


# -------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("stride", ["stride-1", "strided"])
def test_steps_against_the_restatement(dev, any_model, stride):
    """A three-step trajectory through the tied step (the caller's noise: the reference / device modes): every step against the
    float64 restatement; code-0 crystals, positions and species bitwise the untied step on the same inputs; tied axes equal."""
    m, om = any_model
    eng = m.engine()
    case = Case(dev, seed=17)
    B, N = case.B, case.N
    ab, betas = _tables(om)
    na = case.na.numpy()
    tie = _codes(dev)
    f, ty, le, lat = case.fresh()
    g = torch.Generator().manual_seed(4)
    t = T - 1
    eng.status(reset=True)
    for _ in range(3):
        s = t - 1 if stride == "stride-1" else max(1, t - 9)
        t_c, s_c = full_i32(B, t, dev), full_i32(B, s, dev)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        d = lambda v: v.to(dev).contiguous()
        z_l, z_f, u = d(torch.randn(B, 3, generator=g)), d(torch.randn(N, 3, generator=g)), d(torch.rand(N, S, generator=g))
        ref = [x.clone() for x in (f, ty, le, lat)]
        eng.reverse_step_to(*ref[:3], case.an, t_c, s_c, case.off, eps, logits, len0, z_l, z_f, u, ref[3])
        xt = le.cpu().double().numpy()
        eng.reverse_step_tied(f, ty, le, case.an, t_c, s_c, case.off, eps, logits, len0, z_l, z_f, u, lat, tie)
        x0 = len0.cpu().double().numpy() * na[:, None]
        want = ls.tied_update(xt, x0, z_l.cpu().double().numpy(), np.full(B, t), np.full(B, s), ab, betas, CODES)
        got = le.cpu().double().numpy()
        # float32 against float64: within 1e-5 of the crystal's magnitudes (its x0, x_t and result)
        scale = np.maximum(1.0, np.abs(np.concatenate([want, xt, x0], axis=1)).max(axis=1, keepdims=True))
        assert np.all(np.abs(got - want) <= TOL * scale), (t, s, np.abs(got - want).max())
        assert_tied(le, CODES, (t, s))
        assert_same_bits((f, ty), ref[:2], "positions and species are the untied step's")
        for b, code in enumerate(CODES):
            if code == 0:
                assert_same_bits((le[b], lat[b]), (ref[2][b], ref[3][b]), f"code-0 crystal {b}")
        t = s
    eng.check_status()


def test_jump_against_the_restatement(dev, any_model):
    m, om = any_model
    eng = m.engine()
    case = Case(dev, seed=19)
    B, N = case.B, case.N
    ab, _ = _tables(om)
    tie = _codes(dev)
    g = torch.Generator().manual_seed(8)
    d = lambda v: v.to(dev).contiguous()
    z_f, z_l, u = d(torch.randn(N, 3, generator=g)), d(torch.randn(B, 3, generator=g)), d(torch.rand(N, S, generator=g))
    s_c, t_c = np.array([0, 5, 12, 98, 30, 1]), np.array([37, 6, 60, 99, 31, 2])
    s_d, t_d = d(torch.as_tensor(s_c, dtype=torch.int32)), d(torch.as_tensor(t_c, dtype=torch.int32))
    eng.status(reset=True)
    ref = case.fresh()
    eng.resample_jump(*ref[:3], case.an, s_d, t_d, case.off, z_f, z_l, u, ref[3])
    f, ty, le, lat = case.fresh()
    eng.resample_jump(f, ty, le, case.an, s_d, t_d, case.off, z_f, z_l, u, lat, length_tie=tie)
    eng.check_status()
    want = ls.tied_jump(case.lengths.double().numpy(), z_l.cpu().double().numpy(), s_c, t_c, ab, CODES)
    got = le.cpu().double().numpy()
    assert np.all(np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want)))
    assert_tied(le, CODES, "jump")
    assert_same_bits((f, ty), ref[:2], "positions and species are the untied jump's")
    for b, code in enumerate(CODES):
        if code == 0:
            assert_same_bits((le[b], lat[b]), (ref[2][b], ref[3][b]), f"code-0 crystal {b}")
    # a fixed cell is held, tied or not
    f, ty, le, lat = case.fresh()
    fixed = le.clone()
    eng.resample_jump(f, ty, le, case.an, s_d, t_d, case.off, z_f, z_l, u, lat, fixed_lengths=fixed, length_tie=tie)
    assert torch.equal(le, fixed)


def test_bad_codes_are_flagged_and_untied(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    B, N = case.B, case.N
    g = torch.Generator().manual_seed(1)
    d = lambda v: v.to(dev).contiguous()
    z_l, z_f, u = d(torch.randn(B, 3, generator=g)), d(torch.randn(N, 3, generator=g)), d(torch.rand(N, S, generator=g))
    t_c, s_c = full_i32(B, 50, dev), full_i32(B, 49, dev)
    f, ty, le, lat = case.fresh()
    eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
    ref = case.fresh()
    eng.reverse_step_to(*ref[:3], case.an, t_c, s_c, case.off, eps, logits, len0, z_l, z_f, u, ref[3])
    for step in ("step", "jump"):
        eng.status(reset=True)
        f, ty, le, lat = case.fresh()
        bad = _codes(dev, [5, -1])
        if step == "step":
            eng.reverse_step_tied(f, ty, le, case.an, t_c, s_c, case.off, eps, logits, len0, z_l, z_f, u, lat, bad)
            assert_same_bits((f, ty, le, lat), ref, "bad codes count as 0")
        else:
            eng.resample_jump(f, ty, le, case.an, s_c, t_c, case.off, z_f, z_l, u, lat, length_tie=bad)
        assert eng.status()["flags"] == _hip.STATUS_BAD_TIE
        with pytest.raises(_hip.ArreauHipError, match="tie code"):
            eng.check_status()
    with pytest.raises(ValueError, match="length_tie"):
        eng.reverse_step_tied(f, ty, le, case.an, t_c, s_c, case.off, eps, logits, len0, z_l, z_f, u, lat, bad.long())


# -------------------------------------------------------------------------------------------------------------- 2
class Spy:
    """Records the lengths after every engine call that moves them (loop segments, tied steps, jumps)."""

    def __init__(self, eng, monkeypatch):
        self.states = []
        for name in ("sample_loop", "reverse_step_tied", "resample_jump"):
            def wrapped(*a, _orig=getattr(eng, name), **k):
                out = _orig(*a, **k)
                self.states.append(a[2].clone())  # (frac, types, lengths, ...) in all three
                return out
            monkeypatch.setattr(eng, name, wrapped)

    def assert_tied(self, codes):
        assert self.states
        for j, le in enumerate(self.states):
            assert_tied(le, codes, j)


def _cell_geometry(lattice):
    """Edge lengths and the angles (alpha: b, c; beta: a, c; gamma: a, b), in float64 from the float32 cells."""
    L = np.asarray(lattice, dtype=np.float64)
    n = np.linalg.norm(L, axis=2)
    cos = lambda i, j: np.einsum("bk,bk->b", L[:, i], L[:, j]) / (n[:, i] * n[:, j])
    return n, np.stack([cos(1, 2), cos(0, 2), cos(0, 1)], axis=1)


def _check_geometry(res, names):
    n, c = _cell_geometry(res.lattice)
    eps = 4e-6
    for b, name in enumerate(names):
        if name in ("cubic", "tetragonal", "orthorhombic"):
            assert np.all(np.abs(c[b]) <= eps), (name, c[b])
        if name in ("cubic", "rhombohedral"):
            assert np.all(np.abs(n[b] - n[b, 0]) <= eps * n[b, 0]), (name, n[b])
        if name in ("hexagonal", "tetragonal"):
            assert abs(n[b, 1] - n[b, 0]) <= eps * n[b, 0], (name, n[b])
        if name == "hexagonal":
            assert np.all(np.abs(c[b, :2]) <= eps) and abs(c[b, 2] + 0.5) <= eps, (name, c[b])
        if name == "rhombohedral":
            assert np.all(np.abs(c[b] - c[b, 0]) <= eps), (name, c[b])


def test_sample_mixed_systems(dev, fused_model, monkeypatch):
    m, _ = fused_model
    spy = Spy(m.engine(), monkeypatch)
    np.random.seed(1)
    res = m.sample(FREE_COUNTS, len(COUNTS), lattice_system=MIXED, seed=99)
    spy.assert_tied(CODES)
    _check_geometry(res, MIXED)
    assert np.isfinite(res.frac_x).all() and ((res.frac_x >= 0) & (res.frac_x <= 1)).all()
    spy.states.clear()
    res = m.sample(5, 4, lattice_system="cubic", seed=3, use_graph=True)
    spy.assert_tied([2] * 4)
    _check_geometry(res, ["cubic"] * 4)


def test_every_frame_is_tied(dev, fused_model, monkeypatch, tmp_path):
    from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting
    m, _ = fused_model
    spy = Spy(m.engine(), monkeypatch)
    res = m.sample(FREE_COUNTS, len(COUNTS), visualization_setting=VisualizationSetting.ALL_DETAILED, vis_name=str(tmp_path / "f"),
                   lattice_system=MIXED, seed=5, max_steps=6)
    assert len(spy.states) == 5  # one loop segment per frame
    spy.assert_tied(CODES)
    _check_geometry(res, MIXED)


def test_a_known_cell_takes_no_system(dev, fused_model):
    from arreau_amd.diffusion.conditioning import SampleCondition
    m, _ = fused_model
    tmpl = m.sample([4, 3], 2, seed=1, max_steps=2)
    cond = SampleCondition.from_sample_result(tmpl, fix_lattice=np.array([True, False]))
    with pytest.raises(ValueError, match="knows"):
        m.sample(condition=cond, lattice_system="cubic", seed=2)
    r = m.sample(condition=cond, lattice_system=[None, "cubic"], seed=2, max_steps=3)  # the known cell keeps its template
    assert np.isfinite(r.lattice).all()


# -------------------------------------------------------------------------------------------------------------- 3
def test_none_is_todays_sampler(dev, fused_model):
    m, _ = fused_model
    for noise in ("philox", "reference"):
        out = []
        for kw in ({}, dict(lattice_system=None)):
            torch.manual_seed(3)
            np.random.seed(3)
            r = m.sample([4, 7, 1], 3, seed=777, noise=noise, max_steps=6, **kw)
            out.append((r, torch.random.get_rng_state(), np.random.uniform()))
        a, b = out[0][0], out[1][0]
        assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.atomic_numbers, b.atomic_numbers)
        assert np.array_equal(a.lattice, b.lattice) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


@pytest.mark.parametrize("loop_prep", ["0", "1"])
def test_zero_ties_are_the_resampled_loop(dev, any_model, loop_prep, monkeypatch):
    monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    case, seed, k = Case(dev, seed=23, sampler_like=False), 5150, 6
    zeros = _codes(dev, [0] * case.B)
    for use_graph in (False, True):
        for opts in (dict(), dict(corrector=(1, SNR), resampling=(2, 3))):
            want = case.fresh()
            eng.sample_loop(*want[:3], case.an, case.off, 60, k, seed, None, want[3], use_graph=use_graph, **opts)
            got = case.fresh()
            eng.sample_loop(*got[:3], case.an, case.off, 60, k, seed, None, got[3], use_graph=use_graph, length_tie=zeros, **opts)
            assert_same_bits(got, want, (use_graph, opts))
    eng.check_status()


def test_tied_loop_forms_agree(dev, any_model, monkeypatch):
    """Graph replay = eager, one call = segments, ARREAU_LOOP_PREP=1 = the default form; a graph captured with the tie is never
    replayed without it."""
    m, _ = any_model
    eng = m.engine()
    case, seed, k = Case(dev, seed=29, sampler_like=False), 6161, 8
    ls.tie_lengths(case.lengths, CODES)
    tie = _codes(dev)
    runs = {}
    for name, use_graph, cuts, prep in (("eager", False, [k], "0"), ("graph", True, [k], "0"), ("segments", False, [3, 1, 4], "0"),
                                        ("prep", False, [k], "1"), ("prep-graph", True, [k], "1")):
        monkeypatch.setenv("ARREAU_LOOP_PREP", prep)
        got = case.fresh()
        t0 = 60
        for n in cuts:
            eng.sample_loop(*got[:3], case.an, case.off, t0, n, seed, None, got[3], use_graph=use_graph, length_tie=tie)
            t0 -= n
        runs[name] = got
        assert_tied(got[2], CODES, name)
    for name, got in runs.items():
        assert_same_bits(got, runs["eager"], name)
    monkeypatch.setenv("ARREAU_LOOP_PREP", "0")
    bufs = case.fresh()
    eng.sample_loop(*bufs[:3], case.an, case.off, 60, k, seed, None, bufs[3], use_graph=True, length_tie=tie)
    case.load(bufs)
    eng.sample_loop(*bufs[:3], case.an, case.off, 60, k, seed, None, bufs[3], use_graph=True)
    want = case.fresh()
    eng.sample_loop(*want[:3], case.an, case.off, 60, k, seed, None, want[3])
    assert_same_bits(bufs, want, "no stale tied graph")
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 4
MODES = {
    "num_steps": dict(num_steps=20),
    "corrector": dict(corrector_steps=1, max_steps=8),
    "resample": dict(num_steps=20, resample_passes=2, jump_length=5),
    "fixed_cell": dict(fixed_cell=True, max_steps=10),
    "reference": dict(noise="reference", max_steps=6, resample_passes=2, jump_length=3),
    "device": dict(noise="device", num_steps=10),
    # (fixed cells, as the resampled sampler's own whole-run test: free cells of the untrained synthetic model can degenerate)
    "graph-resample-corrector": dict(num_steps=12, resample_passes=2, jump_length=4, corrector_steps=1, use_graph=True,
                                     fixed_cell=True),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_ties_hold_in_every_mode(dev, any_model, mode, monkeypatch):
    m, _ = any_model
    spy = Spy(m.engine(), monkeypatch)
    counts = COUNTS if MODES[mode].get("fixed_cell") else FREE_COUNTS
    res = m.sample(counts, len(counts), lattice_system=MIXED, seed=11, **MODES[mode])  # (sample raises on a status flag)
    spy.assert_tied(CODES)
    _check_geometry(res, MIXED)
    assert np.isfinite(res.frac_x).all() and ((res.frac_x >= 0) & (res.frac_x <= 1)).all()


def test_ties_hold_with_a_condition(dev, fused_model, monkeypatch):
    from arreau_amd.diffusion.conditioning import SampleCondition
    m, _ = fused_model
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from oracle.geometry import lattice_from_params
    rng = np.random.RandomState(3)
    B, N = len(FREE_COUNTS), sum(FREE_COUNTS)
    cells = lattice_from_params(torch.tensor(rng.uniform(3, 6, (B, 3))), torch.tensor(np.deg2rad(rng.uniform(75, 105, (B, 3)))))
    na = np.asarray(FREE_COUNTS, dtype=np.int64)
    tmpl = SampleResult(frac_x=rng.uniform(0, 1, (N, 3)), atomic_numbers=rng.randint(1, S, N).astype(np.float64),
                        lattice=cells.numpy(), num_atoms=na, idx_start=np.cumsum(na) - na)
    cond = SampleCondition.from_sample_result(tmpl, fix_positions=np.arange(N) % 2 == 0, fix_species=np.arange(N) % 3 == 0)
    spy = Spy(m.engine(), monkeypatch)
    res = m.sample(condition=cond, lattice_system=MIXED, seed=4, num_steps=20)
    spy.assert_tied(CODES)
    _check_geometry(res, MIXED)


def test_ties_hold_on_the_make_train_shape(dev, monkeypatch):
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=S, seed=7, num_timesteps=T, hidden_dim=200).to(dev)
    spy = Spy(m.engine(), monkeypatch)
    res = m.sample(FREE_COUNTS, len(COUNTS), lattice_system=MIXED, seed=13, num_steps=15, use_graph=True)
    spy.assert_tied(CODES)
    _check_geometry(res, MIXED)


# -------------------------------------------------------------------------------------------------------------- 5
def test_generate_cubic(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "20", "--lattice_system", "cubic",
                        "--seed", "5", "--out", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == [6] * 5
    _check_geometry(res, ["cubic"] * 5)
