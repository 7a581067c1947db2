"""Conditioned sampling (structure completion) on the device: known positions, species and cells held to a template inside
the update kernels (arreau_sample_loop_conditioned; rules in include/arreau_hip.h).  Against a CPU restatement of the rules
on top of the oracle's step, segment / graph / prep-form invariance, no change to unconditioned runs, independence of the
unconditioned crystals, the end state of whole runs, and the generate.py template driver.  Needs an MI355X: `-m gpu`."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import geometry as OG
from oracle import sampler as OS
from tests.sampling_helpers import Case as _Case, S, T, any_model, dev, fused_model, wrapped_dist  # noqa: F401

pytestmark = pytest.mark.gpu
TOL = 1e-5
COUNTS = [4, 7, 2, 150]  # ragged, one crystal above 128 atoms; crystal 2 is never conditioned
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model_seed():
    return 1234


class Case(_Case):
    """A ragged sampler-like state and a mixed condition: half the atoms of crystals 0 and 3 placed, crystal 1's species and
    some of crystal 3's known, the cells of crystals 0 and 1 known.  Crystal 2 is unconditioned."""
    COUNTS = COUNTS

    def __init__(self, dev, seed=5):
        super().__init__(dev, seed)
        B, N = self.B, self.N
        rng = np.random.RandomState(seed + 100)
        first = np.concatenate([[0], np.cumsum(COUNTS)])
        local = np.arange(N) - first[self.crystal]
        self.pm = ((self.crystal == 0) | (self.crystal == 3)) & (local % 2 == 0)
        self.tm = (self.crystal == 1) | ((self.crystal == 3) & (local % 3 == 1))
        self.lm = np.array([True, True, False, False])
        self.x0 = rng.uniform(0, 1, (N, 3)).astype(np.float32)
        self.a0 = rng.randint(0, S - 1, N).astype(np.int32)
        self.l0 = rng.uniform(3, 6, (B, 3)).astype(np.float32)
        self.g0 = np.deg2rad(rng.uniform(75, 105, (B, 3))).astype(np.float32)
        self.angles = self.angles.clone()
        self.angles[torch.as_tensor(self.lm)] = torch.as_tensor(self.g0)[torch.as_tensor(self.lm)]  # rule 3 (host side)
        self.an = self.angles.to(dev).contiguous()

    def cond(self, pm=None, tm=None, lm=None, x0=None):
        d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=self.dev, dtype=dt).contiguous()
        pm = self.pm if pm is None else pm
        tm = self.tm if tm is None else tm
        lm = self.lm if lm is None else lm
        return dict(x0=d(self.x0 if x0 is None else x0, torch.float32), pos_mask=d(pm.astype(np.uint8), torch.uint8),
                    a0=d(self.a0, torch.int32), type_mask=d(tm.astype(np.uint8), torch.uint8), l0=d(self.l0, torch.float32),
                    len_mask=d(lm.astype(np.uint8), torch.uint8))


def _run(eng, case, t_start, n_steps, seed, cond, use_graph=False, init=True, const=None, state=None):
    f, ty, le, lat = case.fresh() if state is None else state
    if init and cond is not None:
        eng.condition_initial_state(f, ty, le, t_start, seed, cond)
    eng.sample_loop(f, ty, le, case.an, case.off, t_start, n_steps, seed, const, lat, use_graph=use_graph, condition=cond)
    return f, ty, le, lat


def _rules_cpu(om, eng, seed, t, case, frac, types, lengths):
    """Rules 1, 2 and 4 on a CPU state of timestep tau = t - 1 (Philox key t; t = t_start + 1 for the initial state)."""
    frac, types, lengths = frac.clone(), types.clone(), lengths.clone()
    tau = t - 1
    pm, tm, lm = (torch.as_tensor(m) for m in (case.pm, case.tm, case.lm))
    x0, l0 = torch.as_tensor(case.x0), torch.as_tensor(case.l0)
    if tau == 0:
        kf, kl = torch.remainder(x0, 1.0), l0
    else:
        z3 = eng.philox_fill(seed, t, 3, 3 * case.N).view(case.N, 3).cpu()
        z4 = eng.philox_fill(seed, t, 4, 3 * case.B).view(case.B, 3).cpu()
        ab = float(om.vp_alpha_bars[tau])
        kf = torch.remainder(x0 + float(om.ve_sigmas[tau]) * z3, 1.0)
        kl = math.sqrt(ab) * l0 + math.sqrt(1.0 - ab) * z4
    frac[pm] = kf[pm]
    lengths[lm] = kl[lm].to(lengths.dtype)
    types[tm] = torch.as_tensor(case.a0).long()[tm]
    return frac, types, lengths


# ----------------------------------------------------------------------------------------------------------------- 1, 6
def test_conditioned_steps_against_a_cpu_restatement(dev, any_model):
    """Six conditioned steps (the initial state included), each from the device's state: the oracle's predict_scores +
    reverse_step with the device's Philox draws of kinds 0-2, then the replacement rules with the draws of kinds 3-4."""
    m, om = any_model
    eng = m.engine()
    case, seed = Case(dev), 1357911
    batch = torch.as_tensor(case.crystal)
    cond = case.cond()
    f, ty, le, lat = case.fresh()
    eng.condition_initial_state(f, ty, le, T - 1, seed, cond)
    f_o, ty_o, le_o = _rules_cpu(om, eng, seed, T, case, case.frac, case.types, case.lengths)  # rule 5
    assert float(wrapped_dist(f.cpu(), f_o).max()) <= 1e-6 and torch.equal(ty.cpu().long(), ty_o)
    assert float((le.cpu() - le_o).abs().max()) <= 1e-6 * max(1.0, float(le_o.abs().max()))
    for t in range(T - 1, T - 7, -1):
        frac, types, lengths = f.cpu(), ty.cpu().long(), le.cpu()
        scores = OS.predict_scores(om, frac, F.one_hot(types, S), torch.full((case.N,), t), case.na, lengths, case.angles, batch)
        noise = OS.StepNoise(*(eng.philox_fill(seed, t, k, n).view(*shp).cpu()
                               for k, n, shp in ((0, 3 * case.B, (case.B, 3)), (1, 3 * case.N, (case.N, 3)),
                                                 (2, case.N * S, (case.N, S)))))
        f_o, ty_o, le_o, _ = OS.reverse_step(om, frac, types, lengths, case.angles, case.na, scores, t, noise)
        f_o, ty_o, le_o = _rules_cpu(om, eng, seed, t, case, f_o, ty_o, le_o)
        lat_o = OG.lattice_from_params(le_o, case.angles)
        eng.sample_loop(f, ty, le, case.an, case.off, t, 1, seed, None, lat, condition=cond)
        # unknown coordinates: the VE update wraps x - eps (s_t^2 - s_{t-1}^2) into [0, 1); where this random-init model's eps
        # is large that value is far from [0, 1) and carries its own fp32 rounding, so each coordinate is allowed 1e-5
        # relative to it, plus the scores' own bound (assert_scores_close) carried through the update
        s2, sp2 = float(om.ve_sigmas[t]) ** 2, float(om.ve_sigmas[t - 1]) ** 2
        pre = frac - scores[0] * (s2 - sp2)
        bound = TOL * pre.abs().clamp(min=1.0) + TOL * max(1.0, float(scores[0].abs().max())) * (s2 - sp2)
        dd = (f.cpu() - f_o).abs()
        dd = torch.minimum(dd, 1 - dd)
        assert (dd <= bound).all(), (t, float(dd.max()), float(pre.abs().max()))
        assert float((le.cpu() - le_o).abs().max()) <= TOL * max(1.0, float(le_o.abs().max())), t
        assert float((lat.cpu() - lat_o).abs().max()) <= TOL * max(1.0, float(lat_o.abs().max())), t
        pm, tm = torch.as_tensor(case.pm), torch.as_tensor(case.tm)
        assert float(wrapped_dist(f.cpu()[pm], f_o[pm]).max()) <= 1e-6, t  # the replaced components: the rules, to fp32 rounding
        assert torch.equal(ty.cpu().long()[tm], ty_o[tm]), t
        assert int((ty.cpu().long() != ty_o).sum()) <= 1, t  # a Gumbel arg-max within rounding of a tie may go either way
    eng.check_status()


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_segments_graph_and_condition_change(dev, any_model, loop_prep, monkeypatch):
    """Six steps in one call = six one-step calls = the hipGraph replay, bit for bit; a second call with another condition
    is captured anew (never the first condition's graph); a run that ends at timestep 1 leaves the template exactly."""
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=7), 24681357
    cond = case.cond()
    ref = _run(eng, case, T - 1, 6, seed, cond)
    state = case.fresh()
    eng.condition_initial_state(*state[:3], T - 1, seed, cond)
    for t in range(T - 1, T - 7, -1):
        _run(eng, case, t, 1, seed, cond, init=False, state=state)
    for a, b in zip(state, ref):
        assert torch.equal(a, b), "segments"
    for a, b in zip(_run(eng, case, T - 1, 6, seed, cond, use_graph=True), ref):
        assert torch.equal(a, b), "graph"
    x1 = np.ascontiguousarray(case.x0[::-1])
    cond2 = case.cond(x0=x1)
    ref2 = _run(eng, case, T - 1, 6, seed, cond2)
    got2 = _run(eng, case, T - 1, 6, seed, cond2, use_graph=True)
    for a, b in zip(got2, ref2):
        assert torch.equal(a, b), "graph, second condition"
    assert not torch.equal(got2[0], ref[0])
    # the last three steps: tau = 0 writes the template itself
    f, ty, le, lat = _run(eng, case, 3, 3, seed, cond, use_graph=True)
    pm, tm, lm = (torch.as_tensor(v) for v in (case.pm, case.tm, case.lm))
    assert torch.equal(f.cpu()[pm], torch.as_tensor(case.x0)[pm])
    assert torch.equal(ty.cpu()[tm], torch.as_tensor(case.a0)[tm])
    assert torch.equal(le.cpu()[lm], torch.as_tensor(case.l0)[lm])
    lat_t = OG.lattice_from_params(torch.as_tensor(case.l0, dtype=torch.float64), torch.as_tensor(case.g0, dtype=torch.float64))
    np.testing.assert_allclose(lat.cpu().numpy()[case.lm], lat_t.numpy()[case.lm], atol=2e-6, rtol=0)
    eng.check_status()


# ------------------------------------------------------------------------------------------------------------------- 3
def test_empty_condition_and_full_species_mask_change_nothing(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    case, seed = Case(dev, seed=9), 97531
    for use_graph in (False, True):
        plain = _run(eng, case, T - 1, 6, seed, None, use_graph=use_graph)
        empty = {k: None for k in ("x0", "pos_mask", "a0", "type_mask", "l0", "len_mask")}
        none_known = case.cond(pm=np.zeros(case.N, bool), tm=np.zeros(case.N, bool), lm=np.zeros(case.B, bool))
        for c in (empty, none_known):
            for a, b in zip(_run(eng, case, T - 1, 6, seed, c, use_graph=use_graph), plain):
                assert torch.equal(a, b), use_graph
        # every species known = const_types (use_constant_atomic_symbols), from the same initial species
        const = torch.as_tensor(case.a0).to(dev)
        st = case.fresh()
        st[1].copy_(const)
        want = _run(eng, case, T - 1, 6, seed, None, use_graph=use_graph, const=const, state=st)
        species = case.cond(pm=np.zeros(case.N, bool), tm=np.ones(case.N, bool), lm=np.zeros(case.B, bool))
        for a, b in zip(_run(eng, case, T - 1, 6, seed, species, use_graph=use_graph), want):
            assert torch.equal(a, b), use_graph
    eng.check_status()


# ------------------------------------------------------------------------------------------------------------------- 4
def test_unconditioned_crystals_are_untouched(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    case, seed = Case(dev, seed=11), 55555
    plain = _run(eng, case, T - 1, 6, seed, None)
    mixed = _run(eng, case, T - 1, 6, seed, case.cond())
    atoms = torch.as_tensor(case.crystal == 2, device=dev)
    assert torch.equal(mixed[0][atoms], plain[0][atoms]) and torch.equal(mixed[1][atoms], plain[1][atoms])
    assert torch.equal(mixed[2][2], plain[2][2]) and torch.equal(mixed[3][2], plain[3][2])
    assert not torch.equal(mixed[0], plain[0])
    eng.check_status()


# ------------------------------------------------------------------------------------------------------------------- 5, 6
def _template_result(seed=3):
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    rng = np.random.RandomState(seed)
    B, N = len(COUNTS), sum(COUNTS)
    lengths = torch.tensor(rng.uniform(3, 6, (B, 3)))
    angles = torch.tensor(np.deg2rad(rng.uniform(75, 105, (B, 3))))
    na = np.asarray(COUNTS, dtype=np.int64)
    return SampleResult(frac_x=rng.uniform(0, 1, (N, 3)), atomic_numbers=rng.randint(1, S, N).astype(np.float64),
                        lattice=OG.lattice_from_params(lengths, angles).numpy(), num_atoms=na, idx_start=np.cumsum(na) - na)


def _check_end_state(res, tmpl, pm, sm, lm):
    assert res.num_atoms.tolist() == COUNTS
    assert np.array_equal(res.frac_x[pm], tmpl.frac_x[pm].astype(np.float32).astype(np.float64))
    assert np.array_equal(res.atomic_numbers[sm], tmpl.atomic_numbers[sm])
    np.testing.assert_allclose(res.lattice[lm], tmpl.lattice[lm], atol=2e-6, rtol=0)
    from arreau_amd.diffusion.lattice_helpers import matrix_to_params
    np.testing.assert_allclose(matrix_to_params(res.lattice[lm])[0], matrix_to_params(tmpl.lattice[lm])[0], atol=2e-6, rtol=0)
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_whole_run_ends_on_the_template(dev, any_model, use_graph):
    from arreau_amd.diffusion.conditioning import SampleCondition
    m, _ = any_model
    tmpl = _template_result()
    N = sum(COUNTS)
    rng = np.random.RandomState(4)
    pm, sm, lm = rng.rand(N) < 0.5, rng.rand(N) < 0.3, np.array([True, True, False, True])
    cond = SampleCondition.from_sample_result(tmpl, fix_positions=pm, fix_species=sm, fix_lattice=lm)
    torch.manual_seed(2)
    np.random.seed(2)
    res = m.sample(condition=cond, use_graph=use_graph, seed=8642)
    _check_end_state(res, tmpl, pm, sm, lm)
    # counts that agree are accepted; the frames path cuts the same trajectory into segments
    torch.manual_seed(2)
    np.random.seed(2)
    res2 = m.sample(COUNTS, len(COUNTS), condition=cond, use_graph=use_graph, seed=8642)
    assert np.array_equal(res.frac_x, res2.frac_x) and np.array_equal(res.lattice, res2.lattice)


def test_frames_follow_the_conditioned_trajectory(dev, fused_model, tmp_path):
    from arreau_amd.diffusion.conditioning import SampleCondition
    from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting
    m, _ = fused_model
    tmpl = _template_result(seed=6)
    cond = SampleCondition.from_sample_result(tmpl, fix_positions=True, fix_lattice=True)
    runs = []
    for vis in (VisualizationSetting.NONE, VisualizationSetting.ALL):
        torch.manual_seed(1)
        np.random.seed(1)
        runs.append(m.sample(condition=cond, visualization_setting=vis, vis_name=str(tmp_path / "f"), seed=99))
    assert np.array_equal(runs[0].frac_x, runs[1].frac_x) and np.array_equal(runs[0].atomic_numbers, runs[1].atomic_numbers)
    assert os.path.exists(str(tmp_path / "f_90_0.cif")) and os.path.exists(str(tmp_path / "f_final_3.cif"))
    _check_end_state(runs[1], tmpl, np.ones(sum(COUNTS), bool), np.zeros(sum(COUNTS), bool), np.ones(len(COUNTS), bool))


# ------------------------------------------------------------------------------------------------------------------- 7
def test_generate_from_a_template_file(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=30))
    tmpl = _template_result(seed=8)
    src = str(tmp_path / "template.npz")
    np.savez(src, frac_x=tmpl.frac_x, atomic_numbers=tmpl.atomic_numbers, lattice=tmpl.lattice, idx_start=tmpl.idx_start,
             num_atoms=tmpl.num_atoms)
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--template", src, "--fix", "positions,lattice", "--samples_per_template", "2", "--batch", "3",
                        "--seed", "5", "--out", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == COUNTS * 2
    for k in range(2):
        rows = slice(k * sum(COUNTS), (k + 1) * sum(COUNTS))
        assert np.array_equal(res.frac_x[rows], tmpl.frac_x.astype(np.float32).astype(np.float64))
        np.testing.assert_allclose(res.lattice[k * len(COUNTS):(k + 1) * len(COUNTS)], tmpl.lattice, atol=2e-6, rtol=0)
    assert set(res.atomic_numbers.tolist()) <= set(float(z) for z in list(range(1, S)) + [2001])
