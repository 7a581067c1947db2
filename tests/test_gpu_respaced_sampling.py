"""Respaced sampling on the device: the sampler on a subsequence of its timesteps (arreau_sample_loop_scheduled,
arreau_reverse_step_to; rules in include/arreau_hip.h).  The strided step against a float64 restatement of the rules and
bitwise against arreau_reverse_step at stride 1; the respaced loop against the same steps run one by one, through segments,
graph replay and both loop forms; the full schedule against today's sampler; a respaced trajectory against the oracle's
network; conditioned respaced runs; whole runs through sample() and generate.py.  Needs an MI355X: `-m gpu`."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arreau_amd.diffusion import respacing
from oracle import geometry as OG
from oracle import sampler as OS
from tests.sampling_helpers import Case as _Case, S, T, any_model, dev, full_i32, fused_model, model_seed, wrapped_dist  # noqa: F401

pytestmark = pytest.mark.gpu
TOL = 1e-5
COUNTS = [4, 7, 2, 150]  # ragged, one crystal above 128 atoms
CLIP = 0.999
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(_Case):
    COUNTS = COUNTS


# ---------------------------------------------------------------------------------- the rules, restated in float64
def _ve_to(sig, x, eps, t, s, z):
    st2, ss2 = float(sig[t]) ** 2, float(sig[s]) ** 2
    return torch.remainder(x - eps * (st2 - ss2) + math.sqrt(ss2 * (st2 - ss2) / st2) * z, 1.0)


def _vp_to(ab, betas, x, x0, t, s, z):
    ab_t, ab_s = float(ab[t]), float(ab[s])
    beta = float(betas[t]) if s == t - 1 else min(1.0 - ab_t / ab_s, CLIP)
    mean = (math.sqrt(ab_s) * beta * x0 + math.sqrt(1.0 - beta) * (1.0 - ab_s) * x) / (1.0 - ab_t)
    return mean + (1.0 - ab_s) * beta / (1.0 - ab_t) * (z if t > 1 else torch.zeros_like(z))


def _d3pm_post(q1t, qmats, logits, xt, t, s):
    if t == 1:
        return logits
    fact1 = q1t[t - 1, xt, :] if s == t - 1 else qmats[t - s - 1][:, xt].T
    fact2 = torch.softmax(logits, dim=-1) @ qmats[s - 1]
    return torch.log(fact1 + 1e-6) + torch.log(fact2 + 1e-6)


def _step_cpu(om, frac, types, lengths, angles, na, scores, t, s, z_l, z_f, u):
    """Rules 1-3 from t to s in float64 on the model's fp32 tables; returns (frac, types, lengths, lattice, gumbel margin)."""
    d = lambda v: v.double()
    eps, logits, len0 = (d(v) for v in scores)
    le = _vp_to(d(om.vp_alpha_bars), d(om.vp_betas), d(lengths), len0 * na.unsqueeze(-1).double(), t, s, d(z_l))
    fr = _ve_to(d(om.ve_sigmas), d(frac), eps, t, s, d(z_f))
    post = _d3pm_post(d(om.q_one_step_transposed), d(om.q_mats), logits, types, t, s)
    val = post + (-torch.log(-torch.log(torch.clip(d(u), 1e-6, 1.0)))) * (1.0 if t != 1 else 0.2)
    top2 = torch.topk(val, 2, dim=-1).values
    return fr, torch.argmax(val, dim=-1), le, OG.lattice_from_params(le, d(angles)), top2[:, 0] - top2[:, 1]


# -------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("t,s", [(99, 80), (50, 10), (7, 1), (2, 1), (1, 0), (60, 59)])
def test_reverse_step_to_against_the_restatement(dev, fused_model, t, s):
    m, om = fused_model
    eng = m.engine()
    case = Case(dev, seed=t)
    B, N = case.B, case.N
    g = torch.Generator().manual_seed(1000 + t)
    eps = torch.randn(N, 3, generator=g) * 0.3
    logits = torch.randn(N, S, generator=g) * 2.0
    len0 = torch.rand(B, 3, generator=g) + 0.5
    z_l, z_f, u = torch.randn(B, 3, generator=g), torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g)
    dd = lambda v: v.to(dev).contiguous()
    f, ty, le, lat = case.fresh()
    ty.copy_(torch.randint(0, S, (N,), generator=g).to(dev))  # every class as x_t, the mask class included
    x_t = ty.cpu().long()
    eng.reverse_step_to(f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, dd(eps), dd(logits), dd(len0),
                        dd(z_l), dd(z_f), dd(u), lat, CLIP)
    fr_o, ty_o, le_o, lat_o, margin = _step_cpu(om, case.frac, x_t, case.lengths, case.angles, case.na,
                                                (eps, logits, len0), t, s, z_l, z_f, u)
    assert float(wrapped_dist(f.cpu(), fr_o).max()) <= TOL, float((f.cpu().double() - fr_o).abs().max())
    assert float((le.cpu().double() - le_o).abs().max()) <= TOL * max(1.0, float(le_o.abs().max()))
    assert float((lat.cpu().double() - lat_o).abs().max()) <= TOL * max(1.0, float(lat_o.abs().max()))
    diff = ty.cpu().long() != ty_o
    assert bool((margin[diff] < 1e-4).all()), "a species differs away from a Gumbel near-tie"  # fp32 against float64
    assert int(diff.sum()) <= 1
    if s == t - 1:  # rule 4: bit for bit arreau_reverse_step
        f2, ty2, le2, lat2 = case.fresh()
        ty2.copy_(dd(x_t.to(torch.int32)))
        eng.reverse_step(f2, ty2, le2, case.an, full_i32(B, t, dev), case.off, dd(eps), dd(logits), dd(len0), dd(z_l), dd(z_f),
                         dd(u), lat2)
        for a, b in zip((f, ty, le, lat), (f2, ty2, le2, lat2)):
            assert torch.equal(a, b)
    eng.check_status()


def test_bad_targets_are_flagged(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    B, N = case.B, case.N
    z = lambda *shape: torch.zeros(*shape, device=dev)
    for t, s in ((10, 10), (10, -1), (10, 0), (1, 1)):
        eng.status(reset=True)
        f, ty, le, lat = case.fresh()
        eng.reverse_step_to(f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, z(N, 3), z(N, S), z(B, 3),
                            z(B, 3), z(N, 3), z(N, S) + 0.5, lat, CLIP)
        assert eng.status(reset=True)["flags"] & _hip.STATUS_BAD_TIMESTEP, (t, s)


# -------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_respaced_loop_is_its_steps_one_by_one(dev, any_model, loop_prep, monkeypatch):
    """predict_scores + arreau_reverse_step_to with arreau_philox_fill's draws, step by step, against the scheduled loop: in
    one call, in segments, and replayed as a hipGraph -- bit for bit, in both loop forms."""
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=17), 1122334455
    B, N = case.B, case.N
    sched = [99, 98, 80, 61, 40, 39, 12, 3, 2, 1]
    nxt = respacing.next_table(T, sched).to(dev)
    f, ty, le, lat = case.fresh()
    for t, s in zip(sched, sched[1:] + [0]):
        t_c = full_i32(B, t, dev)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        eng.reverse_step_to(f, ty, le, case.an, t_c, full_i32(B, s, dev), case.off, eps, logits, len0,
                            eng.philox_fill(seed, t, 0, 3 * B).view(B, 3), eng.philox_fill(seed, t, 1, 3 * N).view(N, 3),
                            eng.philox_fill(seed, t, 2, N * S).view(N, S), lat, CLIP)
    want = (f, ty, le, lat)
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop(*got[:3], case.an, case.off, sched[0], len(sched), seed, None, got[3], use_graph=use_graph,
                        next_table=nxt, lattice_clipmax=CLIP)
        for a, b in zip(got, want):
            assert torch.equal(a, b), ("one call", use_graph)
    got = case.fresh()
    for lo, hi in ((0, 3), (3, 4), (4, 10)):  # segments start at scheduled timesteps (98 + 1 = 99 is scheduled, 40 + 1 is not)
        eng.sample_loop(*got[:3], case.an, case.off, sched[lo], hi - lo, seed, None, got[3], use_graph=hi - lo >= 3,
                        next_table=nxt, lattice_clipmax=CLIP)
    for a, b in zip(got, want):
        assert torch.equal(a, b), "segments"
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("noise,use_graph", [("philox", True), ("philox", False), ("reference", None)])
def test_full_schedule_given_explicitly_is_todays_sampler(dev, fused_model, noise, use_graph):
    m, _ = fused_model
    # (philox: fixed cells -- this random-init model's free cells diverge over a whole run, with or without a schedule)
    kw = dict(noise=noise, use_graph=use_graph, seed=24680 if noise == "philox" else None, max_steps=None,
              fixed_cell=noise == "philox")
    if noise == "reference":
        kw["max_steps"] = 12  # (the host-noise loop is slow; its schedule is cut the same way)
    runs = []
    for extra in ({}, dict(timesteps=list(range(T - 1, 0, -1))), dict(num_steps=T - 1)):
        torch.manual_seed(3)
        np.random.seed(3)
        runs.append(m.sample(COUNTS, len(COUNTS), **kw, **extra))
    for r in runs[1:]:
        assert np.array_equal(r.frac_x, runs[0].frac_x) and np.array_equal(r.atomic_numbers, runs[0].atomic_numbers)
        assert np.array_equal(r.lattice, runs[0].lattice)


# -------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("counts", [[8], [20] * 4], ids=["1x8", "4x20"])
def test_respaced_trajectory_against_the_oracle(dev, any_model, counts):
    """K = 10 from T - 1: at every scheduled step, from the device's state, the oracle's predict_scores plus the restated step
    with the device's Philox draws against one step of the scheduled loop."""
    m, om = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=29, counts=counts), 777
    B, N = case.B, case.N
    batch = torch.as_tensor(case.crystal)
    sched = respacing.respaced_timesteps(T, 10)
    nxt = respacing.next_table(T, sched).to(dev)
    f, ty, le, lat = case.fresh()
    for t, s in zip(sched, sched[1:] + [0]):
        frac, types, lengths = f.cpu(), ty.cpu().long(), le.cpu()
        scores = OS.predict_scores(om, frac, F.one_hot(types, S), torch.full((N,), t), case.na, lengths, case.angles, batch)
        z_l, z_f, u = (eng.philox_fill(seed, t, k, n).view(*shp).cpu()
                       for k, n, shp in ((0, 3 * B, (B, 3)), (1, 3 * N, (N, 3)), (2, N * S, (N, S))))
        fr_o, ty_o, le_o, lat_o, margin = _step_cpu(om, frac, types, lengths, case.angles, case.na, scores, t, s, z_l, z_f, u)
        eng.sample_loop(f, ty, le, case.an, case.off, t, 1, seed, None, lat, next_table=nxt, lattice_clipmax=CLIP)
        # coordinates: 1e-5 relative to the unwrapped value (this random-init model's eps can be large) plus the scores' bound
        s2, sp2 = float(om.ve_sigmas[t]) ** 2, float(om.ve_sigmas[s]) ** 2
        pre = frac.double() - scores[0].double() * (s2 - sp2)
        bound = TOL * pre.abs().clamp(min=1.0) + TOL * max(1.0, float(scores[0].abs().max())) * (s2 - sp2)
        dd = (f.cpu().double() - fr_o).abs()
        assert (torch.minimum(dd, 1 - dd) <= bound).all(), t
        assert float((le.cpu().double() - le_o).abs().max()) <= TOL * max(1.0, float(le_o.abs().max())), t
        assert float((lat.cpu().double() - lat_o).abs().max()) <= TOL * max(1.0, float(lat_o.abs().max())), t
        assert int((ty.cpu().long() != ty_o).sum()) <= 1, t  # a Gumbel arg-max within rounding of a tie may go either way
        ty.copy_(ty_o.to(torch.int32).to(dev))  # (teacher-forced: such a tie must not fork the rest of the trajectory)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 5
def test_conditioned_respaced_run_ends_on_the_template(dev, fused_model):
    from arreau_amd.diffusion.conditioning import SampleCondition
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    m, _ = fused_model
    rng = np.random.RandomState(3)
    B, N = len(COUNTS), sum(COUNTS)
    lengths = torch.tensor(rng.uniform(3, 6, (B, 3)))
    angles = torch.tensor(np.deg2rad(rng.uniform(75, 105, (B, 3))))
    na = np.asarray(COUNTS, dtype=np.int64)
    tmpl = SampleResult(frac_x=rng.uniform(0, 1, (N, 3)), atomic_numbers=rng.randint(1, S, N).astype(np.float64),
                        lattice=OG.lattice_from_params(lengths, angles).numpy(), num_atoms=na, idx_start=np.cumsum(na) - na)
    crystal = np.repeat(np.arange(B), COUNTS)
    pm = (crystal != 2) & (rng.rand(N) < 0.5)
    sm = (crystal != 2) & (rng.rand(N) < 0.3)
    lm = np.array([True, True, False, True])
    cond = SampleCondition.from_sample_result(tmpl, fix_positions=pm, fix_species=sm, fix_lattice=lm)
    runs = {}
    for name, c in (("cond", cond), ("plain", None)):
        torch.manual_seed(2)
        np.random.seed(2)
        runs[name] = m.sample(COUNTS, B, condition=c, num_steps=12, use_graph=True, seed=8642)
    res = runs["cond"]
    assert np.array_equal(res.frac_x[pm], tmpl.frac_x[pm].astype(np.float32).astype(np.float64))
    assert np.array_equal(res.atomic_numbers[sm], tmpl.atomic_numbers[sm])
    np.testing.assert_allclose(res.lattice[lm], tmpl.lattice[lm], atol=2e-6, rtol=0)
    # crystal 2 is unconditioned: exactly what the same respaced run without a condition gives it
    rows = crystal == 2
    assert np.array_equal(res.frac_x[rows], runs["plain"].frac_x[rows])
    assert np.array_equal(res.atomic_numbers[rows], runs["plain"].atomic_numbers[rows])
    assert np.array_equal(res.lattice[2], runs["plain"].lattice[2])
    assert not np.array_equal(res.frac_x, runs["plain"].frac_x)


# -------------------------------------------------------------------------------------------------------------- 6
def test_whole_respaced_runs_are_finite_and_in_range(dev, any_model, tmp_path):
    from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting
    m, _ = any_model
    # fixed cells: this random-init model's free cells diverge over a whole run (150 atoms scale its predicted lengths)
    res = m.sample(COUNTS, len(COUNTS), num_steps=50, seed=5, fixed_cell=True)
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    assert (res.frac_x >= 0).all() and (res.frac_x <= 1).all()
    # frames follow the schedule and do not change the trajectory; device noise takes the schedule too
    torch.manual_seed(1)
    np.random.seed(1)
    a = m.sample(COUNTS, len(COUNTS), timesteps=[99, 70, 40, 20, 10, 1], seed=5, fixed_cell=True)
    torch.manual_seed(1)
    np.random.seed(1)
    b = m.sample(COUNTS, len(COUNTS), timesteps=[99, 70, 40, 20, 10, 1], seed=5, fixed_cell=True,
                 visualization_setting=VisualizationSetting.ALL, vis_name=str(tmp_path / "f"))
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.lattice, b.lattice)
    names = sorted(p.name.split("_")[1] for p in tmp_path.iterdir())
    assert set(names) == {"70", "40", "20", "10", "final"}, names
    c = m.sample([3, 8, 1, 5], 4, num_steps=8, noise="device")  # (free cells: small crystals, as the plain sampler's tests)
    assert np.isfinite(c.frac_x).all() and np.isfinite(c.lattice).all()
    assert (c.frac_x >= 0).all() and (c.frac_x <= 1).all()


def test_generate_with_num_steps(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "20", "--seed", "5",
                        "--out", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == [6] * 5
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    assert (res.frac_x >= 0).all() and (res.frac_x <= 1).all()
