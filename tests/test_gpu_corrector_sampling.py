"""Predictor-corrector sampling on the device: Langevin corrector moves on the positions before every predictor step
(arreau_sample_loop_corrected, arreau_corrector_step; rule in include/arreau_hip.h).  The corrector move against the float64
restatement (arreau_amd/diffusion/corrector.py); the corrected loop bitwise against its steps run one by one, in both loop
forms and on a respaced schedule; eager, graph replay and segments, and no stale graph after a change of M or snr; M = 0 as
today's sampler; conditioned runs; an oracle trajectory; whole runs through sample() and generate.py.  Needs an MI355X:
`-m gpu`."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arreau_amd.diffusion import corrector as pc
from arreau_amd.diffusion import respacing
from oracle import sampler as OS
from tests.sampling_helpers import (Case as _Case, S, T, any_model, assert_same_bits, dev, full_i32, fused_model,  # noqa: F401
                                     model_seed, wrapped_dist)

pytestmark = pytest.mark.gpu
TOL = 1e-5
COUNTS = [4, 7, 2, 150, 1]  # ragged, one crystal above 128 atoms, one single atom
SNR = 0.16
KIND = 5  # ARREAU_DRAW_Z_CORRECTOR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(_Case):
    COUNTS = COUNTS


# -------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("t", [1, T // 2, T - 1])
@pytest.mark.parametrize("masked", [False, True], ids=["all-free", "masked"])
def test_corrector_step_against_the_restatement(dev, any_model, t, masked):
    m, om = any_model
    eng = m.engine()
    case = Case(dev, seed=t)
    B, N = case.B, case.N
    g = torch.Generator().manual_seed(77 + t)
    f = torch.rand(N, 3, generator=g)
    eps = torch.randn(N, 3, generator=g) * float(om.ve_sigmas[t])  # the size the network is trained to
    eps[case.crystal == 1] *= 40.0  # one crystal far off that size
    eps[case.crystal == 2] = 0.0    # |eps| = 0: unmoved
    z = torch.randn(N, 3, generator=g)
    known = None
    cond = None
    if masked:
        known = torch.rand(N, generator=g) < 0.4
        known[case.crystal == 0] = True  # a crystal with every position known
        x0 = torch.where(known[:, None], f, torch.zeros_like(f))
        cond = {"x0": x0.to(dev).contiguous(), "pos_mask": known.to(torch.uint8).to(dev).contiguous()}
    fd = f.to(dev).contiguous()
    eng.status(reset=True)
    eng.corrector_step(fd, full_i32(B, t, dev), case.off, eps.to(dev).contiguous(), z.to(dev).contiguous(), SNR, condition=cond)
    want = pc.corrector_move(f.double().numpy(), eps.double().numpy(), z.double().numpy(), float(om.ve_sigmas[t]), SNR,
                             case.na.numpy(), known=None if known is None else known.numpy())
    got = fd.cpu()
    assert float(wrapped_dist(got, torch.from_numpy(want)).max()) <= TOL
    unmoved = torch.as_tensor(case.crystal == 2)
    if masked:
        unmoved = unmoved | known
    assert torch.equal(got[unmoved], f[unmoved])
    assert not torch.equal(got[~unmoved], f[~unmoved])
    assert ((got >= 0) & (got <= 1)).all()
    eng.check_status()


def test_out_of_range_timestep_is_flagged(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    for t in (0, T + 1, -4):
        eng.status(reset=True)
        f = case.fresh()[0]
        eng.corrector_step(f, full_i32(case.B, t, dev), case.off, torch.ones(case.N, 3, device=dev), torch.ones(case.N, 3, device=dev),
                           SNR)
        assert eng.status(reset=True)["flags"] & _hip.STATUS_BAD_TIMESTEP, t


def test_bad_arguments_raise(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    f, ty, le, lat = case.fresh()
    for corr in ((17, SNR), (-1, SNR), (1, 0.0), (2, float("nan"))):
        with pytest.raises(ValueError):
            eng.sample_loop(f, ty, le, case.an, case.off, T - 1, 2, 1, None, lat, corrector=corr)
        with pytest.raises(ValueError):
            eng.corrector_step(f, full_i32(case.B, 5, dev), case.off, f, f, corr[1] if corr[0] == 1 else -1.0)
    # the C entry point itself refuses them too (before it looks at anything else)
    lib = _hip.lib()
    for steps, snr in ((17, SNR), (1, float("inf")), (3, -1.0)):
        args = (eng._handle, _hip.ptr(f), _hip.ptr(ty), _hip.ptr(le), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N,
                T - 1, 2, 1, None, None, _hip.ptr(lat), None, 0, 0, None, None)
        rc = lib.arreau_sample_loop_corrected(*args, ctypes.byref(_hip.CorrectorC(steps, snr)), _hip.stream_ptr(dev))
        assert rc == -1 and b"corrector" in lib.arreau_last_error()
    assert torch.equal(f, case.fresh()[0])
    # philox_fill keeps rejecting kind 5; philox_fill_word takes it
    with pytest.raises(_hip.ArreauHipError):
        eng.philox_fill(1, 5, KIND, 8)
    assert torch.isfinite(eng.philox_fill_word(1, 5, KIND, 3, 8)).all()


def test_philox_word3_keys_a_separate_stream(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    for kind in (0, 1, 2, 3, 4):  # word 0 is the existing generator
        a, ra = eng.philox_fill(99, 17, kind, 64, raw=True)
        b, rb = eng.philox_fill_word(99, 17, kind, 0, 64, raw=True)
        assert torch.equal(a, b) and torch.equal(ra, rb)
    z = [eng.philox_fill_word(99, 17, KIND, j, 4096) for j in range(3)]
    assert not torch.equal(z[0], z[1]) and not torch.equal(z[1], z[2])
    assert not torch.equal(z[0], eng.philox_fill(99, 17, 1, 4096))
    for v in z:
        assert abs(float(v.mean())) < 0.08 and abs(float(v.std()) - 1.0) < 0.05


# -------------------------------------------------------------------------------------------------------------- 2, 3
def _one_by_one(eng, case, seed, M, schedule, respaced, snr=SNR):
    """predict_scores -> corrector_step (z from arreau_philox_fill_word) -> ... -> reverse_step, or reverse_step_to on a respaced
    schedule (z from arreau_philox_fill)."""
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh()
    for t, s in zip(schedule, schedule[1:] + [schedule[-1] - 1]):
        t_c = full_i32(B, t, eng.device)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        for j in range(M):
            eng.corrector_step(f, t_c, case.off, eps, eng.philox_fill_word(seed, t, KIND, j, 3 * N).view(N, 3), snr)
            eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        noise = (eng.philox_fill(seed, t, 0, 3 * B).view(B, 3), eng.philox_fill(seed, t, 1, 3 * N).view(N, 3),
                 eng.philox_fill(seed, t, 2, N * S).view(N, S))
        if not respaced:
            eng.reverse_step(f, ty, le, case.an, t_c, case.off, eps, logits, len0, *noise, lat)
        else:
            eng.reverse_step_to(f, ty, le, case.an, t_c, full_i32(B, s, eng.device), case.off, eps, logits, len0, *noise, lat, 0.999)
    return f, ty, le, lat


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
@pytest.mark.parametrize("M", [1, 2])
def test_corrected_loop_is_its_steps_one_by_one(dev, any_model, loop_prep, M, monkeypatch):
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=17), 99887766
    k = 5
    plain = list(range(T - 1, T - 1 - k, -1))
    want = _one_by_one(eng, case, seed, M, plain, respaced=False)
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop(*got[:3], case.an, case.off, plain[0], k, seed, None, got[3], use_graph=use_graph, corrector=(M, SNR))
        assert_same_bits(got, want, ("one call", use_graph))
    got = case.fresh()
    for lo, hi in ((0, 1), (1, 4), (4, 5)):  # segments (frames)
        eng.sample_loop(*got[:3], case.an, case.off, plain[lo], hi - lo, seed, None, got[3], use_graph=hi - lo >= 3,
                        corrector=(M, SNR))
    assert_same_bits(got, want, "segments")
    # respaced: a correction at every scheduled timestep
    sched = [99, 80, 61, 40, 3, 2, 1]
    want = _one_by_one(eng, case, seed, M, sched, respaced=True)
    nxt = respacing.next_table(T, sched).to(dev)
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop(*got[:3], case.an, case.off, sched[0], len(sched), seed, None, got[3], use_graph=use_graph,
                        next_table=nxt, lattice_clipmax=0.999, corrector=(M, SNR))
        assert_same_bits(got, want, ("respaced", use_graph))
    got = case.fresh()
    for lo, hi in ((0, 3), (3, 4), (4, 7)):
        eng.sample_loop(*got[:3], case.an, case.off, sched[lo], hi - lo, seed, None, got[3], use_graph=hi - lo >= 3,
                        next_table=nxt, lattice_clipmax=0.999, corrector=(M, SNR))
    assert_same_bits(got, want, "respaced segments")
    eng.check_status()


def test_changed_corrector_never_replays_a_stale_graph(dev, any_model):
    m, _ = any_model
    eng = m.engine()
    case, seed, k = Case(dev, seed=23), 5150, 4
    bufs = case.fresh()
    for corr in ((1, SNR), (2, SNR), (2, 0.3), (0, SNR), (1, SNR)):
        case.load(bufs)
        eng.sample_loop(*bufs[:3], case.an, case.off, T - 1, k, seed, None, bufs[3], use_graph=True, corrector=corr)
        want = case.fresh()
        eng.sample_loop(*want[:3], case.an, case.off, T - 1, k, seed, None, want[3], use_graph=False, corrector=corr)
        assert_same_bits(bufs, want, corr)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 4
def test_zero_steps_is_todays_sampler(dev, any_model):
    m, _ = any_model
    eng = m.engine()
    case, seed, k = Case(dev, seed=31), 4242, 4
    for use_graph in (False, True):
        runs = []
        for corr in (None, (0, SNR), (0, -1.0)):
            got = case.fresh()
            eng.sample_loop(*got[:3], case.an, case.off, T - 1, k, seed, None, got[3], use_graph=use_graph, corrector=corr)
            runs.append(got)
        sched = [99, 70, 40, 1]
        nxt = respacing.next_table(T, sched).to(dev)
        for corr in (None, (0, SNR)):
            got = case.fresh()
            eng.sample_loop(*got[:3], case.an, case.off, 99, len(sched), seed, None, got[3], use_graph=use_graph,
                            next_table=nxt, corrector=corr)
            runs.append(got)
        for r in runs[1:3]:
            assert_same_bits(r, runs[0], ("plain", use_graph))
        assert_same_bits(runs[4], runs[3], ("scheduled", use_graph))
    torch.manual_seed(3)
    np.random.seed(3)
    a = m.sample([4, 7, 1], 3, seed=777, max_steps=30, fixed_cell=True)
    torch.manual_seed(3)
    np.random.seed(3)
    b = m.sample([4, 7, 1], 3, seed=777, max_steps=30, fixed_cell=True, corrector_steps=0, corrector_snr=5.0)
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.atomic_numbers, b.atomic_numbers)
    assert np.array_equal(a.lattice, b.lattice)


# -------------------------------------------------------------------------------------------------------------- 5
def test_conditioned_corrected_run_keeps_the_known_positions(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    case, seed = Case(dev, seed=41), 13579
    B, N = case.B, case.N
    rng = np.random.RandomState(4)
    known = (rng.rand(N) < 0.5) & (case.crystal != 2)
    known[case.crystal == 0] = True  # crystal 0: every position known
    x0 = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32) * torch.as_tensor(known)[:, None]
    cond = {"x0": x0.to(dev).contiguous(), "pos_mask": torch.as_tensor(known.astype(np.uint8)).to(dev).contiguous()}
    frames = [(99, 9), (90, 40), (50, 49), (1, 1)]  # (t_start, steps): boundaries after t = 91, 51, 2 and the end
    fixed = case.fresh()[2]  # (fixed cells: this random-init model's free cells diverge over a whole run at 150 atoms)
    runs = {}
    for M in (0, 1):
        f, ty, le, lat = case.fresh()
        eng.condition_initial_state(f, ty, le, T - 1, seed, cond)
        states = []
        for t0, n in frames:
            eng.sample_loop(f, ty, le, case.an, case.off, t0, n, seed, None, lat, use_graph=n >= 3, condition=cond,
                            fixed_lengths=fixed, corrector=(M, SNR) if M else None)
            states.append((f.clone(), ty.clone(), le.clone()))
        runs[M] = states
    kt = torch.as_tensor(known, device=dev)
    for (f0, _, _), (f1, _, _) in zip(runs[0], runs[1]):
        assert torch.equal(f0[kt], f1[kt])
        assert not torch.equal(f0[~kt], f1[~kt])
    end = runs[1][-1][0]
    assert torch.equal(end[kt], torch.remainder(cond["x0"], 1.0)[kt])  # the run ends on the template
    c0 = torch.as_tensor(case.crystal == 0, device=dev)
    for (f0, t0, l0), (f1, t1, l1) in zip(runs[0], runs[1]):  # a fully known crystal is untouched by the corrector
        assert torch.equal(f0[c0], f1[c0]) and torch.equal(t0[c0], t1[c0]) and torch.equal(l0[0], l1[0])
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 6
def _move_and_bound(eps, z, sig, na, eps_tol):
    """The pre-wrap move -a eps + c z of every atom (no mask), float64, and how far it can move when every component of eps
    is off by up to eps_tol: a and c scale with 1 / |eps|, so the network's bound reaches the move amplified by
    sqrt(3 n) eps_tol / |eps| (first order: relative change of q = |z| / |eps|, once in c, twice in a) plus a eps_tol."""
    eps, z = eps.double().numpy(), z.double().numpy()
    move, bound, first = np.zeros_like(eps), np.zeros_like(eps), 0
    for n in np.asarray(na):
        rows = slice(first, first + int(n))
        a, c = pc.coefficients(eps[rows], z[rows], sig, SNR)
        move[rows] = -a * eps[rows] + c * z[rows]
        rel_q = eps_tol * np.sqrt(3 * int(n)) / np.linalg.norm(eps[rows])
        bound[rows] = rel_q * (np.abs(c * z[rows]) + 2 * a * np.abs(eps[rows])) + a * eps_tol
        first += int(n)
    return torch.from_numpy(move), torch.from_numpy(bound)


@pytest.mark.parametrize("counts", [[8], [20] * 4], ids=["1x8", "4x20"])
def test_corrected_trajectory_against_the_oracle(dev, any_model, counts):
    """5 steps with M = 1 from T - 1: at every step, from the device's state, the oracle's network and the restated corrector
    against the device's move; then the oracle's network and step on the device's corrected state against the loop's step.
    Physical cells (4-8 A, 70-110 degrees), held fixed: the sampler-start cells (lengths ~ N(0, 1)) put dozens of periodic
    images at nearly equal distances, and a near-tie in the top-k neighbour selection is not what this test is about."""
    m, om = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=29, counts=counts, sampler_like=False), 2468
    B, N = case.B, case.N
    batch = torch.as_tensor(case.crystal)
    f, ty, le, lat = case.fresh()
    fixed = le.clone()
    for t in range(T - 1, T - 6, -1):
        frac, types, lengths = f.cpu(), ty.cpu().long(), le.cpu()
        t_c = full_i32(B, t, dev)
        onehot = F.one_hot(types, S)
        # the corrector move: the restatement on the oracle's eps against the device's move on its own eps
        sig = float(om.ve_sigmas[t])
        eps_o = OS.predict_scores(om, frac, onehot, torch.full((N,), t), case.na, lengths, case.angles, batch)[0]
        z = eng.philox_fill_word(seed, t, KIND, 0, 3 * N).view(N, 3)
        want = pc.corrector_move(frac.double().numpy(), eps_o.double().numpy(), z.cpu().double().numpy(), sig, SNR, case.na.numpy())
        fc = f.clone()
        eps_d = eng.predict_scores(fc, ty, le, case.an, t_c, case.off)[0]
        eng.corrector_step(fc, t_c, case.off, eps_d, z, SNR)
        eps_tol = TOL * max(1.0, float(eps_o.abs().max()))  # the suite's bound on eps (test_gpu_parity: assert_scores_close)
        assert float((eps_d.cpu().double() - eps_o.double()).abs().max()) <= eps_tol, t
        # 1e-5 relative to the unwrapped value, plus the eps bound carried through the step size
        move, carried = _move_and_bound(eps_o, z.cpu(), sig, case.na, eps_tol)
        pre = frac.double() + move
        assert (wrapped_dist(fc.cpu(), torch.from_numpy(want)) <= TOL * pre.abs().clamp(min=1.0) + carried).all(), t
        # ... and the move itself, restated on the device's eps: within 1e-5 of the unwrapped value
        own = pc.corrector_move(frac.double().numpy(), eps_d.cpu().double().numpy(), z.cpu().double().numpy(), sig, SNR,
                                case.na.numpy())
        assert (wrapped_dist(fc.cpu(), torch.from_numpy(own)) <= TOL * pre.abs().clamp(min=1.0)).all(), t
        # the predictor, on the device's corrected state
        frac_c = fc.cpu()
        scores = OS.predict_scores(om, frac_c, onehot, torch.full((N,), t), case.na, lengths, case.angles, batch)
        noise = OS.StepNoise(*(eng.philox_fill(seed, t, k, n).view(*shp).cpu()
                               for k, n, shp in ((0, 3 * B, (B, 3)), (1, 3 * N, (N, 3)), (2, N * S, (N, S)))))
        fr_o, ty_o, _, _ = OS.reverse_step(om, frac_c, types, lengths, case.angles, case.na, scores, t, noise)
        eng.sample_loop(f, ty, le, case.an, case.off, t, 1, seed, None, lat, fixed_lengths=fixed, corrector=(1, SNR))
        s2, sp2 = float(om.ve_sigmas[t]) ** 2, float(om.ve_sigmas[t - 1]) ** 2
        pre = frac_c.double() - scores[0].double() * (s2 - sp2)
        bound = TOL * pre.abs().clamp(min=1.0) + TOL * max(1.0, float(scores[0].abs().max())) * (s2 - sp2)
        assert (wrapped_dist(f.cpu(), fr_o) <= bound).all(), t
        assert torch.equal(le, fixed), t
        assert int((ty.cpu().long() != ty_o).sum()) <= 1, t  # a Gumbel arg-max within rounding of a tie may go either way
        ty.copy_(ty_o.to(torch.int32).to(dev))  # (teacher-forced: such a tie must not fork the rest of the trajectory)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 7
def test_whole_corrected_runs_are_finite_and_in_range(dev, any_model):
    m, _ = any_model
    # free cells: small crystals (this random-init model's free cells diverge at 150 atoms, with or without a corrector)
    res = m.sample([3, 8, 1, 5], 4, num_steps=50, corrector_steps=1, seed=5)
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    assert (res.frac_x >= 0).all() and (res.frac_x <= 1).all()
    # fixed cells: the lengths never move, so the cells are those of the run without a corrector
    runs = []
    for M in (0, 1):
        torch.manual_seed(8)
        np.random.seed(8)
        runs.append(m.sample(COUNTS, len(COUNTS), num_steps=30, corrector_steps=M, seed=6, fixed_cell=True))
    assert np.array_equal(runs[0].lattice, runs[1].lattice)
    assert np.isfinite(runs[1].frac_x).all() and ((runs[1].frac_x >= 0) & (runs[1].frac_x <= 1)).all()
    assert not np.array_equal(runs[0].frac_x, runs[1].frac_x)
    # host-noise modes take the corrector too
    for noise in ("device", "reference"):
        r = m.sample([3, 8, 1], 3, noise=noise, max_steps=6, corrector_steps=2)
        assert np.isfinite(r.frac_x).all() and ((r.frac_x >= 0) & (r.frac_x <= 1)).all()


def test_reference_noise_draws_nothing_extra_at_zero_steps(dev, fused_model):
    m, _ = fused_model
    out = []
    for kw in ({}, dict(corrector_steps=0)):
        torch.manual_seed(11)
        np.random.seed(11)
        r = m.sample([3, 5], 2, noise="reference", max_steps=4, **kw)
        out.append((r.frac_x, torch.random.get_rng_state()))
    assert np.array_equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_generate_with_corrector_steps(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "20", "--corrector_steps", "1",
                        "--seed", "5", "--out", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == [6] * 5
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    assert (res.frac_x >= 0).all() and (res.frac_x <= 1).all()
