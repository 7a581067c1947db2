"""DDIM-style sampling on the device: an eta in [0, 1] that scales the noise of the reverse step (arreau_sample_loop_eta,
arreau_reverse_step_eta; rules in include/arreau_hip.h).  The eta step against the float64 restatement (arreau_amd/diffusion/ddim.py),
untied and tied; eta = 1 against the ancestral step; eta = 0 reading no noise; the eta loop bitwise against its steps one by one,
through segments, graph replay and both loop forms, and combined with a corrector, resampling and a condition; a trajectory
against the oracle's network; whole runs through sample() and generate.py.  Needs an MI355X: `-m gpu`."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arreau_amd.diffusion import ddim, lattice_systems as ls, resampling as rs, respacing
from oracle import geometry as OG
from oracle import sampler as OS
from tests.sampling_helpers import (Case as _Case, S, T, any_model, assert_same_bits, dev, full_i32, fused_model,  # noqa: F401
                                     model_seed, wrapped_dist)

pytestmark = pytest.mark.gpu
TOL = 1e-5
COUNTS = [4, 7, 2, 150]  # ragged, one crystal above 128 atoms
CODES = [0, 1, 2, 0]
CLIP = 0.999
SNR = 0.16
PAIRS = [(99, 80), (50, 10), (7, 1), (2, 1), (1, 0), (60, 59)]
SCHED = [99, 98, 80, 61, 40, 39, 12, 3, 2, 1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(_Case):
    COUNTS = COUNTS


def _codes(dev, codes=CODES):
    return torch.as_tensor(codes, dtype=torch.int32, device=dev).contiguous()


# ---------------------------------------------------------------------------------- the rules, restated in float64
def _tied_inputs(x0, xt, z, codes):
    """Tie rule 1 on the inputs of the length move: the axes of G take the leader's x_t and draw and the group's mean x0."""
    x0, xt, z = (np.array(a, dtype=np.float64) for a in (x0, xt, z))
    for b, code in enumerate(codes or []):
        if code > 0:
            g = ls.tied_axes(code)
            x0[b, g] = sum(x0[b, j] for j in range(g.stop)) / g.stop
            xt[b, g], z[b, g] = xt[b, 0], z[b, 0]
    return x0, xt, z


def _d3pm_post(q1t, qmats, logits, xt, t, s):
    if t == 1:
        return logits
    fact1 = q1t[t - 1, xt, :] if s == t - 1 else qmats[t - s - 1][:, xt].T
    fact2 = torch.softmax(logits, dim=-1) @ qmats[s - 1]
    return torch.log(fact1 + 1e-6) + torch.log(fact2 + 1e-6)


def _step_cpu(om, frac, types, lengths, angles, na, scores, t, s, z_l, z_f, u, eta, codes=None):
    """The eta moves (ddim.py) and the unchanged species rule from t to s in float64 on the model's fp32 tables; returns
    (frac, types, lengths, lattice, gumbel margin)."""
    d = lambda v: v.double()
    eps, logits, len0 = (d(v) for v in scores)
    sig, ab, betas = (d(v).numpy() for v in (om.ve_sigmas, om.vp_alpha_bars, om.vp_betas))
    x0, xt, zz = _tied_inputs((len0 * na.unsqueeze(-1).double()).numpy(), d(lengths).numpy(), d(z_l).numpy(), codes)
    le = torch.as_tensor(ddim.length_step(ab, betas, xt, x0, t, s, zz, eta, CLIP))
    fr = torch.as_tensor(ddim.ve_step(sig, d(frac).numpy(), eps.numpy(), t, s, d(z_f).numpy(), eta))
    post = _d3pm_post(d(om.q_one_step_transposed), d(om.q_mats), logits, types, t, s)
    val = post + (-torch.log(-torch.log(torch.clip(d(u), 1e-6, 1.0)))) * (1.0 if t != 1 else 0.2)
    top2 = torch.topk(val, 2, dim=-1).values
    return fr, torch.argmax(val, dim=-1), le, OG.lattice_from_params(le, d(angles)), top2[:, 0] - top2[:, 1]


def _inputs(case, t):
    """The network outputs, draws and x_t classes of one step (every class as x_t, the mask class included), on the host."""
    g = torch.Generator().manual_seed(1000 + t)
    B, N = case.B, case.N
    eps = torch.randn(N, 3, generator=g) * 0.3
    logits = torch.randn(N, S, generator=g) * 2.0
    len0 = torch.rand(B, 3, generator=g) + 0.5
    z_l, z_f, u = torch.randn(B, 3, generator=g), torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g)
    x_t = torch.randint(0, S, (N,), generator=g)
    return eps, logits, len0, z_l, z_f, u, x_t


def assert_tied(lengths, codes, what=""):
    le = lengths.detach().cpu()
    for b, code in enumerate(codes):
        if code > 0:
            assert torch.equal(le[b, :code + 1], le[b, :1].expand(code + 1)), (what, b, le[b])


# -------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("eta", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("t,s", PAIRS)
def test_reverse_step_eta_against_the_restatement(dev, fused_model, t, s, eta, tied):
    m, om = fused_model
    eng = m.engine()
    case = Case(dev, seed=t)
    B, N = case.B, case.N
    eps, logits, len0, z_l, z_f, u, x_t = _inputs(case, t)
    dd = lambda v: v.to(dev).contiguous()
    f, ty, le, lat = case.fresh()
    ty.copy_(dd(x_t.to(torch.int32)))
    eng.reverse_step_eta(f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, dd(eps), dd(logits), dd(len0),
                         dd(z_l), dd(z_f), dd(u), lat, eta, _codes(dev) if tied else None, CLIP)
    fr_o, ty_o, le_o, lat_o, margin = _step_cpu(om, case.frac, x_t, case.lengths, case.angles, case.na, (eps, logits, len0), t, s,
                                                z_l, z_f, u, eta, CODES if tied else None)
    e_f = float(wrapped_dist(f.cpu(), fr_o).max())
    e_l = float((le.cpu().double() - le_o).abs().max())
    e_c = float((lat.cpu().double() - lat_o).abs().max())
    print(f"t={t} s={s} eta={eta} tied={tied}: frac {e_f:.3g}  lengths {e_l:.3g} of {float(le_o.abs().max()):.3g}  cell {e_c:.3g}")
    assert e_f <= TOL
    assert e_l <= TOL * max(1.0, float(le_o.abs().max()))
    assert e_c <= TOL * max(1.0, float(lat_o.abs().max()))
    diff = ty.cpu().long() != ty_o
    assert bool((margin[diff] < 1e-4).all()), "a species differs away from a Gumbel near-tie"  # fp32 against float64
    assert int(diff.sum()) <= 1
    if tied:
        assert_tied(le, CODES, (t, s, eta))
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("t,s", PAIRS)
def test_eta_one_is_the_ancestral_step(dev, fused_model, t, s):
    """eta = 1 against arreau_reverse_step_to on the same inputs.  Species: the same code, bit-equal.  Positions: two float32
    evaluations of one float64 value.  Lengths: l = c0 x0 + c1 x_t + var z in both; the eta move's coefficients differ from the
    posterior mean's by the rounding of the float32 betas table against 1 - abar_t / abar_s (and by the clip, where it binds);
    the test forms the two differences in float64 from the model's tables, which bounds the difference of the results."""
    m, om = fused_model
    eng = m.engine()
    case = Case(dev, seed=t)
    B, N = case.B, case.N
    eps, logits, len0, z_l, z_f, u, x_t = _inputs(case, t)
    dd = lambda v: v.to(dev).contiguous()
    runs = []
    for step in ("eta", "to"):
        f, ty, le, lat = case.fresh()
        ty.copy_(dd(x_t.to(torch.int32)))
        args = (f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, dd(eps), dd(logits), dd(len0), dd(z_l), dd(z_f),
                dd(u), lat)
        if step == "eta":
            eng.reverse_step_eta(*args, 1.0, None, CLIP)
        else:
            eng.reverse_step_to(*args, CLIP)
        runs.append((f, ty, le, lat))
    (f, ty, le, _), (f2, ty2, le2, _) = runs
    assert torch.equal(ty, ty2)
    assert float(wrapped_dist(f, f2).max()) <= 2e-5
    ab, betas = om.vp_alpha_bars.double().numpy(), om.vp_betas.double().numpy()
    beta = ddim.length_beta(ab, betas, t, s, CLIP)
    c_x0, c_xt, _ = ddim.length_coefficients(ab[t], ab[s], beta, 1.0)
    den = 1.0 - ab[t]
    d0 = abs(c_x0 - math.sqrt(ab[s]) * beta / den)
    d1 = abs(c_xt - math.sqrt(1.0 - beta) * (1.0 - ab[s]) / den)
    x0_max = float((len0.double() * case.na.unsqueeze(-1)).abs().max())
    bound = d0 * x0_max + d1 * float(case.lengths.abs().max()) + 2e-5 * max(1.0, float(le2.abs().max()))
    err = float((le.double() - le2.double()).abs().max())
    print(f"t={t} s={s}: dc0 {d0:.3g} dc1 {d1:.3g}  lengths differ by {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_eta_zero_reads_no_noise(dev, fused_model, tied):
    """Two calls with different z arrays (one of them NaN) and one without the arrays: the same bits."""
    m, _ = fused_model
    eng = m.engine()
    t, s = 50, 10
    case = Case(dev, seed=t)
    B, N = case.B, case.N
    eps, logits, len0, z_l, z_f, u, x_t = _inputs(case, t)
    dd = lambda v: v.to(dev).contiguous()
    nan = lambda v: torch.full_like(v, float("nan"))
    runs = []
    for zl, zf in ((dd(z_l), dd(z_f)), (dd(nan(z_l)), dd(nan(z_f))), (None, None)):
        f, ty, le, lat = case.fresh()
        ty.copy_(dd(x_t.to(torch.int32)))
        eng.reverse_step_eta(f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, dd(eps), dd(logits), dd(len0),
                             zl, zf, dd(u), lat, 0.0, _codes(dev) if tied else None, CLIP)
        runs.append((f, ty, le, lat))
    for r in runs[1:]:
        assert_same_bits(r, runs[0], "eta = 0 read a draw")
    # with an eta the arrays are needed, and read
    from arreau_amd._hip import ArreauHipError
    f, ty, le, lat = case.fresh()
    with pytest.raises(ArreauHipError, match="null pointer"):
        eng.reverse_step_eta(f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, dd(eps), dd(logits), dd(len0),
                             None, None, dd(u), lat, 0.5, None, CLIP)
    eng.reverse_step_eta(f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, dd(eps), dd(logits), dd(len0),
                         dd(z_l), dd(z_f), dd(u), lat, 0.5, None, CLIP)
    assert not torch.equal(f, runs[0][0]) and not torch.equal(le, runs[0][2])
    eng.check_status()


def test_bad_eta_is_rejected_by_the_library(dev, fused_model):
    """ARREAU_EINVAL before any work, through the C entry points themselves (the engine validates first, so it is bypassed)."""
    import ctypes
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh()
    before = tuple(x.clone() for x in (f, ty, le))
    z = lambda *shape: torch.zeros(*shape, device=dev)
    p = _hip.ptr
    ws = eng.workspace(N, B)
    for eta in (-0.1, 1.5, float("nan"), float("inf")):
        rc = _hip.lib().arreau_reverse_step_eta(
            eng._handle, p(f), p(ty), p(le), p(case.an), p(full_i32(B, 10, dev)), p(full_i32(B, 5, dev)), p(case.off), B, N, p(z(N, 3)),
            p(z(N, S)), p(z(B, 3)), p(z(B, 3)), p(z(N, 3)), p(z(N, S) + 0.5), p(lat), CLIP, None, ctypes.c_float(eta),
            _hip.stream_ptr(dev))
        assert rc == -1, eta
        rc = _hip.lib().arreau_sample_loop_eta(
            eng._handle, p(f), p(ty), p(le), p(case.an), p(case.off), B, N, 10, 3, 1, None, None, p(lat), p(ws), ws.numel(), 0,
            None, None, None, None, None, ctypes.c_float(eta), _hip.stream_ptr(dev))
        assert rc == -1, eta
    torch.cuda.synchronize()
    assert_same_bits((f, ty, le), before, "a rejected call touched the state")


# -------------------------------------------------------------------------------------------------------------- 4
def _steps_one_by_one(eng, case, seed, sched, eta, tie=None):
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh()
    for t, s in zip(sched, sched[1:] + [0]):
        t_c = full_i32(B, t, eng.device)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        eng.reverse_step_eta(f, ty, le, case.an, t_c, full_i32(B, s, eng.device), case.off, eps, logits, len0,
                             eng.philox_fill(seed, t, 0, 3 * B).view(B, 3), eng.philox_fill(seed, t, 1, 3 * N).view(N, 3),
                             eng.philox_fill(seed, t, 2, N * S).view(N, S), lat, eta, tie, CLIP)
    return f, ty, le, lat


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_eta_loop_is_its_steps_one_by_one(dev, any_model, loop_prep, eta, monkeypatch):
    """predict_scores + arreau_reverse_step_eta with arreau_philox_fill's draws, step by step, against the eta loop: in one call,
    in segments, and replayed as a hipGraph -- bit for bit, in both loop forms; then the same with the lattice-system tie."""
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=17), 1122334455
    nxt = respacing.next_table(T, SCHED).to(dev)
    for tie in (None, _codes(dev)):
        want = _steps_one_by_one(eng, case, seed, SCHED, eta, tie)
        kw = dict(next_table=nxt, lattice_clipmax=CLIP, eta=eta, length_tie=tie)
        for use_graph in (False, True):
            got = case.fresh()
            eng.sample_loop(*got[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, got[3], use_graph=use_graph, **kw)
            assert_same_bits(got, want, ("one call", use_graph, tie is not None))
        got = case.fresh()
        for lo, hi in ((0, 3), (3, 4), (4, 10)):  # segments start at scheduled timesteps
            eng.sample_loop(*got[:3], case.an, case.off, SCHED[lo], hi - lo, seed, None, got[3], use_graph=hi - lo >= 3, **kw)
        assert_same_bits(got, want, ("segments", tie is not None))
        if tie is not None:
            assert_tied(got[2], CODES, "loop")
    eng.check_status()


def test_eta_loop_without_a_schedule_and_another_eta_is_captured_anew(dev, fused_model):
    """Every timestep from 30 (s = t - 1, the model's betas table) on the same buffers: graph replays at eta = 0.5, then 0, then
    without an eta, each against the eager loop -- a cached graph of another eta must not be replayed."""
    m, _ = fused_model
    eng = m.engine()
    case, seed, n = Case(dev, seed=23, sampler_like=False), 97531, 6
    bufs = case.fresh()
    results = {}
    for eta in (0.5, 0.0, None, 0.5):
        case.load(bufs)
        eng.sample_loop(*bufs[:3], case.an, case.off, 30, n, seed, None, bufs[3], use_graph=True, eta=eta)
        got = tuple(x.clone() for x in bufs)
        want = case.fresh()
        eng.sample_loop(*want[:3], case.an, case.off, 30, n, seed, None, want[3], use_graph=False, eta=eta)
        assert_same_bits(got, want, ("replay against eager", eta), nan_ok=True)
        if eta in results:
            assert_same_bits(got, results[eta], ("the same eta again", eta), nan_ok=True)
        results[eta] = got
    assert not torch.equal(results[0.5][0], results[0.0][0]) and not torch.equal(results[0.5][0], results[None][0])
    # stride 1 through the step: the loop's first step
    f, ty, le, lat = case.fresh()
    t_c = full_i32(case.B, 30, dev)
    eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
    B, N = case.B, case.N
    eng.reverse_step_eta(f, ty, le, case.an, t_c, full_i32(B, 29, dev), case.off, eps, logits, len0,
                         eng.philox_fill(seed, 30, 0, 3 * B).view(B, 3), eng.philox_fill(seed, 30, 1, 3 * N).view(N, 3),
                         eng.philox_fill(seed, 30, 2, N * S).view(N, S), lat, 0.5, None, CLIP)
    one = case.fresh()
    eng.sample_loop(*one[:3], case.an, case.off, 30, 1, seed, None, one[3], eta=0.5)
    assert_same_bits(one, (f, ty, le, lat), "one step of the schedule-less loop", nan_ok=True)


# -------------------------------------------------------------------------------------------------------------- 5
def _condition(case, seed=4):
    """Known positions and species on about half of the atoms (none in crystal 2), the lengths of crystals 0 and 3 known."""
    rng = np.random.RandomState(seed)
    N, B = case.N, case.B
    known = (rng.rand(N) < 0.5) & (case.crystal != 2)
    d = lambda v: v.to(case.dev).contiguous()
    mask = d(torch.as_tensor(known.astype(np.uint8)))
    return {"x0": d(torch.tensor(rng.uniform(-0.5, 1.5, (N, 3)), dtype=torch.float32) * torch.as_tensor(known)[:, None]),
            "pos_mask": mask, "a0": d(torch.as_tensor(rng.randint(0, S - 1, N), dtype=torch.int32)), "type_mask": mask.clone(),
            "l0": d(torch.tensor(rng.uniform(3, 6, (B, 3)), dtype=torch.float32)),
            "len_mask": d(torch.as_tensor(np.array([1, 0, 0, 1], dtype=np.uint8)))}


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_combined_eta_loop_is_its_events(dev, any_model, eta):
    """A respaced, conditioned run with one corrector move per step and resampling (R = 2, J = 2), block by block: the loop
    (graph replay) against its events run one by one -- jumps, corrector moves, the eta step on arreau_philox_fill_word's draws,
    the replacement rules restated on the host -- bit for bit, from the same state at the top of every block."""
    from arreau_amd import _hip
    from tests.test_gpu_resampled_sampling import _jump_noise, _replace
    m, om = any_model
    eng = m.engine()
    case, seed, R, J, M = Case(dev, seed=43, sampler_like=False), 31415, 2, 2, 1
    B, N = case.B, case.N
    cond = _condition(case)
    steps = [60, 45, 30, 20, 3, 2, 1]
    kw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP, resampling=(R, J, steps), eta=eta)
    pm, tm, lm = cond["pos_mask"].bool(), cond["type_mask"].bool(), cond["len_mask"].bool()
    loop = case.fresh()
    eng.status(reset=True)
    eng.condition_initial_state(*loop[:3], steps[0], seed, cond)
    for lo in range(0, len(steps), J):
        hi = min(lo + J, len(steps))
        f, ty, le, lat = tuple(x.clone() for x in loop)
        eng.sample_loop(*loop[:3], case.an, case.off, steps[lo], hi - lo, seed, None, loop[3], use_graph=True, condition=cond,
                        corrector=(M, SNR), **kw)
        for ev in rs.plan(steps[lo:hi], steps[hi] if hi < len(steps) else 0, R, J):
            if ev.kind == "jump":
                eng.resample_jump(f, ty, le, case.an, full_i32(B, ev.s, dev), full_i32(B, ev.t, dev), case.off,
                                  *_jump_noise(eng, seed, ev.t, ev.r, B, N), lat, condition=cond)
                continue
            t, w = ev.t, 256 * ev.r
            t_c = full_i32(B, t, dev)
            eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
            for j in range(M):
                eng.corrector_step(f, t_c, case.off, eps, eng.philox_fill_word(seed, t, 5, w + j, 3 * N).view(N, 3), SNR, condition=cond)
                eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
            eng.reverse_step_eta(f, ty, le, case.an, t_c, full_i32(B, ev.s, dev), case.off, eps, logits, len0,
                                 eng.philox_fill_word(seed, t, 0, w, 3 * B).view(B, 3), eng.philox_fill_word(seed, t, 1, w, 3 * N).view(N, 3),
                                 eng.philox_fill_word(seed, t, 2, w, N * S).view(N, S), lat, eta, None, CLIP)
            _replace(eng, om, cond, seed, t, ev.s, ev.r, f, ty, le, case.an, lat)
        block = (steps[lo], eta)
        assert torch.equal(loop[1][tm], cond["a0"][tm]), block
        assert_same_bits(loop[:3], (f, ty, le), block)
        assert torch.allclose(loop[3], lat, rtol=1e-6, atol=1e-6), block  # (the cell: another kernel's evaluation of it)
    # the run ends at 0: on the template
    assert torch.equal(loop[0][pm], torch.remainder(cond["x0"], 1.0)[pm]) and torch.equal(loop[2][lm], cond["l0"][lm])
    assert not eng.status(reset=True)["flags"] & (_hip.STATUS_BAD_TIMESTEP | _hip.STATUS_BAD_TYPE)


# -------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("counts", [[8], [20] * 4], ids=["1x8", "4x20"])
def test_deterministic_trajectory_against_the_oracle(dev, any_model, counts):
    """K = 10 from T - 1 at eta = 0: at every scheduled step, from the device's state, the oracle's predict_scores plus the
    restated eta step against one step of the eta loop (teacher-forced).  The bounds are those of the respaced trajectory test,
    the weight of eps being the eta step's sig_t (sig_t - sig_s)."""
    m, om = any_model
    eng = m.engine()
    case, seed, eta = Case(dev, seed=29, counts=counts), 777, 0.0
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
        fr_o, ty_o, le_o, lat_o, margin = _step_cpu(om, frac, types, lengths, case.angles, case.na, scores, t, s, z_l, z_f, u, eta)
        eng.sample_loop(f, ty, le, case.an, case.off, t, 1, seed, None, lat, next_table=nxt, lattice_clipmax=CLIP, eta=eta)
        # coordinates: 1e-5 relative to the unwrapped value (this random-init model's eps can be large) plus the scores' bound
        w, _ = ddim.ve_coefficients(float(om.ve_sigmas[t]), float(om.ve_sigmas[s]), eta)
        pre = frac.double() - scores[0].double() * w
        bound = TOL * pre.abs().clamp(min=1.0) + TOL * max(1.0, float(scores[0].abs().max())) * w
        dd = (f.cpu().double() - fr_o).abs()
        assert (torch.minimum(dd, 1 - dd) <= bound).all(), t
        assert float((le.cpu().double() - le_o).abs().max()) <= TOL * max(1.0, float(le_o.abs().max())), t
        assert float((lat.cpu().double() - lat_o).abs().max()) <= TOL * max(1.0, float(lat_o.abs().max())), t
        assert int((ty.cpu().long() != ty_o).sum()) <= 1, t  # a Gumbel arg-max within rounding of a tie may go either way
        ty.copy_(ty_o.to(torch.int32).to(dev))  # (teacher-forced: such a tie must not fork the rest of the trajectory)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 7
def _sample_held(m, counts, seed, **kw):
    """sample() with every species held (constant_atoms; ragged counts), from one initial state whatever the Philox seed."""
    from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable
    torch.manual_seed(7)
    np.random.seed(7)
    held = torch.as_tensor(np.random.RandomState(1).randint(0, S - 1, sum(counts)))
    return m.diffusion_loss.sample(model=m, z_table=AtomicNumberTable(m.z_table_zs.tolist()), t_emb_weights=m.t_emb,
                                   num_atoms_per_sample=counts, num_samples_in_batch=len(counts), constant_atoms=held, seed=seed, **kw)


def test_sample_at_eta_zero_is_a_function_of_the_initial_state(dev, fused_model):
    m, _ = fused_model
    kw = dict(num_steps=10, fixed_cell=True)
    a, b = (_sample_held(m, COUNTS, seed, eta=0.0, **kw) for seed in (11, 987654321))
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.lattice, b.lattice)
    assert np.array_equal(a.atomic_numbers, b.atomic_numbers)
    assert np.isfinite(a.frac_x).all() and (a.frac_x >= 0).all() and (a.frac_x <= 1).all()
    c, d = (_sample_held(m, COUNTS, seed, eta=0.5, **kw) for seed in (11, 987654321))
    assert not np.array_equal(c.frac_x, d.frac_x)
    assert not np.array_equal(a.frac_x, c.frac_x)
    # free cells (small crystals): the lengths are deterministic too
    small = [3, 8, 1, 5]
    e, g = (_sample_held(m, small, seed, eta=0.0, num_steps=8) for seed in (11, 987654321))
    assert np.array_equal(e.frac_x, g.frac_x) and np.array_equal(e.lattice, g.lattice) and np.isfinite(e.lattice).all()
    h, k = (_sample_held(m, small, seed, eta=0.5, num_steps=8) for seed in (11, 987654321))
    assert not np.array_equal(h.lattice, k.lattice)


# -------------------------------------------------------------------------------------------------------------- 8
def test_sample_other_settings(dev, fused_model, monkeypatch):
    from arreau_amd.diffusion.conditioning import SampleCondition
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    m, _ = fused_model
    B, N = len(COUNTS), sum(COUNTS)
    in_range = lambda r: (np.isfinite(r.frac_x).all() and np.isfinite(r.lattice).all() and (r.frac_x >= 0).all()
                          and (r.frac_x <= 1).all())
    # a lattice system: a = b = c bitwise after every engine call that moves the lengths (the loop, the host-noise eta step)
    eng, states = m.engine(), []
    for name in ("sample_loop", "reverse_step_eta"):
        def wrapped(*a, _orig=getattr(eng, name), **k):
            out = _orig(*a, **k)
            states.append(a[2].clone())  # (frac, types, lengths, ...) in both
            return out
        monkeypatch.setattr(eng, name, wrapped)
    for kw in (dict(seed=5), dict(noise="device")):
        states.clear()
        res = m.sample([3, 8, 1, 5], 4, num_steps=8, eta=0.0, lattice_system="cubic", **kw)
        assert in_range(res) and states
        for le in states:
            assert_tied(le, [2] * 4, kw)
        n = np.linalg.norm(res.lattice, axis=2)
        assert np.all(np.abs(n - n[:, :1]) <= 4e-6 * n[:, :1]), n
    # a condition at eta = 0 ends on the template
    rng = np.random.RandomState(3)
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
    res = m.sample(COUNTS, B, condition=cond, num_steps=12, use_graph=True, seed=8642, eta=0.0)
    assert np.array_equal(res.frac_x[pm], tmpl.frac_x[pm].astype(np.float32).astype(np.float64))
    assert np.array_equal(res.atomic_numbers[sm], tmpl.atomic_numbers[sm])
    np.testing.assert_allclose(res.lattice[lm], tmpl.lattice[lm], atol=2e-6, rtol=0)
    # the host-noise modes take the eta step (free cells: small crystals, as the plain sampler's tests)
    for noise in ("device", "reference"):
        res = m.sample([3, 8, 1, 5], 4, num_steps=8, noise=noise, eta=0.5)
        assert in_range(res), noise
    assert in_range(m.sample([3, 8, 1, 5], 4, num_steps=8, noise="reference", eta=0.0, lattice_system="tetragonal"))


# -------------------------------------------------------------------------------------------------------------- 9
def test_generate_with_eta(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "20", "--eta", "0", "--seed", "5",
                        "--out", out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == [6] * 5
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    assert (res.frac_x >= 0).all() and (res.frac_x <= 1).all()
