"""RePaint resampling on the device: blocks of J steps run R times, a forward jump back to the block's top in front of every
pass after the first (arreau_sample_loop_resampled, arreau_resample_jump; rules in include/arreau_hip.h).  The jump against the
float64 restatement (arreau_amd/diffusion/resampling.py), absorbing and dense forms bitwise; errors and the Philox kinds; the
resampled loop bitwise against its events run one by one, in both loop forms, on both network paths, with a schedule and
corrector steps; eager, graph replay and segments, and no stale graph after a change of R or J; R = 1 as today's sampler;
jumps in distribution; conditioned and whole runs, an oracle trajectory and generate.py.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arreau_amd.diffusion import resampling as rs
from arreau_amd.diffusion import respacing
from oracle import sampler as OS
from tests.sampling_helpers import (Case as _Case, S, T, any_model, assert_same_bits, dev, full_i32, fused_model,  # noqa: F401
                                     model_seed, wrapped_dist)

pytestmark = pytest.mark.gpu
TOL = 1e-5
COUNTS = [4, 7, 2, 150, 1]  # ragged, one crystal above 128 atoms, one single atom
SNR = 0.16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(_Case):
    COUNTS = COUNTS


def _tables(om):
    return om.ve_sigmas.double().numpy(), om.vp_alpha_bars.double().numpy(), om.q_mats.double().numpy()


def _jump_noise(eng, seed, t, r, B, N):
    return (eng.philox_fill_word(seed, t, 6, r, 3 * N).view(N, 3), eng.philox_fill_word(seed, t, 7, r, 3 * B).view(B, 3),
            eng.philox_fill_word(seed, t, 8, r, N * S).view(N, S))


def _cell(lengths, angles):
    from arreau_amd.diffusion.lattice_helpers import lattice_from_params
    return lattice_from_params(lengths.contiguous(), angles.contiguous())


# -------------------------------------------------------------------------------------------------------------- 1
PAIRS = [(0, 1), (0, 37), (5, 6), (12, 60), (98, 99)]


@pytest.mark.parametrize("pair", PAIRS + ["mixed"], ids=[f"{s}-{t}" for s, t in PAIRS] + ["mixed"])
def test_jump_against_the_restatement(dev, any_model, pair):
    m, om = any_model
    eng = m.engine()
    case = Case(dev, seed=7)
    B, N = case.B, case.N
    if pair == "mixed":
        s_c, t_c = np.array([p[0] for p in PAIRS]), np.array([p[1] for p in PAIRS])
    else:
        s_c, t_c = np.full(B, pair[0]), np.full(B, pair[1])
    g = torch.Generator().manual_seed(11)
    z_f, z_l, u = torch.randn(N, 3, generator=g), torch.randn(B, 3, generator=g), torch.rand(N, S, generator=g)
    f, ty, le, lat = case.fresh()
    eng.status(reset=True)
    d = lambda v: v.to(dev).contiguous()
    eng.resample_jump(f, ty, le, case.an, d(torch.as_tensor(s_c, dtype=torch.int32)), d(torch.as_tensor(t_c, dtype=torch.int32)),
                      case.off, d(z_f), d(z_l), d(u), lat)
    eng.check_status()
    sig, ab, qm = _tables(om)
    wf, wt, wl = rs.jump(case.frac.numpy(), case.types.numpy(), case.lengths.numpy(), s_c, t_c, case.na.numpy(), sig, ab, qm,
                         z_f.double().numpy(), z_l.double().numpy(), u.double().numpy())
    assert float(wrapped_dist(f.cpu(), torch.from_numpy(wf)).max()) <= 1e-6
    assert np.allclose(le.cpu().double().numpy(), wl, rtol=1e-5, atol=1e-6)
    assert np.array_equal(ty.cpu().numpy(), wt)
    assert torch.allclose(lat, _cell(le, case.an), rtol=1e-6, atol=1e-6)
    assert ((f >= 0) & (f <= 1)).all()


def test_held_components_are_bit_unchanged(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=9)
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh()
    fixed = le.clone()
    known = torch.as_tensor(np.arange(N) % 3 == 0)
    cond = {"a0": ty.clone(), "type_mask": known.to(torch.uint8).to(dev).contiguous()}
    z_f, z_l, u = (torch.randn(N, 3, device=dev), torch.randn(B, 3, device=dev), torch.rand(N, S, device=dev))
    args = (case.an, full_i32(B, 10, dev), full_i32(B, 70, dev), case.off, z_f, z_l, u, lat)
    eng.resample_jump(f, ty, le, *args, const_types=ty.clone(), fixed_lengths=fixed)
    assert_same_bits((ty, le), case.fresh()[1:3], "const species / fixed cell")
    assert not torch.equal(f, case.fresh()[0])
    f, ty, le, lat = case.fresh()
    eng.resample_jump(f, ty, le, *args[:-1], lat, condition=cond)
    kd = known.to(dev)
    assert torch.equal(ty[kd], case.fresh()[1][kd]) and not torch.equal(ty[~kd], case.fresh()[1][~kd])
    assert not torch.equal(le, case.fresh()[2])  # known species hold; lengths still jump


def test_absorbing_and_dense_forms_are_bit_identical(dev, fused_model, monkeypatch):
    from arreau_amd.checkpoint import make_synthetic_model
    m, _ = fused_model
    monkeypatch.setenv("ARREAU_D3PM_DENSE", "1")
    md = make_synthetic_model(S=S, seed=4321, num_timesteps=T).to(dev)
    engines = (m.engine(), md.engine())  # (the switch is read when the library model is created)
    monkeypatch.delenv("ARREAU_D3PM_DENSE")
    case = Case(dev, seed=13)
    B, N = case.B, case.N
    outs = []
    for eng in engines:
        f, ty, le, lat = case.fresh()
        for s, t in ((0, 37), (12, 60), (98, 99), (0, 100)):
            eng.resample_jump(f, ty, le, case.an, full_i32(B, s, dev), full_i32(B, t, dev), case.off, *_jump_noise(eng, 3, t, 1, B, N), lat)
        outs.append((f, ty, le, lat))
    assert_same_bits(outs[0], outs[1], "absorbing against dense")


# -------------------------------------------------------------------------------------------------------------- 2
def test_out_of_range_pairs_are_flagged(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    B, N = case.B, case.N
    for s, t in ((5, 5), (7, 3), (-1, 4), (0, T + 1), (0, 0)):
        eng.status(reset=True)
        f, ty, le, lat = case.fresh()
        eng.resample_jump(f, ty, le, case.an, full_i32(B, s, dev), full_i32(B, t, dev), case.off, torch.zeros(N, 3, device=dev),
                          torch.zeros(B, 3, device=dev), torch.full((N, S), 0.5, device=dev), lat)
        assert eng.status(reset=True)["flags"] & _hip.STATUS_BAD_TIMESTEP, (s, t)
        assert torch.isfinite(f).all() and torch.isfinite(le).all()


def test_bad_arguments_raise(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    f, ty, le, lat = case.fresh()
    for res in ((0, 2), (65, 2), (2, 0)):
        with pytest.raises(ValueError):
            eng.sample_loop(f, ty, le, case.an, case.off, T - 1, 2, 1, None, lat, resampling=res)
    lib = _hip.lib()
    args = (eng._handle, _hip.ptr(f), _hip.ptr(ty), _hip.ptr(le), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N,
            T - 1, 4, 1, None, None, _hip.ptr(lat), None, 0, 0, None, None, None)
    for R, J in ((0, 2), (65, 2), (2, 0), (3, -1)):
        rc = lib.arreau_sample_loop_resampled(*args, ctypes.byref(_hip.ResamplingC(R, J, None, 0)), _hip.stream_ptr(dev))
        assert rc == -1 and b"resampl" in lib.arreau_last_error()
    # a host schedule that does not hold t_start with n_steps steps after it
    nxt = respacing.next_table(T, [99, 50, 1]).to(dev)
    sched = _hip.SampleScheduleC(_hip.ptr(nxt).value, 0.999)
    ts = (ctypes.c_int32 * 3)(99, 50, 1)
    bad = [(80, 2, ts, 3), (50, 3, ts, 3), (99, 2, None, 0)]
    for t0, n, arr, k in bad:
        a = list(args)
        a[8], a[9] = t0, n
        res = _hip.ResamplingC(2, 2, ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)) if arr else None, k)
        rc = lib.arreau_sample_loop_resampled(*a[:-3], None, ctypes.byref(sched), None, ctypes.byref(res), _hip.stream_ptr(dev))
        assert rc == -1, (t0, n)
    assert torch.equal(f, case.fresh()[0])  # nothing ran
    with pytest.raises(_hip.ArreauHipError):
        eng.resample_jump(f, ty, le, case.an, full_i32(2, 0, dev), full_i32(2, 5, dev), case.off, None, None, None, lat)


def test_philox_jump_kinds(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    for kind in (6, 7, 8):
        with pytest.raises(_hip.ArreauHipError):
            eng.philox_fill(1, 5, kind, 8)
        z = [eng.philox_fill_word(99, 17, kind, r, 4096) for r in range(3)]
        assert not torch.equal(z[0], z[1]) and not torch.equal(z[1], z[2])
        for v in z:
            if kind == 8:
                assert (v >= 0).all() and (v < 1).all() and abs(float(v.mean()) - 0.5) < 0.03
            else:
                assert abs(float(v.mean())) < 0.08 and abs(float(v.std()) - 1.0) < 0.05
    assert not torch.equal(eng.philox_fill_word(99, 17, 6, 0, 64), eng.philox_fill_word(99, 17, 7, 0, 64))
    assert not torch.equal(eng.philox_fill_word(99, 17, 6, 0, 64), eng.philox_fill(99, 17, 1, 64))
    with pytest.raises(_hip.ArreauHipError):
        eng.philox_fill_word(1, 5, 9, 0, 8)


# -------------------------------------------------------------------------------------------------------------- 3, 4
def _replace(eng, om, cond, seed, t, s, r, f, ty, le, an, lat):
    """Conditioning rules 1, 2 and 4 after the step that leaves t for s in pass r, with the draws (seed, t, kind 3 / 4,
    word3 = 256 r); the template itself at s = 0.  The device evaluates them as fused multiply-adds, fma(sig_s, z, x0) and
    fma(sqrt(abar_s), l0, sqrt(1 - abar_s) z) -- here formed in float64 from the float32 operands (the products are exact) and
    rounded once, which gives the same bits."""
    N, B = f.shape[0], le.shape[0]
    pm, lm, tm = cond["pos_mask"].bool(), cond["len_mask"].bool(), cond["type_mask"].bool()
    x0, l0 = cond["x0"], cond["l0"]
    if s == 0:
        kf, kl = torch.remainder(x0, 1.0), l0
    else:
        z3 = eng.philox_fill_word(seed, t, 3, 256 * r, 3 * N).view(N, 3)
        z4 = eng.philox_fill_word(seed, t, 4, 256 * r, 3 * B).view(B, 3)
        kf = torch.remainder((x0.double() + float(om.ve_sigmas[s]) * z3.double()).float(), 1.0)
        ab = om.vp_alpha_bars[s:s + 1].to(z4.device)  # float32, like the device's table; square roots taken on the device too
        noise = (torch.sqrt(1.0 - ab) * z4).double()  # (this product is rounded to fp32 first)
        kl = (torch.sqrt(ab).double() * l0.double() + noise).float()
    f[pm] = kf[pm]
    le[lm] = kl[lm]
    ty[tm] = cond["a0"][tm]
    lat.copy_(_cell(le, an))  # (the loop forms the cell from the replaced lengths)


def _events_one_by_one(eng, case, seed, steps, succ, R, J, respaced, M=0, cond=None, om=None, state=None):
    """resampling.plan, run with predict_scores / corrector_step / reverse_step(_to) / resample_jump on philox_fill_word draws
    (from `state`, default the case's initial state).  With `cond`, the jumps and corrector moves take the condition and the
    replacement rules follow every step (_replace)."""
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh() if state is None else state
    for ev in rs.plan(steps, succ, R, J):
        if ev.kind == "jump":
            eng.resample_jump(f, ty, le, case.an, full_i32(B, ev.s, eng.device), full_i32(B, ev.t, eng.device), case.off,
                              *_jump_noise(eng, seed, ev.t, ev.r, B, N), lat, condition=cond)
            continue
        t, w = ev.t, 256 * ev.r
        t_c = full_i32(B, t, eng.device)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        for j in range(M):
            eng.corrector_step(f, t_c, case.off, eps, eng.philox_fill_word(seed, t, 5, w + j, 3 * N).view(N, 3), SNR,
                               condition=cond)
            eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        noise = (eng.philox_fill_word(seed, t, 0, w, 3 * B).view(B, 3), eng.philox_fill_word(seed, t, 1, w, 3 * N).view(N, 3),
                 eng.philox_fill_word(seed, t, 2, w, N * S).view(N, S))
        if not respaced:
            eng.reverse_step(f, ty, le, case.an, t_c, case.off, eps, logits, len0, *noise, lat)
        else:
            eng.reverse_step_to(f, ty, le, case.an, t_c, full_i32(B, ev.s, eng.device), case.off, eps, logits, len0, *noise, lat, 0.999)
        if cond is not None:
            _replace(eng, om, cond, seed, t, ev.s, ev.r, f, ty, le, case.an, lat)
    return f, ty, le, lat


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
@pytest.mark.parametrize("M", [0, 1])
def test_resampled_loop_is_its_events_one_by_one(dev, any_model, loop_prep, M, monkeypatch):
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    # physical cells, block tops at or below t = 30; the random-init model's shrinking cells overflow the fp16x3 kernels
    # (NaN in the state, the same bits in both runs: nan_ok)
    case, seed, R, J = Case(dev, seed=17, sampler_like=False), 99887766, 3, 2
    corr = (M, SNR) if M else None
    plain = list(range(30, 23, -1))  # 7 steps
    want = _events_one_by_one(eng, case, seed, plain, plain[-1] - 1, R, J, respaced=False, M=M)
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop(*got[:3], case.an, case.off, plain[0], 7, seed, None, got[3], use_graph=use_graph, corrector=corr,
                        resampling=(R, J))
        assert_same_bits(got, want, ("one call", use_graph), nan_ok=True)
    got = case.fresh()
    for lo, hi in ((0, 2), (2, 6), (6, 7)):  # calls cut at block boundaries
        eng.sample_loop(*got[:3], case.an, case.off, plain[lo], hi - lo, seed, None, got[3], use_graph=hi - lo >= 2, corrector=corr,
                        resampling=(R, J))
    assert_same_bits(got, want, "segments", nan_ok=True)
    # respaced, ending at t = 1 (the final block's bottom is 0)
    sched = [30, 24, 18, 12, 3, 2, 1]
    want = _events_one_by_one(eng, case, seed, sched, 0, R, J, respaced=True, M=M)
    nxt = respacing.next_table(T, sched).to(dev)
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop(*got[:3], case.an, case.off, sched[0], len(sched), seed, None, got[3], use_graph=use_graph, next_table=nxt,
                        lattice_clipmax=0.999, corrector=corr, resampling=(R, J, sched))
        assert_same_bits(got, want, ("respaced", use_graph), nan_ok=True)
    got = case.fresh()
    for lo, hi in ((0, 4), (4, 7)):
        eng.sample_loop(*got[:3], case.an, case.off, sched[lo], hi - lo, seed, None, got[3], use_graph=True, next_table=nxt,
                        lattice_clipmax=0.999, corrector=corr, resampling=(R, J, sched))
    assert_same_bits(got, want, "respaced segments", nan_ok=True)
    # every timestep and species index the loop formed was in range (the fp16x3 range flag of this random-init model's
    # shrinking cells is not what this test is about: sample() re-runs such a batch on the full-range kernels)
    from arreau_amd import _hip
    assert not eng.status(reset=True)["flags"] & (_hip.STATUS_BAD_TIMESTEP | _hip.STATUS_BAD_TYPE)


def _condition(case, seed=4):
    """Known positions and species on about half of the atoms (none in crystal 2), every cell's lengths known."""
    rng = np.random.RandomState(seed)
    N, B = case.N, case.B
    known = (rng.rand(N) < 0.5) & (case.crystal != 2)
    d = lambda v: v.to(case.dev).contiguous()
    mask = d(torch.as_tensor(known.astype(np.uint8)))
    return {"x0": d(torch.tensor(rng.uniform(-0.5, 1.5, (N, 3)), dtype=torch.float32) * torch.as_tensor(known)[:, None]),
            "pos_mask": mask, "a0": d(torch.as_tensor(rng.randint(0, S - 1, N), dtype=torch.int32)), "type_mask": mask.clone(),
            "l0": d(torch.tensor(rng.uniform(3, 6, (B, 3)), dtype=torch.float32)), "len_mask": d(torch.ones(B, dtype=torch.uint8))}


@pytest.mark.parametrize("respaced", [False, True], ids=["plain", "respaced"])
def test_conditioned_resampled_loop_is_its_events(dev, any_model, respaced):
    """A conditioned run with R = 3, J = 2 and one corrector move per step, block by block: the loop (graph replay) against its
    events with the replacement rules restated on the host, bit for bit, from the same state at the top of every block.  The
    known components at a block's bottom are the template noised with the draws of the block's last pass (word3 = 512), so a
    wrong counter word in the update or the corrector of a resampled pass shows here."""
    from arreau_amd import _hip
    m, om = any_model
    eng = m.engine()
    case, seed, R, J, M = Case(dev, seed=43, sampler_like=False), 31415, 3, 2, 1
    cond = _condition(case)
    steps = [60, 45, 30, 20, 3, 2, 1] if respaced else list(range(60, 53, -1))
    last_succ = 0 if respaced else 53
    kw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=0.999, resampling=(R, J, steps)) if respaced \
        else dict(resampling=(R, J))
    pm, tm = cond["pos_mask"].bool(), cond["type_mask"].bool()
    loop = case.fresh()
    eng.status(reset=True)
    eng.condition_initial_state(*loop[:3], steps[0], seed, cond)
    for lo in range(0, len(steps), J):
        hi = min(lo + J, len(steps))
        host = tuple(x.clone() for x in loop)
        eng.sample_loop(*loop[:3], case.an, case.off, steps[lo], hi - lo, seed, None, loop[3], use_graph=True, condition=cond,
                        corrector=(M, SNR), **kw)
        f, ty, le, lat = _events_one_by_one(eng, case, seed, steps[lo:hi], steps[hi] if hi < len(steps) else last_succ, R, J,
                                            respaced, M=M, cond=cond, om=om, state=host)
        block = (steps[lo], respaced)
        assert float(wrapped_dist(loop[0][pm], f[pm]).max()) <= 1e-6, block  # the replaced components: the rules
        assert torch.equal(loop[1][tm], ty[tm]) and torch.equal(loop[1][tm], cond["a0"][tm]), block
        assert torch.allclose(loop[2], le, rtol=1e-6, atol=1e-6), block
        assert_same_bits(loop[:3], (f, ty, le), block)
        assert torch.allclose(loop[3], lat, rtol=1e-6, atol=1e-6), block  # (the cell: another kernel's evaluation of it)
    if respaced:  # the run ends at 0: on the template
        assert torch.equal(loop[0][pm], torch.remainder(cond["x0"], 1.0)[pm]) and torch.equal(loop[2], cond["l0"])
    assert not eng.status(reset=True)["flags"] & (_hip.STATUS_BAD_TIMESTEP | _hip.STATUS_BAD_TYPE)


def test_changed_resampling_never_replays_a_stale_graph(dev, any_model):
    m, _ = any_model
    eng = m.engine()
    case, seed, k = Case(dev, seed=23, sampler_like=False), 5150, 6
    bufs = case.fresh()
    for res in ((2, 2), (3, 2), (3, 4), (1, 2), None, (2, 2)):
        case.load(bufs)
        eng.sample_loop(*bufs[:3], case.an, case.off, 60, k, seed, None, bufs[3], use_graph=True, resampling=res)
        want = case.fresh()
        eng.sample_loop(*want[:3], case.an, case.off, 60, k, seed, None, want[3], use_graph=False, resampling=res)
        assert_same_bits(bufs, want, res)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 5
def test_one_pass_is_todays_sampler(dev, any_model):
    m, _ = any_model
    eng = m.engine()
    case, seed, k = Case(dev, seed=31), 4242, 5
    for use_graph in (False, True):
        runs = []
        for res in (None, (1, 1), (1, 3), (1, 100)):
            got = case.fresh()
            eng.sample_loop(*got[:3], case.an, case.off, T - 1, k, seed, None, got[3], use_graph=use_graph, corrector=(1, SNR),
                            resampling=res)
            runs.append(got)
        for r in runs[1:]:
            assert_same_bits(r, runs[0], use_graph)
    for noise in ("philox", "reference"):
        out = []
        for kw in ({}, dict(resample_passes=1, jump_length=3)):
            torch.manual_seed(3)
            np.random.seed(3)
            r = m.sample([4, 7, 1], 3, seed=777, noise=noise, max_steps=6, **kw)
            out.append((r, torch.random.get_rng_state()))
        a, b = out[0][0], out[1][0]
        assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.atomic_numbers, b.atomic_numbers)
        assert np.array_equal(a.lattice, b.lattice) and torch.equal(out[0][1], out[1][1])  # nothing extra drawn


def test_one_pass_through_the_c_entry_point(dev, fused_model):
    """arreau_sample_loop_resampled itself with NULL or passes == 1 is arreau_sample_loop_corrected, eager and graph replay."""
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    lib = _hip.lib()
    case, seed, k = Case(dev, seed=37, sampler_like=False), 8642, 5
    ws = eng.workspace(case.N, case.B)
    corr = _hip.CorrectorC(1, SNR)
    for use_graph in (0, 1):
        runs = []
        for res in ("corrected", None, (1, 1), (1, 3)):
            f, ty, le, lat = got = case.fresh()
            args = (eng._handle, _hip.ptr(f), _hip.ptr(ty), _hip.ptr(le), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N, 60,
                    k, seed, None, None, _hip.ptr(lat), _hip.ptr(ws), ws.numel(), use_graph, None, None, ctypes.byref(corr))
            if res == "corrected":
                rc = lib.arreau_sample_loop_corrected(*args, _hip.stream_ptr(dev))
            else:
                rs_c = ctypes.byref(_hip.ResamplingC(res[0], res[1], None, 0)) if res else None
                rc = lib.arreau_sample_loop_resampled(*args, rs_c, _hip.stream_ptr(dev))
            assert rc == 0, (res, lib.arreau_last_error())
            runs.append(got)
        for r in runs[1:]:
            assert_same_bits(r, runs[0], use_graph)
    # a schedule without its host copy is fine at one pass (the copy is read only to form blocks)
    nxt = respacing.next_table(T, [60, 30, 1]).to(dev)
    f, ty, le, lat = case.fresh()
    eng.sample_loop(f, ty, le, case.an, case.off, 60, 3, seed, None, lat, next_table=nxt, resampling=(1, 4))


# -------------------------------------------------------------------------------------------------------------- 6
def test_jumps_in_distribution(dev, fused_model):
    """x0 noised to s by arreau_diffusion_noise, then jumped s -> t, against x0 noised to t: same law."""
    m, om = fused_model
    eng = m.engine()
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    B, n = 2000, 4
    N = B * n
    g = torch.Generator().manual_seed(5)
    frac0 = (0.5 + 0.01 * torch.rand(N, 3, generator=g)).to(dev)
    types0 = torch.randint(0, S - 1, (N,), generator=g, dtype=torch.int32).to(dev)
    L = torch.diag(torch.tensor([5.0, 6.0, 7.0]))
    lat0 = L.expand(B, 3, 3).contiguous().to(dev)
    off = crystal_offsets(torch.full((B,), n), dev)
    _, ab, qm = _tables(om)
    for s, t in ((3, 8), (10, 60)):
        def noised(tt):
            z_f, u, z_l = torch.randn(N, 3, device=dev), torch.rand(N, S, device=dev), torch.randn(B, 3, device=dev)
            return eng.diffusion_noise(frac0, types0, lat0, full_i32(B, tt, dev), off, z_f, u, z_l)
        a, b = noised(s), noised(t)
        f, ty, le = a["noisy_frac"].clone(), a["noisy_types"].clone(), a["noisy_lengths"].clone()
        lat = torch.empty(B, 3, 3, device=dev)
        eng.resample_jump(f, ty, le, a["angles"], full_i32(B, s, dev), full_i32(B, t, dev), off, torch.randn(N, 3, device=dev),
                          torch.randn(B, 3, device=dev), torch.rand(N, S, device=dev), lat)
        for x, y in ((le, b["noisy_lengths"]),):
            x, y = x.double().cpu().reshape(-1), y.double().cpu().reshape(-1)
            se_m = np.sqrt(float(y.var()) / len(y)) * np.sqrt(2)
            assert abs(float(x.mean() - y.mean())) < 5 * se_m, (s, t)
            se_v = float(y.var()) * np.sqrt(2.0 / len(y)) * np.sqrt(2)
            assert abs(float(x.var() - y.var())) < 5 * se_v, (s, t)
        p = float(np.mean([qm[t - 1][int(c), S - 1] for c in types0.cpu().numpy()]))
        se = np.sqrt(p * (1 - p) / N)
        assert abs(float((ty == S - 1).double().mean()) - p) < 5 * se, (s, t)
        assert abs(float((b["noisy_types"] == S - 1).double().mean()) - p) < 5 * se, (s, t)
        if s == 3:  # small sigma: nothing wraps, the displacement variance is sig_t^2
            d = (f - frac0).double().cpu().reshape(-1)
            v = float(om.ve_sigmas[t]) ** 2
            assert abs(float((d ** 2).mean()) - v) < 5 * v * np.sqrt(2.0 / len(d)), (s, t)


# -------------------------------------------------------------------------------------------------------------- 7
def test_conditioned_resampled_run_ends_on_the_template(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    case, seed = Case(dev, seed=41, sampler_like=False), 13579
    B, N = case.B, case.N
    rng = np.random.RandomState(4)
    known = (rng.rand(N) < 0.5) & (case.crystal != 2)
    x0 = torch.tensor(rng.uniform(-0.5, 1.5, (N, 3)), dtype=torch.float32) * torch.as_tensor(known)[:, None]
    lmask = np.ones(B, np.uint8)  # (every cell known: this random-init model's free cells are not what this test is about)
    l0 = torch.tensor(rng.uniform(3, 6, (B, 3)), dtype=torch.float32)
    cond = {"x0": x0.to(dev).contiguous(), "pos_mask": torch.as_tensor(known.astype(np.uint8)).to(dev).contiguous(),
            "a0": torch.as_tensor(rng.randint(0, S - 1, N), dtype=torch.int32).to(dev).contiguous(),
            "type_mask": torch.as_tensor(known.astype(np.uint8)).to(dev).contiguous(),
            "l0": l0.to(dev).contiguous(), "len_mask": torch.as_tensor(lmask).to(dev).contiguous()}
    runs = []
    for use_graph in (False, True):
        f, ty, le, lat = case.fresh()
        eng.condition_initial_state(f, ty, le, 12, seed, cond)
        eng.sample_loop(f, ty, le, case.an, case.off, 12, 12, seed, None, lat, use_graph=use_graph, condition=cond, resampling=(2, 5))
        runs.append((f, ty, le, lat))
    assert_same_bits(runs[0], runs[1], "eager against graph")
    f, ty, le, lat = runs[0]
    kt = torch.as_tensor(known, device=dev)
    assert torch.equal(f[kt], torch.remainder(cond["x0"], 1.0)[kt])
    assert torch.equal(ty[kt], cond["a0"][kt])
    lk = torch.as_tensor(lmask.astype(bool), device=dev)
    assert torch.equal(le[lk], cond["l0"][lk])
    assert torch.isfinite(f).all() and ((f >= 0) & (f <= 1)).all()
    eng.check_status()


def test_whole_resampled_runs_are_finite_and_in_range(dev, any_model):
    m, _ = any_model
    res = m.sample([3, 8, 1, 5], 4, num_steps=30, resample_passes=2, jump_length=5, seed=5)
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    assert (res.frac_x >= 0).all() and (res.frac_x <= 1).all()
    r = m.sample(COUNTS, len(COUNTS), num_steps=20, resample_passes=3, jump_length=4, corrector_steps=1, seed=6, fixed_cell=True,
                 use_graph=True)
    assert np.isfinite(r.frac_x).all() and ((r.frac_x >= 0) & (r.frac_x <= 1)).all()
    for noise in ("device", "reference"):
        r = m.sample([3, 8, 1], 3, noise=noise, max_steps=6, resample_passes=2, jump_length=3)
        assert np.isfinite(r.frac_x).all() and ((r.frac_x >= 0) & (r.frac_x <= 1)).all()


def test_reference_noise_run_against_the_oracle(dev, fused_model):
    """A short reference-noise run (T = 100), event by event from the device's state: each step against the oracle's network
    and step, each jump against the float64 restatement.  Physical cells, held fixed; species teacher-forced at near-ties."""
    m, om = fused_model
    eng = m.engine()
    case = Case(dev, seed=29, counts=[8, 6], sampler_like=False)
    B, N = case.B, case.N
    batch = torch.as_tensor(case.crystal)
    sig, ab, qm = _tables(om)
    f, ty, le, lat = case.fresh()
    fixed = le.clone()
    g = torch.Generator().manual_seed(2)
    for ev in rs.plan(list(range(T - 1, T - 5, -1)), T - 5, 2, 2):
        frac, types = f.cpu(), ty.cpu().long()
        if ev.kind == "jump":
            z_f, z_l, u = torch.randn(N, 3, generator=g), torch.randn(B, 3, generator=g), torch.rand(N, S, generator=g)
            d = lambda v: v.to(dev).contiguous()
            eng.resample_jump(f, ty, le, case.an, full_i32(B, ev.s, dev), full_i32(B, ev.t, dev), case.off, d(z_f), d(z_l), d(u), lat,
                              fixed_lengths=fixed)
            wf, wt, _ = rs.jump(frac.numpy(), types.numpy(), fixed.cpu().numpy(), np.full(B, ev.s), np.full(B, ev.t),
                                case.na.numpy(), sig, ab, qm, z_f.double().numpy(), z_l.double().numpy(), u.double().numpy(),
                                fixed_cell=True)
            assert float(wrapped_dist(f.cpu(), torch.from_numpy(wf)).max()) <= TOL
            assert np.array_equal(ty.cpu().numpy(), wt) and torch.equal(le, fixed)
            continue
        t = ev.t
        onehot = F.one_hot(types, S)
        scores = OS.predict_scores(om, frac, onehot, torch.full((N,), t), case.na, fixed.cpu(), case.angles, batch)
        noise = OS.StepNoise(torch.randn(B, 3, generator=g), torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g))
        fr_o, ty_o, _, _ = OS.reverse_step(om, frac, types, fixed.cpu(), case.angles, case.na, scores, t, noise)
        t_c = full_i32(B, t, dev)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        d = lambda v: v.to(dev).contiguous()
        eng.reverse_step(f, ty, le, case.an, t_c, case.off, eps, logits, len0, d(noise.z_lattice), d(noise.z_frac), d(noise.u_types),
                         lat)
        le.copy_(fixed)
        s2, sp2 = float(om.ve_sigmas[t]) ** 2, float(om.ve_sigmas[t - 1]) ** 2
        pre = frac.double() - scores[0].double() * (s2 - sp2)
        bound = TOL * pre.abs().clamp(min=1.0) + TOL * max(1.0, float(scores[0].abs().max())) * (s2 - sp2)
        assert (wrapped_dist(f.cpu(), fr_o) <= bound).all(), t
        assert int((ty.cpu().long() != ty_o).sum()) <= 1, t
        ty.copy_(ty_o.to(torch.int32).to(dev))
    eng.check_status()


def test_generate_with_resampling(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "20", "--resample_passes", "2",
                        "--jump_length", "5", "--seed", "5", "--out", out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == [6] * 5
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    assert (res.frac_x >= 0).all() and (res.frac_x <= 1).all()
