"""Species control on the device: per-crystal element sets and a species temperature (arreau_sample_loop_species,
arreau_reverse_step_species; rules in include/arreau_hip.h).  The step against the float64 restatement
(arreau_amd/diffusion/species.py) at S = 12 and S = 124; all-ones rows at temperature 1 bitwise the existing steps and loop;
temperature 0 reading no uniform and making eta = 0 runs functions of the initial state; the loop bitwise against its steps
through segments, graph replay and both loop forms, and with a condition, corrector steps, resampling, a tie, an eta, multistep
and symmetry; NaN logits; whole runs through sample() and generate.py; the rejections.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import multistep as ms, resampling as rs, respacing, species as sp
from tests import species_cases as C
from tests.helpers import oracle_from_module, random_state
from tests.sampling_helpers import (Case as _Case, S, T, any_model, assert_same_bits, dev, full_i32, fused_model,  # noqa: F401
                                     model_seed)

pytestmark = pytest.mark.gpu
CLIP = 0.999
SNR = 0.16
SCHED = [99, 98, 80, 61, 40, 39, 12, 3, 2, 1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Case(_Case):
    COUNTS = C.COUNTS


@pytest.fixture(scope="module")
def models(dev, fused_model):
    """{name: (S, module, oracle model)}: the S = 12 model of the scaffolding and make_synthetic_model(S=124, num_timesteps=100)."""
    from arreau_amd.checkpoint import make_synthetic_model
    big = make_synthetic_model(S=C.S124, seed=C.MODEL_SEED, num_timesteps=T).to(dev)
    return {"S12": (S, *fused_model), "S124": (C.S124, big, oracle_from_module(big, torch.float32))}


def _state(dev, n_classes, seed, counts=C.COUNTS):
    """A ragged sampler state with n_classes species on the device: (frac, types, lengths, lattice), angles, offsets."""
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    frac, types, lengths, angles, na = random_state(n_classes, counts, seed, sampler_like=True)
    d = lambda v: v.to(dev).contiguous()
    return (d(frac), d(types.to(torch.int32)), d(lengths), torch.zeros(len(counts), 3, 3, device=dev)), d(angles), crystal_offsets(na, dev)


def _clone(bufs):
    return tuple(x.clone() for x in bufs)


def _in_sets(types, rows, crystal, t):
    """Every class lies in E(b, t) of its crystal."""
    E = sp.admitted(rows, t)[crystal]
    ty = np.asarray(types.cpu()).astype(np.int64)
    return bool(E[np.arange(len(ty)), ty].all())


# -------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("tau", C.TAUS)
@pytest.mark.parametrize("t,s", C.PAIRS)
@pytest.mark.parametrize("name,group", C.CASES)
def test_step_against_the_restatement(dev, models, name, group, t, s, tau):
    """The species equal species_step except where its top-two margin is below MARGIN, and on at most one atom (float32 against
    float64; the CPU test caps such atoms at one per case); with no exception every class lies in E(b, t); positions, lengths and
    the cell are bitwise those of arreau_reverse_step_to on the same inputs."""
    n_classes, m, om = models[name]
    eng = m.engine()
    rows, crystal = C.rows_of(C.ROWS[name][group], n_classes), C.crystal_index()
    B, N = len(C.COUNTS), sum(C.COUNTS)
    eps, logits, len0, z_l, z_f, u, x_t = C.step_inputs(n_classes, t)
    dd = lambda v: v.to(dev).contiguous()
    start, an, off = _state(dev, n_classes, t)
    start[1].copy_(dd(x_t.to(torch.int32)))
    args = (an, full_i32(B, t, dev), full_i32(B, s, dev), off, dd(eps), dd(logits), dd(len0), dd(z_l), dd(z_f))
    f, ty, le, lat = _clone(start)
    eng.reverse_step_species(f, ty, le, *args, dd(u) if tau > 0 else None, lat, (sp.device_rows(rows, dev), tau), lattice_clipmax=CLIP)
    f2, ty2, le2, lat2 = _clone(start)
    eng.reverse_step_to(f2, ty2, le2, *args, dd(u), lat2, CLIP)
    assert_same_bits((f, le, lat), (f2, le2, lat2), "positions, lengths or cell differ from the step without the option")
    want, margin = sp.species_step(om.q_one_step_transposed, om.q_mats, logits, x_t, t, s, u if tau > 0 else None, rows, crystal, tau)
    diff = ty.cpu().numpy().astype(np.int64) != want
    print(f"{name}/{group} t={t} s={s} tau={tau}: {int(diff.sum())} species differ, smallest margin {float(margin.min()):.3g}")
    assert _in_sets(ty, rows, crystal, t), "a class outside its crystal's admitted set"
    assert bool((margin[diff] < C.MARGIN).all()), "a species differs away from a near-tie"
    assert int(diff.sum()) <= 1
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("allow", ["null", "ones"])
@pytest.mark.parametrize("t,s", [(50, 10), (2, 1), (1, 0), (60, 59)])
def test_all_ones_rows_at_temperature_one_are_the_existing_steps(dev, models, t, s, allow):
    """arreau_reverse_step_to, the eta step, the multistep step and the symmetric step, at S = 124: bit for bit."""
    from tests import symmetry_cases as SC
    from tests.test_gpu_symmetry import _on_device
    n_classes, m, _ = models["S124"]
    eng = m.engine()
    B, N = len(C.COUNTS), sum(C.COUNTS)
    eps, logits, len0, z_l, z_f, u, x_t = C.step_inputs(n_classes, t)
    dd = lambda v: v.to(dev).contiguous()
    start, an, off = _state(dev, n_classes, t)
    start[1].copy_(dd(x_t.to(torch.int32)))
    ctl = lambda nb: (None if allow == "null" else sp.device_rows(np.ones((nb, n_classes), bool), dev), 1.0)
    args = (an, full_i32(B, t, dev), full_i32(B, s, dev), off, dd(eps), dd(logits), dd(len0), dd(z_l), dd(z_f), dd(u))
    tie = torch.as_tensor([0, 1, 2, 0], dtype=torch.int32, device=dev)
    for what in ("to", "tied", "eta", "multistep"):
        a, b = _clone(start), _clone(start)
        if what == "to":
            eng.reverse_step_to(*a[:3], *args, a[3], CLIP)
            eng.reverse_step_species(*b[:3], *args, b[3], ctl(B), lattice_clipmax=CLIP)
        elif what == "tied":
            eng.reverse_step_tied(*a[:3], *args, a[3], tie, CLIP)
            eng.reverse_step_species(*b[:3], *args, b[3], ctl(B), length_tie=tie, lattice_clipmax=CLIP)
        elif what == "eta":
            eng.reverse_step_eta(*a[:3], *args, a[3], 0.3, tie, CLIP)
            eng.reverse_step_species(*b[:3], *args, b[3], ctl(B), length_tie=tie, eta=0.3, lattice_clipmax=CLIP)
        else:
            ha, hb = ms.allocate_history(N, B, dev), ms.allocate_history(N, B, dev)
            for h in (ha, hb):  # a usable history one level up
                h["hist_eps"].copy_(dd(z_f) * 0.1); h["hist_x0"].copy_(dd(len0) * 3); h["hist_t_atom"].fill_(t + 3); h["hist_t_len"].fill_(t + 3)
            eng.reverse_step_multistep(*a[:3], *args[:7], dd(u), a[3], ha, None, CLIP)
            eng.reverse_step_species(*b[:3], *args, b[3], ctl(B), multistep=hb, lattice_clipmax=CLIP)
            assert_same_bits(tuple(hb[k] for k in ms.HISTORY_KEYS), tuple(ha[k] for k in ms.HISTORY_KEYS), "history")
        assert_same_bits(b, a, (what, t, s))
    # the symmetric step on a batch with orbits and unconstrained crystals
    specs, counts = SC.batch(SC.LOOP)
    Bs, Ns = len(counts), sum(counts)
    sstart, san, soff, stie, tables = _on_device(dev, specs, counts, n_classes, 61, cell=(7.0, 11.0))
    g = torch.Generator().manual_seed(t)
    r = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    sargs = (san, full_i32(Bs, t, dev), full_i32(Bs, s, dev), soff, r(Ns, 3) * 0.3, r(Ns, n_classes) * 2, r(Bs, 3).abs() + 0.5, r(Bs, 3),
             r(Ns, 3), torch.rand(Ns, n_classes, generator=g).to(dev))
    a, b = _clone(sstart), _clone(sstart)
    eng.reverse_step_sym(*a[:3], *sargs, a[3], stie, tables, CLIP)
    eng.reverse_step_species(*b[:3], *sargs, b[3], ctl(Bs), length_tie=stie, symmetry=tables, lattice_clipmax=CLIP)
    assert_same_bits(b, a, ("sym", t, s))
    eng.check_status()


def test_all_ones_rows_at_temperature_one_are_the_existing_loop(dev, any_model):
    m, _ = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=17), 1122334455
    nxt = respacing.next_table(T, SCHED).to(dev)
    kw = dict(next_table=nxt, lattice_clipmax=CLIP)
    for use_graph in (False, True):
        want, got = case.fresh(), case.fresh()
        eng.sample_loop(*want[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, want[3], use_graph=use_graph, **kw)
        eng.sample_loop_species(*got[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, got[3],
                                (sp.device_rows(np.ones((case.B, S), bool), dev), 1.0), use_graph=use_graph, **kw)
        assert_same_bits(got, want, use_graph)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 3
def test_temperature_zero_reads_no_uniform(dev, models):
    """Two calls with different uniforms (one of them NaN) and one with d_u_types = NULL: the same bits; above 0 they are needed."""
    from arreau_amd._hip import ArreauHipError
    n_classes, m, _ = models["S124"]
    eng = m.engine()
    t, s = 50, 10
    B = len(C.COUNTS)
    rows = C.rows_of(C.ROWS["S124"]["words"], n_classes)
    eps, logits, len0, z_l, z_f, u, x_t = C.step_inputs(n_classes, t)
    dd = lambda v: v.to(dev).contiguous()
    start, an, off = _state(dev, n_classes, t)
    start[1].copy_(dd(x_t.to(torch.int32)))
    args = (an, full_i32(B, t, dev), full_i32(B, s, dev), off, dd(eps), dd(logits), dd(len0), dd(z_l), dd(z_f))
    runs = []
    for uu in (dd(u), dd(torch.full_like(u, float("nan"))), None):
        bufs = _clone(start)
        eng.reverse_step_species(*bufs[:3], *args, uu, bufs[3], (sp.device_rows(rows, dev), 0.0), lattice_clipmax=CLIP)
        runs.append(bufs)
    for r in runs[1:]:
        assert_same_bits(r, runs[0], "temperature 0 read a uniform")
    bufs = _clone(start)
    with pytest.raises(ArreauHipError, match="null pointer"):
        eng.reverse_step_species(*bufs[:3], *args, None, bufs[3], (sp.device_rows(rows, dev), 0.5), lattice_clipmax=CLIP)
    eng.check_status()


def test_sample_at_eta_zero_and_temperature_zero_is_a_function_of_the_initial_state(dev, fused_model):
    m, _ = fused_model
    counts = [3, 8, 1, 5]
    torch.manual_seed(7)
    np.random.seed(7)
    state = m.diffusion_loss.draw_initial_state(counts, len(counts), num_atomic_states=S)
    kw = dict(initial_state=state, num_steps=10, eta=0.0)
    a, b = (m.sample(seed=seed, species_temperature=0.0, **kw) for seed in (11, 987654321))
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.lattice, b.lattice) and np.array_equal(a.atomic_numbers, b.atomic_numbers)
    assert np.isfinite(a.frac_x).all() and np.isfinite(a.lattice).all()
    c, d = (m.sample(seed=seed, **kw) for seed in (11, 987654321))
    assert not np.array_equal(c.atomic_numbers, d.atomic_numbers)  # at the default temperature the species follow the seed


# -------------------------------------------------------------------------------------------------------------- 4
def _steps_one_by_one(eng, start, an, off, seed, sched, ctl, n_classes=S, **options):
    f, ty, le, lat = _clone(start)
    B, N = le.shape[0], f.shape[0]
    for t, s in zip(sched, sched[1:] + [0]):
        t_c = full_i32(B, t, eng.device)
        eps, logits, len0 = eng.predict_scores(f, ty, le, an, t_c, off)
        eng.reverse_step_species(f, ty, le, an, t_c, full_i32(B, s, eng.device), off, eps, logits, len0,
                                 eng.philox_fill(seed, t, 0, 3 * B).view(B, 3), eng.philox_fill(seed, t, 1, 3 * N).view(N, 3),
                                 eng.philox_fill(seed, t, 2, N * n_classes).view(N, n_classes), lat, ctl, lattice_clipmax=CLIP, **options)
    return f, ty, le, lat


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_species_loop_is_its_steps_one_by_one(dev, any_model, loop_prep, monkeypatch):
    """predict_scores + arreau_reverse_step_species with arreau_philox_fill's draws, step by step, against the species loop: in one
    call, in segments and replayed as a hipGraph -- bit for bit, in both loop forms and on the shape-general path."""
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=17), 1122334455
    rows = C.rows_of(C.ROWS["S12"]["mixed"], S)
    ctl = (sp.device_rows(rows, dev), 0.5)
    nxt = respacing.next_table(T, SCHED).to(dev)
    want = _steps_one_by_one(eng, case.fresh(), case.an, case.off, seed, SCHED, ctl)
    assert _in_sets(want[1], rows, case.crystal, 1)
    kw = dict(next_table=nxt, lattice_clipmax=CLIP)
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop_species(*got[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, got[3], ctl, use_graph=use_graph, **kw)
        assert_same_bits(got, want, ("one call", use_graph))
    got = case.fresh()
    for lo, hi in ((0, 3), (3, 4), (4, 10)):  # segments start at scheduled timesteps
        eng.sample_loop_species(*got[:3], case.an, case.off, SCHED[lo], hi - lo, seed, None, got[3], ctl, use_graph=hi - lo >= 3, **kw)
    assert_same_bits(got, want, "segments")
    # another temperature, other rows on the same buffers: a cached graph must not be replayed
    bufs = case.fresh()
    for other in ((ctl[0], 0.0), (sp.device_rows(C.rows_of([{1}, {2}, {4, 6}, None], S), dev), 0.5), ctl):
        case.load(bufs)
        eng.sample_loop_species(*bufs[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, bufs[3], other, use_graph=True, **kw)
        eager = case.fresh()
        eng.sample_loop_species(*eager[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, eager[3], other, use_graph=False, **kw)
        assert_same_bits(bufs, eager, "replay against eager")
    assert_same_bits(bufs, want, "the first control again")
    eng.check_status()


@pytest.mark.parametrize("option", ["tie", "eta", "multistep"])
def test_species_loop_with_an_option_is_its_steps(dev, fused_model, option):
    m, _ = fused_model
    eng = m.engine()
    case, seed = Case(dev, seed=19), 24680
    rows = C.rows_of(C.ROWS["S12"]["mixed"], S)
    ctl = (sp.device_rows(rows, dev), 1.0 if option == "tie" else 0.0)
    tie = torch.as_tensor([0, 1, 2, 0], dtype=torch.int32, device=dev)
    nxt = respacing.next_table(T, SCHED).to(dev)
    step_kw = {"tie": dict(length_tie=tie), "eta": dict(eta=0.3), "multistep": dict(length_tie=tie)}[option]
    loop_kw = dict(step_kw)
    if option == "multistep":
        step_kw["multistep"], loop_kw["multistep"] = ms.allocate_history(case.N, case.B, dev), ms.allocate_history(case.N, case.B, dev)
    want = _steps_one_by_one(eng, case.fresh(), case.an, case.off, seed, SCHED, ctl, **step_kw)
    got = case.fresh()
    eng.sample_loop_species(*got[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, got[3], ctl, use_graph=True, next_table=nxt,
                            lattice_clipmax=CLIP, **loop_kw)
    assert_same_bits(got, want, option)
    assert _in_sets(got[1], rows, case.crystal, 1)
    # the option is taken: the loop without it differs
    plain = case.fresh()
    eng.sample_loop_species(*plain[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, plain[3], ctl, next_table=nxt, lattice_clipmax=CLIP)
    assert not torch.equal(plain[2], got[2])
    eng.check_status()


def test_symmetric_species_loop_is_its_steps(dev, fused_model):
    """A symmetry batch of tests/symmetry_cases.py: the loop against its steps, every orbit sharing one admitted class."""
    from tests import symmetry_cases as SC
    from tests.test_gpu_symmetry import _on_device, assert_symmetric
    m, _ = fused_model
    eng = m.engine()
    specs, counts = SC.batch(SC.LOOP)
    B = len(counts)
    sets = [{3}, {0, 5, 10}, None, set(range(S - 1)), {1, 2}, {7}, None, {4, 9}]
    rows, crystal = C.rows_of(sets, S), np.repeat(np.arange(B), counts)
    ctl = (sp.device_rows(rows, dev), 0.5)
    seed = 9988776655
    start, an, off, tie, tables = _on_device(dev, specs, counts, S, 61, cell=(7.0, 11.0))
    eng.status(reset=True)
    want = _steps_one_by_one(eng, start, an, off, seed, SCHED, ctl, length_tie=tie, symmetry=tables)
    nxt = respacing.next_table(T, SCHED).to(dev)
    for use_graph in (False, True):
        got = _clone(start)
        eng.sample_loop_species(*got[:3], an, off, SCHED[0], len(SCHED), seed, None, got[3], ctl, use_graph=use_graph, next_table=nxt,
                                lattice_clipmax=CLIP, length_tie=tie, symmetry=tables)
        assert_same_bits(got, want, ("symmetric", use_graph))
    assert_symmetric(specs, counts, want[0].cpu().numpy(), want[1].cpu().numpy(), "the loop's end")
    assert _in_sets(want[1], rows, crystal, 1)
    eng.check_status()


def test_combined_species_loop_is_its_events(dev, fused_model):
    """A respaced, conditioned run with one corrector move per step and resampling (R = 2, J = 2), block by block: the species
    loop (graph replay) against its events run one by one, as tests/test_gpu_ddim_sampling.py does for the eta loop."""
    from arreau_amd import _hip
    from tests.test_gpu_ddim_sampling import _condition
    from tests.test_gpu_resampled_sampling import _jump_noise, _replace
    m, om = fused_model
    eng = m.engine()
    case, seed, R, J, M = Case(dev, seed=43, sampler_like=False), 31415, 2, 2, 1
    B, N = case.B, case.N
    cond = _condition(case)
    rows = C.rows_of(C.ROWS["S12"]["mixed"], S)
    ctl = (sp.device_rows(rows, dev), 0.5)
    steps = [60, 45, 30, 20, 3, 2, 1]
    kw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP, resampling=(R, J, steps))
    tm = cond["type_mask"].bool()
    loop = case.fresh()
    eng.status(reset=True)
    eng.condition_initial_state(*loop[:3], steps[0], seed, cond)
    for lo in range(0, len(steps), J):
        hi = min(lo + J, len(steps))
        f, ty, le, lat = _clone(loop)
        eng.sample_loop_species(*loop[:3], case.an, case.off, steps[lo], hi - lo, seed, None, loop[3], ctl, use_graph=True, condition=cond,
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
            eng.reverse_step_species(f, ty, le, case.an, t_c, full_i32(B, ev.s, dev), case.off, eps, logits, len0,
                                     eng.philox_fill_word(seed, t, 0, w, 3 * B).view(B, 3), eng.philox_fill_word(seed, t, 1, w, 3 * N).view(N, 3),
                                     eng.philox_fill_word(seed, t, 2, w, N * S).view(N, S), lat, ctl, lattice_clipmax=CLIP)
            _replace(eng, om, cond, seed, t, ev.s, ev.r, f, ty, le, case.an, lat)
        assert torch.equal(loop[1][tm], cond["a0"][tm]), steps[lo]
        assert_same_bits(loop[:3], (f, ty, le), steps[lo])
        assert torch.allclose(loop[3], lat, rtol=1e-6, atol=1e-6), steps[lo]  # (the cell: another kernel's evaluation of it)
    free = ~tm.cpu().numpy()
    assert _in_sets(loop[1][~tm], rows, case.crystal[free], 1)
    assert not eng.status(reset=True)["flags"] & (_hip.STATUS_BAD_TIMESTEP | _hip.STATUS_BAD_TYPE)


# -------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("t,s", [(50, 10), (1, 0)])
def test_nan_logits_give_the_lowest_admitted_class(dev, models, t, s):
    n_classes, m, _ = models["S124"]
    eng = m.engine()
    sets = C.ROWS["S124"]["words"]
    rows, crystal = C.rows_of(sets, n_classes), C.crystal_index()
    B = len(C.COUNTS)
    eps, logits, len0, z_l, z_f, u, x_t = C.step_inputs(n_classes, t)
    bad = [0, 5, 12, 100]  # one atom of every crystal
    logits[bad] = float("nan")
    dd = lambda v: v.to(dev).contiguous()
    (f, ty, le, lat), an, off = _state(dev, n_classes, t)
    ty.copy_(dd(x_t.to(torch.int32)))
    eng.status(reset=True)
    eng.reverse_step_species(f, ty, le, an, full_i32(B, t, dev), full_i32(B, s, dev), off, dd(eps), dd(logits), dd(len0), dd(z_l), dd(z_f),
                             dd(u), lat, (sp.device_rows(rows, dev), 1.0), lattice_clipmax=CLIP)
    torch.cuda.synchronize()
    E = sp.admitted(rows, t)
    assert ty.cpu()[bad].tolist() == [int(np.argmax(E[crystal[i]])) for i in bad]
    assert _in_sets(ty, rows, crystal, t)
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 6
def test_sample_within_element_sets(dev, models):
    _, m, _ = models["S124"]
    counts = [4, 7, 2]
    first = np.concatenate([[0], np.cumsum(counts)])
    kw = dict(num_steps=10, seed=2468)

    def run(**more):
        torch.manual_seed(3)
        np.random.seed(3)
        return m.sample(counts, 3, **kw, **more)
    res = run(elements=[["Li", "O"], None, [26]])
    z = np.rint(res.atomic_numbers).astype(int)
    assert set(z[first[0]:first[1]].tolist()) <= {3, 8}
    assert set(z[first[2]:first[3]].tolist()) <= {26}
    plain = run()
    b = slice(first[1], first[2])  # the unrestricted crystal: bitwise the crystal of the same call without `elements`
    assert np.array_equal(res.frac_x[b], plain.frac_x[b]) and np.array_equal(res.atomic_numbers[b], plain.atomic_numbers[b])
    assert np.array_equal(res.lattice[1], plain.lattice[1])
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
    # a host-noise mode takes the step export
    res = m.sample(counts, 3, num_steps=8, noise="device", elements=[3, 8, 26], species_temperature=0.5)
    assert set(np.rint(res.atomic_numbers).astype(int).tolist()) <= {3, 8, 26}


def test_generate_with_elements(dev, tmp_path):
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt,
                        "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "20", "--elements", "Li,O,5",
                        "--species_temperature", "0.5", "--seed", "5", "--out", out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=660)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stdout.count("species control: elements Z in {3, 5, 8}, species temperature 0.5") == 1, p.stdout
    res = load_sample_results_from_hdf5(out)
    assert res.num_atoms.tolist() == [6] * 5
    assert set(np.rint(res.atomic_numbers).astype(int).tolist()) <= {3, 5, 8}
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()


# -------------------------------------------------------------------------------------------------------------- 7
def test_rejections_before_any_work(dev, fused_model):
    from arreau_amd import _hip
    from tests import symmetry_cases as SC
    from tests.test_gpu_symmetry import _on_device
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh()
    before = _clone((f, ty, le))
    z = lambda *shape: torch.zeros(*shape, device=dev)
    p = _hip.ptr
    ws = eng.workspace(N, B)
    step_args = lambda: (eng._handle, p(f), p(ty), p(le), p(case.an), p(full_i32(B, 10, dev)), p(full_i32(B, 5, dev)), p(case.off), B, N,
                         p(z(N, 3)), p(z(N, S)), p(z(B, 3)), p(z(B, 3)), p(z(N, 3)), p(z(N, S) + 0.5), p(lat), CLIP, None)
    loop_args = lambda: (eng._handle, p(f), p(ty), p(le), p(case.an), p(case.off), B, N, 10, 3, 1, None, None, p(lat), p(ws), ws.numel(), 0)
    stream = _hip.stream_ptr(dev)
    lib = _hip.lib()
    good = _hip.SpeciesControlC(None, 1.0)
    # a temperature that is negative or not finite, and a missing struct
    for tau in (-0.1, float("nan"), float("inf")):
        bad = _hip.SpeciesControlC(None, tau)
        assert lib.arreau_reverse_step_species(*step_args(), None, None, None, ctypes.byref(bad), stream) == -1, tau
        assert lib.arreau_sample_loop_species(*loop_args(), None, None, None, None, None, None, None, None, ctypes.byref(bad), stream) == -1, tau
        with pytest.raises(ValueError):
            eng.sample_loop_species(f, ty, le, case.an, case.off, 10, 3, 1, None, lat, (None, tau))
        with pytest.raises(ValueError):
            m.sample([3, 5], 2, num_steps=4, species_temperature=tau)
    assert lib.arreau_reverse_step_species(*step_args(), None, None, None, None, stream) == -1
    assert lib.arreau_sample_loop_species(*loop_args(), None, None, None, None, None, None, None, None, None, stream) == -1
    # what the underlying steps reject: a bad eta, symmetry with an eta, multistep with an eta other than 0, with a condition,
    # corrector steps or resampling, symmetry with resampling
    specs, counts = SC.batch(["p21c", 4])
    sbufs, san, soff, stie, tables = _on_device(dev, specs, counts, S, 61)
    sym = eng._symmetry_struct(tables, sum(counts))
    hist = eng._multistep_struct(ms.allocate_history(N, B, dev), N, B)
    eta = lambda v: ctypes.byref(ctypes.c_float(v))
    sp_ref = ctypes.byref(good)
    assert lib.arreau_reverse_step_species(*step_args(), None, eta(1.5), None, sp_ref, stream) == -1
    assert lib.arreau_reverse_step_species(*step_args(), None, eta(0.5), ctypes.byref(hist), sp_ref, stream) == -1
    sN, sB = sum(counts), len(counts)
    sym_step = (eng._handle, p(sbufs[0]), p(sbufs[1]), p(sbufs[2]), p(san), p(full_i32(sB, 10, dev)), p(full_i32(sB, 5, dev)), p(soff), sB, sN,
                p(z(sN, 3)), p(z(sN, S)), p(z(sB, 3)), p(z(sB, 3)), p(z(sN, 3)), p(z(sN, S) + 0.5), p(sbufs[3]), CLIP, None)
    sym_before = _clone(sbufs[:3])
    assert lib.arreau_reverse_step_species(*sym_step, ctypes.byref(sym), eta(0.5), None, sp_ref, stream) == -1
    corr, res = _hip.CorrectorC(1, SNR), _hip.ResamplingC(2, 2, None, 0)
    known = {"x0": z(N, 3), "pos_mask": torch.ones(N, dtype=torch.uint8, device=dev)}  # (alive through the calls)
    cond = eng._condition_struct(known, N, B)
    for opts in ((None, None, None, None, None, None, eta(-0.5), None),
                 (None, None, None, None, None, None, eta(0.5), ctypes.byref(hist)),
                 (ctypes.byref(cond), None, None, None, None, None, None, ctypes.byref(hist)),
                 (None, None, ctypes.byref(corr), None, None, None, None, ctypes.byref(hist)),
                 (None, None, None, ctypes.byref(res), None, None, None, ctypes.byref(hist))):
        assert lib.arreau_sample_loop_species(*loop_args(), *opts, sp_ref, stream) == -1, opts
    sws = eng.workspace(sN, sB)
    sym_loop = (eng._handle, p(sbufs[0]), p(sbufs[1]), p(sbufs[2]), p(san), p(soff), sB, sN, 10, 3, 1, None, None, p(sbufs[3]), p(sws),
                sws.numel(), 0)
    for opts in ((None, None, None, None, None, ctypes.byref(sym), eta(0.5), None),
                 (None, None, None, ctypes.byref(res), None, ctypes.byref(sym), None, None),
                 (None, None, ctypes.byref(corr), None, None, ctypes.byref(sym), None, None)):
        assert lib.arreau_sample_loop_species(*sym_loop, *opts, sp_ref, stream) == -1, opts
    torch.cuda.synchronize()
    assert_same_bits((f, ty, le), before, "a rejected call touched the state")
    assert_same_bits(sbufs[:3], sym_before, "a rejected call touched the state")
    # a held species outside its crystal's set, an element the table does not hold
    with pytest.raises(ValueError, match="outside the crystal's element set"):
        m.sample(3, 2, num_steps=4, elements=["Li", "O"], use_constant_atomic_symbols=["Li", "O", "C"])
    with pytest.raises(ValueError, match="not in the model's table"):
        m.sample([3, 5], 2, num_steps=4, elements=["Fe"])
    with pytest.raises(ValueError, match="entries for a batch"):
        m.sample([3, 5], 2, num_steps=4, elements=[["Li"], None, ["O"]])
    eng.check_status()
