"""Second-order multistep sampling on the device (arreau_sample_loop_multistep, arreau_reverse_step_multistep; rules in
include/arreau_hip.h): the step with an empty history against the eta = 0 step, three consecutive steps against the float64
restatement (arreau_amd/diffusion/multistep.py) within its derived bounds, the loop bitwise against its steps one by one, through
segments, graph replay and both loop forms, whole runs through sample(), the analytic Gaussian trajectory through the step
export, and what the C entry points reject.  Needs an MI355X: `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import multistep as ms, respacing
from tests.multistep_cases import CODES, COUNTS, L_START, MEAN, STEP_SCHEDULES, VAR, X_START
from tests.sampling_helpers import (Case as _Case, S, T, any_model, assert_same_bits, dev, full_i32, fused_model,  # noqa: F401
                                     model_seed)

pytestmark = pytest.mark.gpu
CLIP = 0.999
SCHED = [99, 98, 80, 61, 40, 39, 12, 3, 2, 1]
U = 2.0 ** -24


class Case(_Case):
    COUNTS = COUNTS


def _codes(dev, codes=CODES):
    return torch.as_tensor(codes, dtype=torch.int32, device=dev).contiguous()


def _history(case, fill=None):
    h = ms.allocate_history(case.N, case.B, case.dev)
    if fill is not None:  # values a first-order move must not read into its result
        h["hist_eps"].fill_(fill)
        h["hist_x0"].fill_(fill)
    return h


def _inputs(case, t, scale=1.0):
    """The network outputs, uniforms and x_t classes of one step, made on the host."""
    g = torch.Generator().manual_seed(2000 + t)
    B, N = case.B, case.N
    eps = torch.randn(N, 3, generator=g) * 0.3 * scale
    logits = torch.randn(N, S, generator=g) * 2.0
    len0 = torch.rand(B, 3, generator=g) + 0.5
    return eps, logits, len0, torch.rand(N, S, generator=g), torch.randint(0, S, (N,), generator=g)


def _tables(om):
    return om.ve_sigmas.double().numpy(), om.vp_alpha_bars.double().numpy()


def _hist_bits(h):
    return tuple(h[k] for k in ms.HISTORY_KEYS)


def assert_tied(lengths, codes, what=""):
    le = lengths.detach().cpu()
    for b, code in enumerate(codes):
        if code > 0:
            assert torch.equal(le[b, :code + 1], le[b, :1].expand(code + 1)), (what, b, le[b])


# -------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("t,s", [(99, 80), (50, 49), (2, 1), (1, 0)])
def test_empty_history_is_the_eta_zero_step(dev, fused_model, t, s, tied):
    """Levels of 0, and levels that are not usable (p <= t, p > T) over NaN history values: arreau_reverse_step_eta at eta = 0 bit
    for bit on positions, species, lengths and cell; the history then holds e, x0 and t."""
    m, om = fused_model
    eng = m.engine()
    case = Case(dev, seed=t)
    B, N = case.B, case.N
    eps, logits, len0, u, x_t = _inputs(case, t)
    dd = lambda v: v.to(dev).contiguous()
    tie = _codes(dev) if tied else None
    t_c, s_c = full_i32(B, t, dev), full_i32(B, s, dev)
    want = case.fresh()
    want[1].copy_(dd(x_t.to(torch.int32)))
    eng.reverse_step_eta(*want[:3], case.an, t_c, s_c, case.off, dd(eps), dd(logits), dd(len0), None, None, dd(u), want[3], 0.0, tie, CLIP)
    for level, fill in ((0, None), (0, float("nan")), (t, float("nan")), (t - 1, float("nan")), (T + 1, float("nan")), (-5, 1e30)):
        h = _history(case, fill)
        h["hist_t_atom"].fill_(level)
        h["hist_t_len"].fill_(level)
        got = case.fresh()
        got[1].copy_(dd(x_t.to(torch.int32)))
        eng.reverse_step_multistep(*got[:3], case.an, t_c, s_c, case.off, dd(eps), dd(logits), dd(len0), dd(u), got[3], h, tie, CLIP)
        assert_same_bits(got, want, ("empty history", level))
        assert torch.equal(h["hist_t_atom"], full_i32(N, t, dev)) and torch.equal(h["hist_t_len"], full_i32(B, t, dev))
        assert torch.equal(h["hist_eps"].cpu(), eps * om.ve_sigmas[t].float())
        if not tied:
            assert torch.equal(h["hist_x0"].cpu(), len0 * case.na.unsqueeze(-1).float())
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 2
def _expected_step(om, case, state, hist, scores, t_of, s_of, codes):
    """One step of every crystal in float64 on the device's state and history (read back), by the restatement: returns the
    expected (frac, lengths), their bounds, and the expected history values and orders per crystal."""
    sig, ab = _tables(om)
    f, le = state[0].cpu().double().numpy(), state[2].cpu().double().numpy()
    he, hx = hist["hist_eps"].cpu().double().numpy(), hist["hist_x0"].cpu().double().numpy()
    pa, pl = hist["hist_t_atom"].cpu().numpy(), hist["hist_t_len"].cpu().numpy()
    eps, len0 = scores[0].double().numpy(), scores[2].double().numpy()
    x0 = len0 * case.na.double().numpy()[:, None]
    x0_t, le_t, hx_t = ms.tie_inputs(x0, le, hx, codes)
    first = np.concatenate([[0], np.cumsum(case.na.numpy())])
    fr_o, fr_b, le_o, le_b = np.empty_like(f), np.empty_like(f), np.empty_like(le), np.empty_like(le)
    e_o, orders = np.empty_like(f), []
    for b in range(case.B):
        a = slice(first[b], first[b + 1])
        t, s = int(t_of[b]), int(s_of[b])
        assert (pa[a] == pa[first[b]]).all()
        fr_o[a], e_o[a], o_x = ms.position_step(sig, f[a], eps[a], he[a], int(pa[first[b]]), t, s)
        fr_b[a] = ms.position_error_bound(sig, f[a], eps[a], he[a], int(pa[first[b]]), t, s)
        le_o[b], o_l = ms.length_step(ab, le_t[b], x0_t[b], hx_t[b], int(pl[b]), t, s)
        le_b[b] = ms.length_error_bound(ab, le_t[b], x0_t[b], hx_t[b], int(pl[b]), t, s)
        orders.append((o_x, o_l))
    return fr_o, fr_b, le_o, le_b, e_o, x0_t, orders


def _three_steps(dev, m, om, scheds, tied):
    """Crystal b walks scheds[b] (four levels: three steps).  Every step: the restatement on the state and history read back
    from the device, then the step; positions and lengths within the derived bounds, the history e, x0 and t, the species those of
    the eta = 0 step, tied axes bitwise equal."""
    eng = m.engine()
    case = Case(dev, seed=11)
    B, N = case.B, case.N
    codes = CODES if tied else None
    tie = _codes(dev) if tied else None
    dd = lambda v: v.to(dev).contiguous()
    state, h = case.fresh(), _history(case, float("nan"))
    seen = []
    for i in range(3):
        t_of, s_of = [sc[i] for sc in scheds], [sc[i + 1] for sc in scheds]
        t_c, s_c = (torch.as_tensor(v, dtype=torch.int32, device=dev) for v in (t_of, s_of))
        eps, logits, len0, u, x_t = _inputs(case, 1000 * (i + 1) + t_of[0])  # (other scores at every step)
        state[1].copy_(dd(x_t.to(torch.int32)))
        fr_o, fr_b, le_o, le_b, e_o, x0_t, orders = _expected_step(om, case, state, h, (eps, logits, len0), t_of, s_of, codes)
        seen.append(orders)
        ref = tuple(x.clone() for x in state)  # the species of the eta = 0 step on the same inputs
        eng.reverse_step_eta(*ref[:3], case.an, t_c, s_c, case.off, dd(eps), dd(logits), dd(len0), None, None, dd(u), ref[3], 0.0, tie, CLIP)
        eng.reverse_step_multistep(*state[:3], case.an, t_c, s_c, case.off, dd(eps), dd(logits), dd(len0), dd(u), state[3], h, tie, CLIP)
        assert torch.equal(state[1], ref[1]), "the species step changed"
        d = np.abs(state[0].cpu().double().numpy() - fr_o)
        d = np.minimum(d, 1 - d)
        e_l = np.abs(state[2].cpu().double().numpy() - le_o)
        print(f"step {i} {t_of} -> {s_of} tied={tied}: frac {d.max():.3g} ({(d / fr_b).max():.2f} of its bound)  "
              f"lengths {e_l.max():.3g} ({(e_l / le_b).max():.2f} of its bound)  orders {orders}")
        assert (d <= fr_b).all(), (i, float((d / fr_b).max()))
        assert (e_l <= le_b).all(), (i, float((e_l / le_b).max()))
        # a first-order move is the eta = 0 move bit for bit; a second-order one is not, where the extrapolation is above rounding
        first = np.concatenate([[0], np.cumsum(case.na.numpy())])
        f1 = np.remainder(ref[0].cpu().double().numpy(), 1.0)
        for b, (o_x, o_l) in enumerate(orders):
            a = slice(first[b], first[b + 1])
            same_x, same_l = torch.equal(state[0][a], ref[0][a]), torch.equal(state[2][b], ref[2][b])
            assert same_x or o_x, (i, b, "positions")
            assert same_l or o_l, (i, b, "lengths")
            dx = np.abs(fr_o[a] - f1[a])
            if o_x and np.minimum(dx, 1 - dx).max() > 1e-5:
                assert not same_x, (i, b, "positions")
            if o_l and np.abs(le_o[b] - ref[2][b].cpu().double().numpy()).max() > 1e-5:
                assert not same_l, (i, b, "lengths")
        # the history: e and x0 as float32 values, the levels t
        he = h["hist_eps"].cpu().double().numpy()
        assert (np.abs(he - e_o) <= U * np.abs(e_o)).all()
        hx = h["hist_x0"].cpu().double().numpy()
        assert (np.abs(hx - x0_t) <= ms.X0_ROUNDINGS * U * np.abs(x0_t)).all()
        crystal = torch.as_tensor(case.crystal, device=dev)
        assert torch.equal(h["hist_t_len"], t_c) and torch.equal(h["hist_t_atom"], t_c[crystal])
        if tied:
            assert_tied(state[2], CODES, i)
            assert_tied(h["hist_x0"], CODES, i)
    eng.check_status()
    return seen


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
@pytest.mark.parametrize("sched", list(STEP_SCHEDULES), ids=lambda s: "-".join(map(str, s)))
def test_three_steps_against_the_restatement(dev, fused_model, sched, tied):
    m, om = fused_model
    seen = _three_steps(dev, m, om, [sched] * len(COUNTS), tied)
    want = STEP_SCHEDULES[sched]
    for i, orders in enumerate(seen):
        assert all(o == (want["positions"][i], want["lengths"][i]) for o in orders), (i, orders)


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_three_steps_with_crystals_at_different_levels(dev, fused_model, tied):
    m, om = fused_model
    keys = list(STEP_SCHEDULES)
    scheds = [keys[b % 3] for b in range(len(COUNTS))]
    seen = _three_steps(dev, m, om, scheds, tied)
    for i, orders in enumerate(seen):
        for b, o in enumerate(orders):
            assert o == (STEP_SCHEDULES[scheds[b]]["positions"][i], STEP_SCHEDULES[scheds[b]]["lengths"][i]), (i, b)


# -------------------------------------------------------------------------------------------------------------- 3
def _steps_one_by_one(eng, case, seed, sched, tie=None):
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh()
    h = _history(case)
    for t, s in zip(sched, sched[1:] + [0]):
        t_c = full_i32(B, t, eng.device)
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        eng.reverse_step_multistep(f, ty, le, case.an, t_c, full_i32(B, s, eng.device), case.off, eps, logits, len0,
                                   eng.philox_fill(seed, t, 2, N * S).view(N, S), lat, h, tie, CLIP)
    return (f, ty, le, lat), h


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_multistep_loop_is_its_steps_one_by_one(dev, any_model, loop_prep, monkeypatch):
    """predict_scores + arreau_reverse_step_multistep with arreau_philox_fill's uniforms, step by step, against the loop: in one
    call eager, in one call replayed as a hipGraph, and cut into calls that share the history -- bit for bit, state and history, in
    both loop forms and on the shape-general path; then the same with the lattice-system tie."""
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = any_model
    eng = m.engine()
    case, seed = Case(dev, seed=17), 1122334455
    nxt = respacing.next_table(T, SCHED).to(dev)
    for tie in (None, _codes(dev)):
        want, want_h = _steps_one_by_one(eng, case, seed, SCHED, tie)
        kw = dict(next_table=nxt, lattice_clipmax=CLIP, length_tie=tie)
        for use_graph in (False, True):
            got, h = case.fresh(), _history(case)
            eng.sample_loop(*got[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, got[3], use_graph=use_graph, multistep=h, **kw)
            assert_same_bits(got, want, ("one call", use_graph, tie is not None))
            assert_same_bits(_hist_bits(h), _hist_bits(want_h), ("history", use_graph, tie is not None))
        got, h = case.fresh(), _history(case)
        for lo, hi in ((0, 3), (3, 4), (4, 10)):  # segments start at scheduled timesteps; the calls never empty the history
            eng.sample_loop(*got[:3], case.an, case.off, SCHED[lo], hi - lo, seed, None, got[3], use_graph=hi - lo >= 3, multistep=h, **kw)
        assert_same_bits(got, want, ("segments", tie is not None))
        assert_same_bits(_hist_bits(h), _hist_bits(want_h), ("history of the segments", tie is not None))
        if tie is not None:
            assert_tied(got[2], CODES, "loop")
        # and it is not the eta = 0 loop
        plain = case.fresh()
        eng.sample_loop(*plain[:3], case.an, case.off, SCHED[0], len(SCHED), seed, None, plain[3], eta=0.0, **kw)
        assert not torch.equal(plain[0], want[0]) and not torch.equal(plain[2], want[2])
    eng.check_status()


def test_loop_without_a_schedule_and_the_graph_key(dev, fused_model):
    """Every timestep from 30 (s = t - 1) on the same buffers: graph replays with one history, with another history, at eta = 0
    without one, each against its eager loop -- a cached graph of other history buffers or of the eta loop must not be replayed."""
    m, _ = fused_model
    eng = m.engine()
    case, seed, n = Case(dev, seed=23, sampler_like=False), 97531, 6
    bufs = case.fresh()
    h1, h2 = _history(case), _history(case)
    results = []
    for h in (h1, h2, None, h1):
        case.load(bufs)
        kw = dict(multistep=h) if h is not None else dict(eta=0.0)
        if h is not None:
            ms.empty_history(h)
        eng.sample_loop(*bufs[:3], case.an, case.off, 30, n, seed, None, bufs[3], use_graph=True, **kw)
        got = tuple(x.clone() for x in bufs)
        want, hw = case.fresh(), _history(case)
        eng.sample_loop(*want[:3], case.an, case.off, 30, n, seed, None, want[3], use_graph=False,
                        **(dict(multistep=hw) if h is not None else dict(eta=0.0)))
        assert_same_bits(got, want, "replay against eager", nan_ok=True)
        if h is not None:
            assert_same_bits(_hist_bits(h), _hist_bits(hw), "history of the replay", nan_ok=True)
            assert torch.equal(h["hist_t_len"], full_i32(case.B, 30 - n + 1, dev))
        results.append(got)
    assert_same_bits(results[0], results[1], "another history buffer, the same run", nan_ok=True)
    assert_same_bits(results[0], results[3], "the first history again", nan_ok=True)
    assert not torch.equal(results[0][0], results[2][0])


# -------------------------------------------------------------------------------------------------------------- 4, 5
def _held(counts):
    return torch.as_tensor(np.random.RandomState(1).randint(0, S - 1, sum(counts)))


def test_sample_multistep_is_a_function_of_the_initial_state(dev, fused_model):
    m, _ = fused_model
    counts = [3, 8, 1, 5]
    torch.manual_seed(7)
    np.random.seed(7)
    state = m.diffusion_loss.draw_initial_state(counts, len(counts), num_atomic_states=S, constant_atoms=_held(counts))
    kw = dict(initial_state=state, use_constant_atomic_symbols=True, num_steps=12)
    a, b = (m.sample(multistep=True, seed=seed, **kw) for seed in (11, 987654321))
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.lattice, b.lattice)
    assert np.isfinite(a.frac_x).all() and np.isfinite(a.lattice).all() and (a.frac_x >= 0).all() and (a.frac_x <= 1).all()
    c = m.sample(eta=0.0, seed=11, **kw)
    assert not np.array_equal(a.frac_x, c.frac_x) and not np.array_equal(a.lattice, c.lattice)
    d = m.sample(multistep=True, eta=0.0, seed=5, use_graph=True, **kw)  # eta = 0 is accepted; graph replay
    assert np.array_equal(a.frac_x, d.frac_x) and np.array_equal(a.lattice, d.lattice)
    in_range = lambda r: (np.isfinite(r.frac_x).all() and np.isfinite(r.lattice).all() and (r.frac_x >= 0).all()
                          and (r.frac_x <= 1).all())
    for noise in ("device", "reference"):
        r = m.sample(multistep=True, noise=noise, **kw)
        assert in_range(r), noise
        # the host-noise loops hold the history and call the step export: the same deterministic positions and lengths
        assert np.array_equal(a.frac_x, r.frac_x) and np.array_equal(a.lattice, r.lattice), noise
    assert in_range(m.sample(counts, len(counts), num_steps=12, multistep=True, lattice_system="cubic", seed=3))
    assert in_range(m.sample(counts, len(counts), num_steps=12, multistep=True, fixed_cell=True, max_steps=5, seed=3))


def test_multistep_false_is_the_sampler(dev, fused_model):
    m, _ = fused_model
    counts = [3, 8, 1, 5]
    runs = []
    for kw in (dict(multistep=False), {}):
        torch.manual_seed(7)
        np.random.seed(7)
        runs.append(m.sample(counts, len(counts), num_steps=8, seed=42, **kw))
    a, b = runs
    assert np.array_equal(a.frac_x, b.frac_x) and np.array_equal(a.lattice, b.lattice)
    assert np.array_equal(a.atomic_numbers, b.atomic_numbers)


# -------------------------------------------------------------------------------------------------------------- 6
def test_analytic_trajectory_through_the_step_export(dev, fused_model):
    """Gaussian data N(0.3, 0.25), K = 12: the closed-form predictions, computed on the host from the device's state at every
    step, through arreau_reverse_step_multistep -- against the float64 trajectory of the restatement, within K times the per-step
    bound (the largest over the steps, evaluated on the float64 trajectory)."""
    m, om = fused_model
    eng = m.engine()
    sig, ab = _tables(om)
    K = 12
    sched = respacing.respaced_timesteps(T, K)
    case = Case(dev, seed=3, sampler_like=False)
    B, N = case.B, case.N
    n = case.na.double().numpy()[:, None]
    eps_fn, x0_fn = ms.gaussian_eps(sig, MEAN, VAR), ms.gaussian_x0(ab, MEAN, VAR)
    f, ty, le, lat = case.fresh()
    f.fill_(X_START)
    le.fill_(L_START)
    h = _history(case)
    x64, l64 = np.full((N, 3), float(np.float32(X_START))), np.full((B, 3), float(np.float32(L_START)))
    hx, hl, p = np.zeros_like(x64), np.zeros_like(l64), 0
    bound_x = bound_l = 0.0
    g = torch.Generator().manual_seed(5)
    for t, s in zip(sched, sched[1:] + [0]):
        # the float64 trajectory and the per-step bound on it
        e64, x064 = eps_fn(x64, t), x0_fn(l64, t)
        bound_x = max(bound_x, float(ms.position_error_bound(sig, x64, e64, hx, p, t, s).max()))
        bound_l = max(bound_l, float(ms.length_error_bound(ab, l64, x064, hl, p, t, s).max()))
        x64, hx, _ = ms.position_step(sig, x64, e64, hx, p, t, s, wrap=False)
        l64, _ = ms.length_step(ab, l64, x064, hl, p, t, s)
        hl, p = x064, t
        # the device: predictions from its own state
        eps = torch.as_tensor(eps_fn(f.cpu().double().numpy(), t), dtype=torch.float32).to(dev)
        len0 = torch.as_tensor(x0_fn(le.cpu().double().numpy(), t) / n, dtype=torch.float32).to(dev)
        logits, u = torch.randn(N, S, generator=g).to(dev), torch.rand(N, S, generator=g).to(dev)
        eng.reverse_step_multistep(f, ty, le, case.an, full_i32(B, t, dev), full_i32(B, s, dev), case.off, eps, logits, len0, u, lat, h,
                                   None, CLIP)
    assert (x64 > 0).all() and (x64 < 1).all()  # (the trajectory never wraps)
    e_x = float(np.abs(f.cpu().double().numpy() - x64).max())
    e_l = float(np.abs(le.cpu().double().numpy() - l64).max())
    print(f"K = {K}: positions {e_x:.3g} of {K * bound_x:.3g}, lengths {e_l:.3g} of {K * bound_l:.3g}")
    assert e_x <= K * bound_x and e_l <= K * bound_l
    # and the trajectory is the second-order one: closer to the probability-flow image than the eta = 0 error of this schedule
    want = ms.gaussian_position_flow(sig, MEAN, VAR, np.float32(X_START), sched[0], 0)
    assert float(np.abs(f.cpu().double().numpy() - want).max()) < 0.012
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 7
def test_the_library_rejects_what_the_rules_do_not_combine(dev, fused_model):
    """ARREAU_EINVAL before any work, through the C entry points themselves; the state and the history stay untouched."""
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    case = Case(dev, seed=3, counts=[3, 5])
    B, N = case.B, case.N
    f, ty, le, lat = case.fresh()
    h = _history(case, 0.25)
    h["hist_t_atom"].fill_(40)
    h["hist_t_len"].fill_(40)
    before = tuple(x.clone() for x in (f, ty, le) + _hist_bits(h))
    z = lambda *shape: torch.zeros(*shape, device=dev)
    p = _hip.ptr
    ws = eng.workspace(N, B)
    ptrs = [p(h[k]).value for k in ms.HISTORY_KEYS]
    good = _hip.MultistepC(*ptrs)
    holes = [_hip.MultistepC(*[None if j == i else v for j, v in enumerate(ptrs)]) for i in range(4)]
    mask = torch.ones(N, dtype=torch.uint8, device=dev)
    cond = _hip.SampleConditionC(p(z(N, 3)).value, p(mask).value, None, None, None, None)
    ref = ctypes.byref

    def loop(cond_=None, corr=None, res=None, hist=None):
        return _hip.lib().arreau_sample_loop_multistep(
            eng._handle, p(f), p(ty), p(le), p(case.an), p(case.off), B, N, 10, 3, 1, None, None, p(lat), p(ws), ws.numel(), 0,
            cond_, None, corr, res, None, hist, _hip.stream_ptr(dev))

    def step(hist):
        return _hip.lib().arreau_reverse_step_multistep(
            eng._handle, p(f), p(ty), p(le), p(case.an), p(full_i32(B, 10, dev)), p(full_i32(B, 5, dev)), p(case.off), B, N, p(z(N, 3)),
            p(z(N, S)), p(z(B, 3)), None, None, p(z(N, S) + 0.5), p(lat), CLIP, None, hist, _hip.stream_ptr(dev))

    assert loop(cond_=ref(cond), hist=ref(good)) == -1
    assert loop(corr=ref(_hip.CorrectorC(1, 0.16)), hist=ref(good)) == -1
    assert loop(res=ref(_hip.ResamplingC(2, 2, None, 0)), hist=ref(good)) == -1
    assert loop(hist=None) == -1 and step(None) == -1
    for hole in holes:
        assert loop(hist=ref(hole)) == -1 and step(ref(hole)) == -1
    torch.cuda.synchronize()
    assert_same_bits((f, ty, le) + _hist_bits(h), before, "a rejected call touched the state or the history")
    # the engine's own checks raise ValueError before the library is called
    with pytest.raises(ValueError, match="not combined with"):
        eng.sample_loop(f, ty, le, case.an, case.off, 10, 3, 1, None, lat, multistep=h, corrector=(1, 0.16))
    with pytest.raises(ValueError, match="not combined with"):
        eng.sample_loop(f, ty, le, case.an, case.off, 10, 3, 1, None, lat, multistep=h, eta=0.5)
    with pytest.raises(ValueError, match="multistep history"):
        eng.sample_loop(f, ty, le, case.an, case.off, 10, 3, 1, None, lat, multistep={k: h[k] for k in ms.HISTORY_KEYS[:3]})
    # a NULL corrector / resampling with no passes / an empty condition are the loop without them
    assert loop(cond_=ref(_hip.SampleConditionC()), corr=ref(_hip.CorrectorC(0, 0.0)), res=ref(_hip.ResamplingC(1, 1, None, 0)),
                hist=ref(good)) == 0
    torch.cuda.synchronize()
    assert not torch.equal(f, before[0]) and torch.equal(h["hist_t_len"], full_i32(B, 8, dev))
    eng.status(reset=True)
