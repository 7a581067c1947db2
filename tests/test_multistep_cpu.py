"""Second-order multistep sampling, the host side (no GPU): what sample(multistep=True) rejects before any work, the order of
the float64 restatement (arreau_amd/diffusion/multistep.py; rules in include/arreau_hip.h) on the analytic Gaussian case, the
step-size guard, and the derived float32 bounds against the moves evaluated in float32 operation by operation."""
import numpy as np
import pytest

from arreau_amd.diffusion import ddim, multistep as ms, respacing
from tests.multistep_cases import MEAN, STEP_SCHEDULES, T, VAR, analytic_errors, tables


# ------------------------------------------------------------------------------------------------- 1. validation
class NoEngine:
    def engine(self):
        raise AssertionError("the engine was touched")


def _dl():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = T
    return dl


def _rng_states():
    import torch
    return np.random.get_state()[1].copy(), torch.random.get_rng_state().clone()


def _assert_nothing_drawn(before):
    import torch
    assert np.array_equal(np.random.get_state()[1], before[0]) and torch.equal(torch.random.get_rng_state(), before[1])


def test_sample_rejects_multistep_combinations_before_any_work():
    from arreau_amd.diffusion import symmetry as sy
    from arreau_amd.diffusion.conditioning import SampleCondition
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    gen = sy.SymmetrySpec.general_positions(["-x,y+1/2,-z+1/2", "-x,-y,-z"], 2, "monoclinic")
    tmpl = SampleResult(frac_x=np.zeros((5, 3)), atomic_numbers=np.ones(5), lattice=np.tile(np.eye(3) * 4, (2, 1, 1)),
                        num_atoms=np.array([3, 2]), idx_start=np.array([0, 3]))
    cond = SampleCondition.from_sample_result(tmpl, fix_positions=True)
    before = _rng_states()
    kw = dict(model=NoEngine(), z_table=list(range(5)), num_atoms_per_sample=[3, 2], num_samples_in_batch=2)
    for extra, match in ((dict(condition=cond), "condition="), (dict(corrector_steps=1), "corrector_steps > 0"),
                         (dict(resample_passes=2), "resample_passes > 1"), (dict(symmetry=gen), "symmetry="),
                         (dict(symmetry=[gen, None]), "symmetry="), (dict(eta=0.5), "eta=0.5"), (dict(eta=1.0), "eta=1.0"),
                         (dict(condition=cond, eta=0.3), "condition=, eta=0.3")):
        for noise in ("philox", "reference", "device"):
            with pytest.raises(ValueError, match="multistep=True is not combined with " + match):
                _dl().sample(multistep=True, noise=noise, **extra, **kw)
    for bad in ("yes", 1, None, 0.0):
        with pytest.raises(ValueError, match="multistep must be True or False"):
            _dl().sample(multistep=bad, **kw)
    _assert_nothing_drawn(before)
    # what is accepted reaches the engine
    for extra in ({}, dict(eta=0.0), dict(eta=None, num_steps=12), dict(timesteps=[99, 60, 50, 45, 1], fixed_cell=True),
                  dict(lattice_system="cubic", max_steps=3), dict(noise="reference"), dict(noise="device", num_steps=5)):
        with pytest.raises(AssertionError, match="engine was touched"):
            _dl().sample(multistep=True, **extra, **kw)
    # off, the combinations are the sampler's own business
    for extra in (dict(corrector_steps=1), dict(resample_passes=2), dict(eta=0.5)):
        with pytest.raises(AssertionError, match="engine was touched"):
            _dl().sample(multistep=False, **extra, **kw)
    _assert_nothing_drawn(before)


def test_wrapper_and_module_validate():
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=12, seed=1, num_timesteps=30)
    m.engine = NoEngine().engine
    before = _rng_states()
    with pytest.raises(ValueError, match="corrector_steps > 0"):
        m.sample(4, 2, multistep=True, corrector_steps=2)
    with pytest.raises(ValueError, match="eta=0.25"):
        m.sample(4, 2, multistep=True, eta=0.25)
    _assert_nothing_drawn(before)
    with pytest.raises(AssertionError, match="engine was touched"):
        m.sample(4, 2, multistep=True, num_steps=12)
    assert ms.check_multistep(False, eta=0.7, corrector_steps=3) is False and ms.check_multistep(True, eta=-0.0) is True


def test_generate_parses_the_multistep_flag():
    from arreau_amd import generate
    ap = generate.build_parser()
    base = ["--model_path", "x.ckpt"]
    assert ap.parse_args(base).multistep is False
    a = ap.parse_args(base + ["--multistep", "--num_steps", "12", "--eta", "0"])
    assert a.multistep is True and a.num_steps == 12 and a.eta == 0.0


# ------------------------------------------------------------------------------------------------- 2. the analytic order
def test_analytic_order_of_the_restatement(capsys):
    """Gaussian data N(0.3, 0.25): closed-form predictions, closed-form probability-flow map, the project's evenly spaced
    schedules at T = 100.  Second order against first: the thresholds sit under theory and under the measured table (printed)."""
    err = {K: analytic_errors(K) for K in (12, 24, 48, 96)}
    with capsys.disabled():
        print("\n  K   positions: multistep   eta=0   ratio     lengths: multistep   eta=0   ratio")
        for K, (pm, p1, lm, l1) in err.items():
            print(f"  {K:<3d} {pm:21.3e} {p1:9.3e} {p1 / pm:6.2f} {lm:23.3e} {l1:9.3e} {l1 / lm:6.2f}")
    for K in (12, 24, 48):
        assert err[K][0] * 3 <= err[K][1], ("positions", K, err[K])
    assert err[24][0] >= 3 * err[48][0], ("positions, error per doubling of K", err[24][0], err[48][0])
    assert err[48][2] * 2 <= err[48][3], ("lengths", 48, err[48])
    assert err[96][2] * 4 <= err[96][3], ("lengths", 96, err[96])


def test_trajectory_in_two_calls_is_the_trajectory():
    """position_step / length_step carried by hand with the history kept across a cut: the trajectory functions' result."""
    sig, ab, _ = tables()
    sched = respacing.respaced_timesteps(T, 12)
    eps_fn, x0_fn = ms.gaussian_eps(sig, MEAN, VAR), ms.gaussian_x0(ab, MEAN, VAR)
    x, l = np.array([0.9, 0.1]), np.array([1.7, -0.4])
    want_x, orders_x = ms.position_trajectory(sig, sched, x, eps_fn)
    want_l, orders_l = ms.length_trajectory(ab, sched, l, x0_fn)
    hx, hl, p = np.zeros(2), np.zeros(2), 0
    for t, s in zip(sched, sched[1:] + [0]):
        x, hx, _ = ms.position_step(sig, x, eps_fn(x, t), hx, p, t, s, wrap=False)
        x0 = x0_fn(l, t)
        l, _ = ms.length_step(ab, l, x0, hl, p, t, s)
        hl, p = x0, t
    assert np.array_equal(x, want_x) and np.array_equal(l, want_l)
    assert orders_x[0] is False and orders_x[-1] is False and orders_l[0] is False and orders_l[-1] is False
    assert sum(orders_x) == 10 and sum(orders_l) == 8  # the lengths' guard refuses two more moves of this schedule


# ------------------------------------------------------------------------------------------------- 3. the guard
@pytest.mark.parametrize("sched", list(STEP_SCHEDULES), ids=lambda s: "-".join(map(str, s)))
def test_the_guard_takes_the_stated_branches(sched):
    sig, ab, _ = tables()
    rng = np.random.RandomState(1)
    x, l, hx, hl, p = rng.rand(4, 3), rng.rand(2, 3) * 4 + 2, np.zeros((4, 3)), np.zeros((2, 3)), 0
    got_x, got_l = [], []
    for t, s in zip(sched, sched[1:]):
        eps, x0 = rng.randn(4, 3) * 0.3, rng.rand(2, 3) * 5 + 1
        first_x = np.remainder(ddim.ve_step(sig, x, eps, t, s, None, 0.0), 1.0)
        first_l = ddim.length_step(ab, tables()[2], l, x0, t, s, None, 0.0, 0.999)
        x_new, e, second_x = ms.position_step(sig, x, eps, hx, p, t, s)
        l_new, second_l = ms.length_step(ab, l, x0, hl, p, t, s)
        # a first-order move is the eta = 0 move; a second-order one is not
        d = np.abs(x_new - first_x)
        assert (np.minimum(d, 1 - d).max() <= 1e-15) == (not second_x), (t, s)
        assert (np.abs(l_new - first_l).max() <= 1e-13) == (not second_l), (t, s)
        got_x.append(second_x)
        got_l.append(second_l)
        x, l, hx, hl, p = x_new, l_new, e, x0, t
    assert got_x == STEP_SCHEDULES[sched]["positions"] and got_l == STEP_SCHEDULES[sched]["lengths"]


def test_the_ratios_the_cases_state():
    sig, ab, _ = tables()
    assert abs(ms.position_ratio(sig, 99, 60, 50) - 3.9) < 1e-5 and abs(ms.position_ratio(sig, 60, 50, 45) - 2.0) < 1e-5
    assert 11.9 < ms.length_ratio(ab, 99, 60, 50) < 12.1 and 2.0 < ms.length_ratio(ab, 60, 50, 45) < 2.05
    assert 1.70 < ms.length_ratio(ab, 99, 98, 97) < 1.72 and 1.40 < ms.length_ratio(ab, 98, 97, 96) < 1.42
    assert 0.58 < ms.length_ratio(ab, 3, 2, 1) < 0.60
    # an unusable history, a target of 0 and a ratio that is not finite: first order
    x, e = np.array([0.2]), np.array([0.1])
    for p, t, s in ((0, 50, 45), (50, 50, 45), (40, 50, 45), (T + 1, 50, 45), (2, 1, 0)):
        assert ms.position_step(sig, x, e, e, p, t, s)[2] is False and ms.length_step(ab, x, e, e, p, t, s)[1] is False
    assert ms.length_step(ab, x, e, e, T, T - 1, T - 2)[1] in (False, True)  # abar_T is tiny but positive on this table
    # the first respaced step of the cosine schedule at T = 1000 is several times the second in half-log-SNR units: beyond the guard
    ab1000 = tables(1000)[1]
    for K in (12, 24):
        sK = respacing.respaced_timesteps(1000, K)
        assert ms.length_ratio(ab1000, sK[0], sK[1], sK[2]) > 4.0


# ------------------------------------------------------------------------------------------------- 4. the bounds
def _f32_position_move(sig, x, eps, he, p, t, s):
    f = np.float32
    st, ss, sp = f(sig[t]), f(sig[s]), f(sig[p])
    e = eps * st
    r = np.log(sp / st, dtype=f) / np.log(st / ss, dtype=f)
    d = e + (e - he) / (f(2) * r)
    return np.remainder(x - (st - ss) * d, f(1)), e


def _f32_length_move(ab, l, x0, h0, p, t, s):
    f = np.float32
    lam = lambda a: f(0.5) * (np.log(f(a), dtype=f) - np.log(f(1) - f(a), dtype=f))
    at, as_ = f(ab[t]), f(ab[s])
    r = (lam(ab[t]) - lam(ab[p])) / (lam(ab[s]) - lam(ab[t]))
    k = np.sqrt(np.maximum(f(1) - as_, f(0)) / (f(1) - at), dtype=f)
    D = x0 + (x0 - h0) / (f(2) * r)
    return (np.sqrt(as_, dtype=f) - k * np.sqrt(at, dtype=f)) * D + k * l


@pytest.mark.parametrize("T_", [100, 1000])
def test_the_bounds_hold_for_the_moves_in_float32(T_):
    """Second-order moves at adjacent timesteps (where r is worst conditioned) and at wide ones, in float32 operation by
    operation, against the float64 restatement on the same float32 inputs: within the derived bounds, and the bounds are not
    slack by orders of magnitude."""
    sig, ab, _ = tables(T_)
    rng = np.random.RandomState(T_)
    f = np.float32
    triples = [(T_ - 1, T_ - 2, T_ - 3), (T_ // 2 + 1, T_ // 2, T_ // 2 - 1), (3, 2, 1), (60 * T_ // 100, 50 * T_ // 100, 45 * T_ // 100)]
    worst_x = worst_l = 0.0
    for p, t, s in triples:
        x, eps, he = rng.rand(200, 3).astype(f), (rng.randn(200, 3) * 0.5).astype(f), (rng.randn(200, 3) * 0.3).astype(f)
        got, e32 = _f32_position_move(sig, x, eps, he, p, t, s)
        assert got.dtype == f
        want, e64, second = ms.position_step(sig, x, eps, he, p, t, s)
        assert second
        d = np.abs(got.astype(np.float64) - want)
        ratio = np.minimum(d, 1 - d) / ms.position_error_bound(sig, x, eps, he, p, t, s)
        assert ratio.max() <= 1.0, (p, t, s, ratio.max())
        assert np.abs(e32.astype(np.float64) - e64).max() <= 2.0 ** -24 * np.abs(e64).max()
        worst_x = max(worst_x, float(ratio.max()))
        l, x0, h0 = (rng.randn(200, 3) * 3).astype(f), (rng.rand(200, 3) * 7).astype(f), (rng.rand(200, 3) * 7).astype(f)
        got = _f32_length_move(ab, l, x0, h0, p, t, s)
        assert got.dtype == f
        want, second = ms.length_step(ab, l, x0, h0, p, t, s)
        assert second
        ratio = np.abs(got.astype(np.float64) - want) / ms.length_error_bound(ab, l, x0, h0, p, t, s)
        assert ratio.max() <= 1.0, (p, t, s, ratio.max())
        worst_l = max(worst_l, float(ratio.max()))
    assert worst_x > 0.02 and worst_l > 0.02, (worst_x, worst_l)
    # the conditioning of r at adjacent timesteps, as DESIGN.md states it
    u = 2.0 ** -24
    if T_ == 1000:
        assert 290 < ms.position_ratio_error(sig, 501, 500, 499) / u < 300
        assert 2000 < ms.length_ratio_error(ab, 501, 500, 499) / u < 2600
    else:
        assert 30 < ms.position_ratio_error(sig, 51, 50, 49) / u < 40
        assert 80 < ms.length_ratio_error(ab, 99, 98, 97) / u < 130
