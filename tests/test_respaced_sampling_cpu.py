"""Respaced sampling, the host side (no GPU): the schedule builder, validation of num_steps / timesteps before the engine is
touched, a float64 restatement of the respaced step rules (include/arreau_hip.h) against the oracle's one-step reverse updates
at s = t - 1, the time-homogeneity of the mask chain the species rule rests on, and generate.py's --num_steps."""
import math

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import respacing
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable
from oracle import diffusion as OD

ZT = AtomicNumberTable(list(range(1, 12)) + [2001])
S = len(ZT)


# ------------------------------------------------------------------------------------------------ the schedule builder
def test_full_schedule_is_every_timestep():
    for T in (3, 10, 100, 1000):
        assert respacing.respaced_timesteps(T, T - 1) == list(range(T - 1, 0, -1))


def test_every_k_at_t100_has_its_ends_length_and_distinct_steps():
    T = 100
    for K in range(2, T):
        ts = respacing.respaced_timesteps(T, K)
        assert len(ts) == K and ts[0] == T - 1 and ts[-1] == 1, K
        assert all(a > b for a, b in zip(ts, ts[1:])), K
        assert respacing.check_timesteps(T, ts) == ts


def test_known_values_at_t1000_k100():
    ts = respacing.respaced_timesteps(1000, 100)
    # t_i = 999 - round_half_up(998 i / 99)
    assert ts[:6] == [999, 989, 979, 969, 959, 949]
    assert ts[-4:] == [31, 21, 11, 1]
    assert ts[50] == 999 - (2 * 50 * 998 + 99) // 198 == 495
    assert all(10 <= a - b <= 11 for a, b in zip(ts, ts[1:]))


def test_next_table_holds_successors_and_one_above_entries():
    T = 100
    for ts in (respacing.respaced_timesteps(T, 7), [99, 98, 50, 2, 1], [1], list(range(99, 0, -1))):
        nxt = respacing.next_table(T, ts)
        assert nxt.dtype == torch.int32 and tuple(nxt.shape) == (T + 1,)
        for a, b in zip(ts, ts[1:] + [0]):
            assert int(nxt[a]) == b
            assert int(nxt[a + 1]) == a  # a loop call starting at a advances from a + 1
    assert respacing.next_table(T, list(range(99, 0, -1))).tolist()[1:] == list(range(0, 99)) + [99]


# -------------------------------------------------------------------------------- validation before the engine is used
class _NoEngine:
    """A model whose engine must not be reached: every ValueError below comes from validation first."""
    def engine(self):
        raise AssertionError("the engine was touched before the schedule was validated")


def _sample(**kw):
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = 100
    return dl.sample(model=_NoEngine(), z_table=ZT, num_atoms_per_sample=3, num_samples_in_batch=2, **kw)


@pytest.mark.parametrize("kw", [
    dict(num_steps=1), dict(num_steps=0), dict(num_steps=-5), dict(num_steps=100), dict(num_steps=1000),
    dict(num_steps=10.0), dict(num_steps="10"), dict(num_steps=True),
    dict(num_steps=10, timesteps=[99, 1]),
    dict(timesteps=[]), dict(timesteps=[100, 1]), dict(timesteps=[99, 2]), dict(timesteps=[99, 50, 50, 1]),
    dict(timesteps=[50, 99, 1]), dict(timesteps=[99, 10.5, 1]), dict(timesteps=[0]), dict(timesteps=[2, 1, 0]),
    dict(timesteps=5), dict(timesteps=[99, True]),
], ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()))
@pytest.mark.parametrize("noise", ["philox", "reference", "device"])
def test_invalid_schedules_raise_before_the_engine(kw, noise):
    with pytest.raises(ValueError):
        _sample(noise=noise, **kw)


def test_valid_schedules_reach_the_engine():
    for kw in (dict(num_steps=2), dict(num_steps=99), dict(timesteps=[1]), dict(timesteps=np.array([99, 40, 1])),
               dict(timesteps=(50, 1), max_steps=1)):
        with pytest.raises(AssertionError, match="engine was touched"):
            _sample(**kw)


def test_wrapper_validates_before_sampling():
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=S, seed=1, num_timesteps=30)
    m.engine = _NoEngine().engine
    for kw in (dict(num_steps=30), dict(num_steps=5, timesteps=[29, 1]), dict(timesteps=[29, 3])):
        with pytest.raises(ValueError):
            m.sample(3, 2, **kw)


# ------------------------------------------------------------------------- the step rules, restated in float64 (CPU)
def ve_to(sig, x, eps, t, s, z):
    """Rule 1: VE positions from t to s."""
    st2, ss2 = float(sig[t]) ** 2, float(sig[s]) ** 2
    mean = x - eps * (st2 - ss2)
    std = math.sqrt(ss2 * (st2 - ss2) / st2)
    return torch.remainder(mean + std * z, 1.0)


def vp_to(ab, betas, clipmax, x, x0, t, s, z):
    """Rule 2: VP lengths from t to s (betas[t] at stride 1, rule 4)."""
    ab_t, ab_s = float(ab[t]), float(ab[s])
    beta = float(betas[t]) if s == t - 1 else min(1.0 - ab_t / ab_s, clipmax)
    alpha = 1.0 - beta
    mean = (math.sqrt(ab_s) * beta * x0 + math.sqrt(alpha) * (1.0 - ab_s) * x) / (1.0 - ab_t)
    var = (1.0 - ab_s) * beta / (1.0 - ab_t)
    return mean + var * (z if t > 1 else torch.zeros_like(z))


def d3pm_logits_to(q1t, qmats, logits, xt, t, s):
    """Rule 3: the posterior logits from t to s (q_one_step_transposed at stride 1, rule 4)."""
    if t == 1:
        return logits
    fact1 = q1t[t - 1, xt, :] if s == t - 1 else qmats[t - s - 1][:, xt].T
    fact2 = torch.softmax(logits, dim=-1) @ qmats[s - 1]
    return torch.log(fact1 + OD.D3PM_EPS) + torch.log(fact2 + OD.D3PM_EPS)


def d3pm_to(q1t, qmats, logits, xt, t, s, u):
    post = d3pm_logits_to(q1t, qmats, logits, xt, t, s)
    u = torch.clip(u, OD.D3PM_EPS, 1.0)
    return torch.argmax(post + (-torch.log(-torch.log(u))) * (1.0 if t != 1 else 0.2), dim=-1)


@pytest.mark.parametrize("t", [99, 50, 7, 2, 1])
def test_restated_rules_at_stride_one_equal_the_oracle(t):
    T, N, B = 100, 9, 3
    dt = torch.float64
    g = torch.Generator().manual_seed(t)
    sig = OD.ve_sigmas(T, 0.001, 1.0, dtype=dt)
    ab, betas, _ = OD.vp_schedule(T, dtype=dt)
    q1t, qmats = OD.d3pm_buffers(T, S, dtype=dt)
    x = torch.rand(N, 3, generator=g, dtype=dt)
    eps = torch.randn(N, 3, generator=g, dtype=dt)
    z = torch.randn(N, 3, generator=g, dtype=dt)
    want = OD.ve_reverse(sig, x, eps, torch.full((N,), t), z)
    assert torch.allclose(ve_to(sig, x, eps, t, t - 1, z), want, rtol=0, atol=1e-12)
    L, L0, zl = (torch.randn(B, 3, generator=g, dtype=dt) for _ in range(3))
    want = OD.vp_reverse_given_x0(ab.to(dt), betas, L, L0, torch.tensor([t]), zl)
    assert torch.allclose(vp_to(ab.to(dt), betas, 0.999, L, L0, t, t - 1, zl), want, rtol=1e-12, atol=1e-12)
    logits = torch.randn(N, S, generator=g, dtype=dt)
    xt = torch.randint(0, S, (N,), generator=g)
    u = torch.rand(N, S, generator=g, dtype=dt)
    want = OD.d3pm_reverse(q1t, qmats, xt, logits, torch.full((N,), t), u)
    assert torch.equal(d3pm_to(q1t, qmats, logits, xt, t, t - 1, u), want)
    if t > 1:
        want = OD.d3pm_q_posterior_logits(q1t, qmats, logits, xt, torch.full((N,), t))
        assert torch.allclose(d3pm_logits_to(q1t, qmats, logits, xt, t, t - 1), want, rtol=0, atol=1e-12)


def test_respaced_vp_beta_is_the_composed_schedule():
    """1 - ab_t / ab_s is 1 - prod of the one-step alphas in between (before the clip): the t -> s jump of the same chain."""
    T = 100
    ab, betas, _ = OD.vp_schedule(T, dtype=torch.float64)
    ab = ab.double()
    for t, s in ((99, 80), (50, 10), (7, 1)):
        comp = 1.0 - float(torch.prod(1.0 - (1.0 - ab[s + 1:t + 1] / ab[s:t])))
        assert abs(min(1.0 - float(ab[t] / ab[s]), 0.999) - min(comp, 0.999)) < 1e-12


def test_mask_chain_is_time_homogeneous():
    """Rule 3 rests on Qbar_t = Qbar_s Qbar_{t-s} for the mask chain.  In float64 at T = 100 the two sides agree to the
    rounding of the running products (at most 5.6e-16 on entries of size <= 1; the products associate differently, so
    they are not bit for bit equal for every pair)."""
    T = 100
    _, qmats = OD.d3pm_buffers(T, S, dtype=torch.float64)
    for t in range(2, T + 1):
        for s in range(1, t):
            assert float((qmats[t - 1] - qmats[s - 1] @ qmats[t - s - 1]).abs().max()) <= 1e-15, (t, s)


def test_column_of_the_multi_step_matrix_is_zero_off_the_diagonal_except_for_the_mask():
    """The absorbing-chain shortcut of the column read (update_dev.h): Qbar_k[c, x] = 0 for c != x unless x is the mask class."""
    _, qmats = OD.d3pm_buffers(100, S, dtype=torch.float32)
    for k in (1, 2, 19, 98):
        q = qmats[k - 1]
        off = q - torch.diag(torch.diagonal(q))
        off[:, S - 1] = 0
        assert torch.count_nonzero(off) == 0


# ----------------------------------------------------------------------------------------------- generate.py
def test_generate_parses_num_steps():
    from arreau_amd import generate
    ap = generate.build_parser()
    assert ap.parse_args(["--model_path", "x.ckpt"]).num_steps is None
    assert ap.parse_args(["--model_path", "x.ckpt", "--num_steps", "20"]).num_steps == 20
    with pytest.raises(SystemExit):
        ap.parse_args(["--model_path", "x.ckpt", "--num_steps", "twenty"])
