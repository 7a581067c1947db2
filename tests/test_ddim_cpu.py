"""DDIM-style sampling, the host side (no GPU): validation of eta before the engine is touched, the float64 restatements of the
two moves (arreau_amd/diffusion/ddim.py; rules in include/arreau_hip.h) against the ancestral step's closed forms at eta = 1,
what eta = 0 does not read, the last step of the lengths, and generate.py's --eta."""
import math

import numpy as np
import pytest

from arreau_amd.diffusion import ddim
from oracle import diffusion as OD

T = 100
CLIP = 0.999


def _tables():
    """The model's float32 tables, held as float64 (what the device reads, without further rounding)."""
    import torch
    sig = OD.ve_sigmas(T, 0.001, 1.0, dtype=torch.float32).double().numpy()
    ab, betas, _ = OD.vp_schedule(T, dtype=torch.float32)
    return sig, ab.double().numpy(), betas.double().numpy()


# --------------------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("eta", [0, 0.5, 1, 0.0, 1.0, np.float32(0.25)])
def test_check_eta_accepts(eta):
    out = ddim.check_eta(eta)
    assert isinstance(out, float) and out == float(eta)


@pytest.mark.parametrize("eta", [-0.1, 1.5, float("nan"), "0.5", float("inf"), True, None])
def test_check_eta_rejects(eta):
    with pytest.raises(ValueError, match="eta"):
        ddim.check_eta(eta)


class NoEngine:
    def engine(self):
        raise AssertionError("the engine was touched")


def _dl():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = T
    return dl


@pytest.mark.parametrize("noise", ["philox", "reference", "device"])
def test_sample_rejects_bad_eta_before_any_work(noise):
    state = np.random.get_state()
    for eta in (-0.1, 1.5, float("nan"), "0.5"):
        with pytest.raises(ValueError, match="eta"):
            _dl().sample(model=NoEngine(), z_table=None, num_atoms_per_sample=3, num_samples_in_batch=2, noise=noise, eta=eta)
    assert np.array_equal(np.random.get_state()[1], state[1])  # nothing drawn


def test_sample_rejects_symmetry_with_eta_before_any_work():
    from arreau_amd.diffusion import symmetry as sy
    gen = sy.SymmetrySpec.general_positions(["-x,y+1/2,-z+1/2", "-x,-y,-z"], 2, "monoclinic")
    with pytest.raises(ValueError, match="not supported with eta"):
        _dl().sample(model=NoEngine(), z_table=None, symmetry=gen, num_samples_in_batch=2, eta=0.0)
    # a valid eta reaches the engine
    with pytest.raises(AssertionError, match="engine was touched"):
        _dl().sample(model=NoEngine(), z_table=list(range(5)), num_atoms_per_sample=3, num_samples_in_batch=2, eta=0.5)


def test_wrapper_validates_eta_before_sampling():
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=12, seed=1, num_timesteps=30)
    m.engine = NoEngine().engine
    for eta in (2.0, -1e-9, float("inf")):
        with pytest.raises(ValueError, match="eta"):
            m.sample(3, 2, eta=eta)


# ------------------------------------------------------------------------------------------------- the moves at eta = 1
def test_ve_move_at_eta_one_is_the_respaced_closed_form():
    sig, _, _ = _tables()
    worst = 0.0
    for t in range(1, T + 1):
        for s in range(0, t):
            w, c = ddim.ve_coefficients(sig[t], sig[s], 1.0)
            st2, ss2 = sig[t] ** 2, sig[s] ** 2
            worst = max(worst, abs(w - (st2 - ss2)), abs(c - math.sqrt(ss2 * (st2 - ss2) / st2)))
    assert worst <= 1e-13, worst
    # and through the step itself
    rng = np.random.RandomState(0)
    x, eps, z = rng.rand(7, 3), rng.randn(7, 3), rng.randn(7, 3)
    for t, s in ((99, 80), (50, 10), (7, 1), (2, 1), (1, 0), (60, 59)):
        st2, ss2 = sig[t] ** 2, sig[s] ** 2
        want = np.remainder(x - eps * (st2 - ss2) + math.sqrt(ss2 * (st2 - ss2) / st2) * z, 1.0)
        d = np.abs(ddim.ve_step(sig, x, eps, t, s, z, 1.0) - want)
        assert np.minimum(d, 1 - d).max() <= 1e-13


def test_length_move_at_eta_one_is_the_posterior_mean():
    """betas recomputed in float64 as 1 - abar_t / abar_s, unclipped pairs only: the two coefficients of the posterior mean
    (sqrt(abar_s) beta / den, sqrt(1 - beta) (1 - abar_s) / den) and the ancestral amplitude of the noise."""
    _, ab, _ = _tables()
    worst, n = 0.0, 0
    for t in range(1, T):
        for s in range(0, t):
            beta = 1.0 - ab[t] / ab[s]
            if beta >= CLIP:
                continue
            n += 1
            den = 1.0 - ab[t]
            c_x0, c_xt, c_z = ddim.length_coefficients(ab[t], ab[s], beta, 1.0)
            worst = max(worst, abs(c_x0 - math.sqrt(ab[s]) * beta / den), abs(c_xt - math.sqrt(1.0 - beta) * (1.0 - ab[s]) / den))
            assert c_z == (1.0 - ab[s]) * beta / den
    assert n > 4000 and worst <= 1e-12, (n, worst)


def test_length_beta_is_the_ancestral_choice():
    _, ab, betas = _tables()
    assert ddim.length_beta(ab, betas, 60, 59, CLIP) == betas[60]
    assert ddim.length_beta(ab, betas, 60, 40, CLIP) == 1.0 - ab[60] / ab[40]
    assert ddim.length_beta(ab, betas, 99, 1, CLIP) == CLIP


# ------------------------------------------------------------------------------------------------- the moves at eta = 0
def test_eta_zero_does_not_read_the_noise():
    sig, ab, betas = _tables()
    rng = np.random.RandomState(1)
    x, eps = rng.rand(5, 3), rng.randn(5, 3)
    L, L0 = rng.rand(2, 3) + 1, rng.rand(2, 3) + 1
    for t, s in ((99, 80), (50, 49), (2, 1), (1, 0)):
        a = ddim.ve_step(sig, x, eps, t, s, np.full((5, 3), np.nan), 0.0)
        assert np.isfinite(a).all() and np.array_equal(a, ddim.ve_step(sig, x, eps, t, s, None, 0.0))
        assert np.array_equal(a, np.remainder(x - eps * (sig[t] * (sig[t] - sig[s])), 1.0))
        b = ddim.length_step(ab, betas, L, L0, t, s, np.full((2, 3), np.nan), 0.0, CLIP)
        assert np.isfinite(b).all() and np.array_equal(b, ddim.length_step(ab, betas, L, L0, t, s, None, 0.0, CLIP))
    # with an eta the noise is read
    assert np.isnan(ddim.ve_step(sig, x, eps, 50, 10, np.full((5, 3), np.nan), 0.3)).all()
    assert np.isnan(ddim.length_step(ab, betas, L, L0, 50, 10, np.full((2, 3), np.nan), 0.3, CLIP)).all()


@pytest.mark.parametrize("eta", [0.0, 0.3, 1.0])
def test_last_length_step_is_exactly_x0(eta):
    _, ab, betas = _tables()
    assert ab[0] == 1.0
    rng = np.random.RandomState(2)
    L, L0 = rng.rand(4, 3) * 5, rng.rand(4, 3) * 7
    assert np.array_equal(ddim.length_step(ab, betas, L, L0, 1, 0, rng.randn(4, 3), eta, CLIP), L0)


def test_deterministic_length_move_is_ddim():
    """eta = 0: l_s = sqrt(abar_s) x0 + sqrt(1 - abar_s) (x_t - sqrt(abar_t) x0) / sqrt(1 - abar_t), Song et al.'s equation 12."""
    _, ab, betas = _tables()
    for t, s in ((99, 80), (50, 10), (7, 1), (60, 59)):
        c_x0, c_xt, c_z = ddim.length_coefficients(ab[t], ab[s], ddim.length_beta(ab, betas, t, s, CLIP), 0.0)
        k = math.sqrt((1 - ab[s]) / (1 - ab[t]))
        assert abs(c_xt - k) <= 1e-15 and abs(c_x0 - (math.sqrt(ab[s]) - k * math.sqrt(ab[t]))) <= 1e-15 and c_z == 0.0


# ---------------------------------------------------------------------------------------------------------- generate.py
def test_generate_parses_eta():
    from arreau_amd import generate
    ap = generate.build_parser()
    assert ap.parse_args(["--model_path", "x.ckpt"]).eta is None
    assert ap.parse_args(["--model_path", "x.ckpt", "--eta", "0"]).eta == 0.0
    assert ap.parse_args(["--model_path", "x.ckpt", "--num_steps", "20", "--eta", "0.5"]).eta == 0.5
    for bad in ("2", "-0.5", "nan", "half"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--model_path", "x.ckpt", "--eta", bad])
