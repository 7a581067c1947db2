"""Predictor-corrector sampling, the host side (no GPU): the float64 restatement of one corrector move
(arreau_amd/diffusion/corrector.py; rule in include/arreau_hip.h) on hand-checkable cases, validation of corrector_steps /
corrector_snr in sample() before the engine is touched, and generate.py's --corrector_steps / --corrector_snr."""
import math

import numpy as np
import pytest

from arreau_amd.diffusion import corrector as pc
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable

ZT = AtomicNumberTable(list(range(1, 12)) + [2001])


# ------------------------------------------------------------------------------------------------------ the restatement
def test_displacement_is_the_snr_rule():
    rng = np.random.RandomState(0)
    frac = rng.uniform(0.3, 0.7, (5, 3))
    eps, z = rng.randn(5, 3) * 0.02, rng.randn(5, 3)
    sig, r = 0.05, 0.16
    ee, zz = float((eps ** 2).sum()), float((z ** 2).sum())
    a = 2 * r ** 2 * sig ** 2 * zz / ee
    b = 2 * r * sig ** 2 * math.sqrt(zz) / math.sqrt(ee)
    assert pc.coefficients(eps, z, sig, r) == pytest.approx((a, b), rel=1e-14)
    out = pc.corrector_move(frac, eps, z, sig, r, [5])
    np.testing.assert_allclose(out, frac - a * eps + b * z, rtol=0, atol=1e-15)  # no wrap: stays inside (0, 1)
    # the same move from Song et al.'s form: g = -eps / sig^2, gamma = 2 (r |z| / |g|)^2, x + gamma g + sqrt(2 gamma) z
    g = -eps / sig ** 2
    gamma = 2 * (r * math.sqrt(zz) / math.sqrt(float((g ** 2).sum()))) ** 2
    np.testing.assert_allclose(out, frac + gamma * g + math.sqrt(2 * gamma) * z, rtol=0, atol=1e-13)


def test_hand_checked_numbers():
    # one atom: eps = (3, 4, 0) -> |eps| = 5, z = (0, 0, 10) -> |z| = 10, q = 2; sig = 0.5, r = 0.25
    # a = 2 * 0.0625 * 0.25 * 4 = 0.125, c = 2 * 0.25 * 0.25 * 2 = 0.25
    a, c = pc.coefficients([3.0, 4.0, 0.0], [0.0, 0.0, 10.0], 0.5, 0.25)
    assert (a, c) == (0.125, 0.25)
    out = pc.corrector_move([[0.5, 0.5, 0.5]], [[3.0, 4.0, 0.0]], [[0.0, 0.0, 10.0]], 0.5, 0.25, [1])
    # (0.5 - 0.375, 0.5 - 0.5, 0.5 + 2.5) wrapped
    np.testing.assert_allclose(out, [[0.125, 0.0, 0.0]], atol=1e-15)


def test_zero_or_nonfinite_eps_leaves_the_crystal_unmoved():
    rng = np.random.RandomState(1)
    frac = rng.uniform(0, 1, (6, 3))
    z = rng.randn(6, 3)
    eps = rng.randn(6, 3)
    eps[:2] = 0.0          # crystal 0 (2 atoms): |eps| = 0
    eps[2, 1] = np.nan     # crystal 1 (3 atoms): not finite
    out = pc.corrector_move(frac, eps, z, 0.3, 0.16, [2, 3, 1])
    assert np.array_equal(out[:5], frac[:5])
    assert not np.array_equal(out[5], frac[5])
    assert pc.coefficients(np.zeros(3), np.ones(3), 0.3, 0.16) is None
    assert pc.coefficients([np.inf, 0, 0], np.ones(3), 0.3, 0.16) is None


def test_known_atoms_are_unmoved_and_left_out_of_the_norms():
    rng = np.random.RandomState(2)
    frac = rng.uniform(0.2, 0.8, (7, 3))
    eps, z = rng.randn(7, 3) * 0.05, rng.randn(7, 3)
    known = np.array([True, False, False, True, False, True, True])  # crystal 0 = atoms 0..3, crystal 1 = atoms 4..6
    sig = np.array([0.2, 0.4])
    out = pc.corrector_move(frac, eps, z, sig, 0.16, [4, 3], known=known)
    assert np.array_equal(out[known], frac[known])
    for rows, s in ((np.array([1, 2]), 0.2), (np.array([4]), 0.4)):  # the norms over the free atoms only
        a, c = pc.coefficients(eps[rows], z[rows], s, 0.16)
        np.testing.assert_allclose(out[rows], np.remainder(frac[rows] - a * eps[rows] + c * z[rows], 1.0), atol=1e-15)
    # a crystal with every position known is untouched
    out2 = pc.corrector_move(frac, eps, z, sig, 0.16, [4, 3], known=np.ones(7, dtype=bool))
    assert np.array_equal(out2, frac)


def test_outputs_lie_in_the_unit_interval():
    rng = np.random.RandomState(3)
    for trial in range(20):
        n = [1, 4, 150][trial % 3]
        frac = rng.uniform(0, 1, (n, 3))
        frac[0, 0] = 0.0
        out = pc.corrector_move(frac, rng.randn(n, 3) * 1e-3, rng.randn(n, 3) * 50, 1.0, 0.5, [n])
        assert ((out >= 0.0) & (out < 1.0)).all()
    # a tiny negative pre-wrap value must not come back as 1.0
    out = pc.corrector_move([[1e-18, 0.5, 0.5]], [[1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], 1.0, 0.16, [1])
    assert (out < 1.0).all()


# -------------------------------------------------------------------------------- validation before the engine is used
@pytest.mark.parametrize("steps,snr", [(0, 0.16), (1, 0.16), (16, 1e-3), (3, 2.0), (0, -1.0), (0, float("nan"))])
def test_valid_arguments(steps, snr):
    assert pc.check_corrector(steps, snr) == (steps, snr) or math.isnan(snr)


@pytest.mark.parametrize("steps,snr", [(-1, 0.16), (17, 0.16), (1.0, 0.16), ("1", 0.16), (True, 0.16), (None, 0.16),
                                       (1, 0.0), (1, -0.1), (1, float("nan")), (1, float("inf")), (1, "0.16"), (1, None)])
def test_invalid_arguments(steps, snr):
    with pytest.raises(ValueError):
        pc.check_corrector(steps, snr)


class _NoEngine:
    """A model whose engine must not be reached: every ValueError below comes from validation first."""
    def engine(self):
        raise AssertionError("the engine was touched before the corrector arguments were validated")


def _sample(**kw):
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = 100
    return dl.sample(model=_NoEngine(), z_table=ZT, num_atoms_per_sample=3, num_samples_in_batch=2, **kw)


@pytest.mark.parametrize("kw", [
    dict(corrector_steps=-1), dict(corrector_steps=17), dict(corrector_steps=1.5), dict(corrector_steps="2"),
    dict(corrector_steps=1, corrector_snr=0.0), dict(corrector_steps=1, corrector_snr=-0.16),
    dict(corrector_steps=2, corrector_snr=float("nan")), dict(corrector_steps=2, corrector_snr=float("inf")),
    dict(corrector_steps=1, num_steps=10, corrector_snr=0.0),
], ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()))
@pytest.mark.parametrize("noise", ["philox", "reference", "device"])
def test_invalid_corrector_raises_before_the_engine(kw, noise):
    with pytest.raises(ValueError):
        _sample(noise=noise, **kw)


def test_valid_corrector_reaches_the_engine():
    with pytest.raises(AssertionError, match="engine was touched"):
        _sample(corrector_steps=2, corrector_snr=0.1)


# ------------------------------------------------------------------------------------------------------------ generate.py
def test_generate_parser_takes_the_corrector_flags():
    from arreau_amd.generate import build_parser
    args = build_parser().parse_args(["--model_path", "x.ckpt"])
    assert (args.corrector_steps, args.corrector_snr) == (0, 0.16)
    args = build_parser().parse_args(["--model_path", "x.ckpt", "--corrector_steps", "2", "--corrector_snr", "0.2"])
    assert (args.corrector_steps, args.corrector_snr) == (2, 0.2)


@pytest.mark.parametrize("argv", [["--corrector_steps", "-1"], ["--corrector_steps", "17"], ["--corrector_steps", "1.5"],
                                  ["--corrector_snr", "0"], ["--corrector_snr", "-1"], ["--corrector_snr", "nan"],
                                  ["--corrector_snr", "inf"], ["--corrector_snr", "x"]])
def test_generate_parser_rejects_bad_corrector_flags(argv, capsys):
    from arreau_amd.generate import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--model_path", "x.ckpt"] + argv)
    assert "corrector" in capsys.readouterr().err
