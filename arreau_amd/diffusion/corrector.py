"""Predictor-corrector sampling: Langevin corrector steps on the fractional coordinates (Song et al. 2021, "Score-Based
Generative Modeling through SDEs", Algorithms 2 and 5).  At every visited timestep t, M corrector moves come before the
predictor step that leaves t; the rule is stated in include/arreau_hip.h and runs on the device (arreau_sample_loop_corrected,
arreau_corrector_step).  Here: the argument validation shared by sample() and generate.py, and a float64 numpy restatement
of one corrector move for the tests.  Nothing here touches the engine.
"""
import math
from numbers import Integral, Real

import numpy as np

DEFAULT_SNR = 0.16  # Song et al.'s setting for VE processes
MAX_STEPS = 16      # ARREAU_MAX_CORRECTOR_STEPS


def check_corrector(steps, snr):
    """(steps, snr) validated: an integer 0 <= steps <= MAX_STEPS and, when steps > 0, a finite snr > 0.  Returns
    (int steps, float snr)."""
    if not isinstance(steps, Integral) or isinstance(steps, bool):
        raise ValueError(f"corrector_steps must be an integer, got {steps!r}")
    steps = int(steps)
    if not 0 <= steps <= MAX_STEPS:
        raise ValueError(f"corrector_steps must lie in 0..{MAX_STEPS}, got {steps}")
    if not isinstance(snr, Real) or isinstance(snr, bool):
        raise ValueError(f"corrector_snr must be a number, got {snr!r}")
    snr = float(snr)
    if steps > 0 and not (math.isfinite(snr) and snr > 0.0):
        raise ValueError(f"corrector_snr must be finite and > 0, got {snr}")
    return steps, snr


def coefficients(eps, z, sigma, snr):
    """(a, c) of one crystal's move x <- remainder(x - a eps + c z, 1): q = |z| / |eps| over the given components,
    a = 2 r^2 sig^2 q^2, c = 2 r sig^2 q.  None when |eps|^2 is 0 or not finite (the crystal is not moved)."""
    eps = np.asarray(eps, dtype=np.float64).reshape(-1)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    ee, zz = float(np.dot(eps, eps)), float(np.dot(z, z))
    if not (ee > 0.0 and math.isfinite(ee)):
        return None
    q = math.sqrt(zz) / math.sqrt(ee)
    sig2 = float(sigma) ** 2
    a, c = 2.0 * snr * snr * sig2 * q * q, 2.0 * snr * sig2 * q
    if not (math.isfinite(a) and math.isfinite(c)):
        return None
    return a, c


def corrector_move(frac, eps, z, sigma, snr, num_atoms, known=None):
    """One corrector move of a batch in float64: frac, eps, z [N,3]; sigma = ve_sigmas[t] per crystal ([B] or a scalar);
    num_atoms [B] (atoms of a crystal contiguous); known [N] bool (optional): positions that are neither moved nor counted.
    Returns the new fractional coordinates in [0, 1)."""
    frac = np.array(frac, dtype=np.float64).reshape(-1, 3)
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, 3)
    z = np.asarray(z, dtype=np.float64).reshape(-1, 3)
    num_atoms = np.asarray(num_atoms, dtype=np.int64).reshape(-1)
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), num_atoms.shape)
    moved = np.ones(len(frac), dtype=bool) if known is None else ~np.asarray(known, dtype=bool).reshape(-1)
    out = frac.copy()
    first = 0
    for b, n in enumerate(num_atoms):
        rows = np.arange(first, first + n)
        rows = rows[moved[rows]]
        first += n
        ac = coefficients(eps[rows], z[rows], sig[b], snr) if len(rows) else None
        if ac is None:
            continue
        a, c = ac
        x = np.remainder(frac[rows] - a * eps[rows] + c * z[rows], 1.0)
        x[x >= 1.0] = 0.0  # (a tiny negative value rounds to 1.0 in float64)
        out[rows] = x
    return out
