"""DDIM-style sampling: an eta in [0, 1] that scales the noise a reverse step injects (Song, Meng & Ermon 2021, "Denoising
Diffusion Implicit Models").  eta = 1 is the ancestral step, eta = 0 a deterministic map from the state at t to the state at s;
the same trained network and the same schedule serve every eta.  The rules are stated in include/arreau_hip.h and run on the
device (arreau_sample_loop_eta, arreau_reverse_step_eta).  Here: the argument validation shared by sample(), the engine and
generate.py, and float64 numpy restatements of the two moves for the tests.  Nothing here touches the engine.
"""
import math
from numbers import Real

import numpy as np


def check_eta(eta) -> float:
    """eta validated: a finite number in [0, 1] (a bool or a string is not a number).  Returns it as a float."""
    if not isinstance(eta, Real) or isinstance(eta, bool):
        raise ValueError(f"eta must be a number in [0, 1], got {eta!r}")
    eta = float(eta)
    if not (math.isfinite(eta) and 0.0 <= eta <= 1.0):
        raise ValueError(f"eta must be finite and lie in [0, 1], got {eta}")
    return eta + 0.0  # (-0.0 -> 0.0)


def ve_coefficients(sig_t, sig_s, eta):
    """(w, c) of the position move x_s = remainder(x_t - w eps + c z, 1): r = sig_s / sig_t,
    dir = sig_s sqrt((1 - eta^2) + eta^2 r^2), w = sig_t (sig_t - dir), c = eta sig_s sqrt(1 - r^2)."""
    sig_t, sig_s, eta = float(sig_t), float(sig_s), float(eta)
    r = sig_s / sig_t
    direction = sig_s * math.sqrt((1.0 - eta * eta) + eta * eta * r * r)
    return sig_t * (sig_t - direction), eta * sig_s * math.sqrt(1.0 - r * r)


def ve_step(sigmas, x, eps, t, s, z, eta):
    """The position move from timestep t to s in float64 on the table `sigmas` [T+1]: x, eps, z arrays of one shape.  At
    eta = 0 z is not read (it may be None)."""
    w, c = ve_coefficients(sigmas[t], sigmas[s], eta)
    out = np.asarray(x, dtype=np.float64) - np.asarray(eps, dtype=np.float64) * w
    if eta > 0.0:
        out = out + c * np.asarray(z, dtype=np.float64)
    return np.remainder(out, 1.0)


def length_beta(alpha_bars, betas, t, s, clipmax):
    """The beta of the step from t to s as the ancestral step chooses it: the table at stride 1, otherwise
    min(1 - abar_t / abar_s, clipmax)."""
    return float(betas[t]) if s == t - 1 else min(1.0 - float(alpha_bars[t]) / float(alpha_bars[s]), float(clipmax))


def length_coefficients(ab_t, ab_s, beta, eta):
    """(c_x0, c_xt, c_z) of the length move l_s = c_x0 x0 + c_xt x_t + c_z z: den = 1 - abar_t, var = (1 - abar_s) beta / den,
    k = sqrt(max((1 - abar_s) (1 - eta^2 beta / den), 0) / den); c_x0 = sqrt(abar_s) - k sqrt(abar_t), c_xt = k, c_z = eta var."""
    ab_t, ab_s, beta, eta = float(ab_t), float(ab_s), float(beta), float(eta)
    den = 1.0 - ab_t
    var = (1.0 - ab_s) * beta / den
    k = math.sqrt(max((1.0 - ab_s) * (1.0 - eta * eta * beta / den), 0.0) / den)
    return math.sqrt(ab_s) - k * math.sqrt(ab_t), k, eta * var


def length_step(alpha_bars, betas, x, x0, t, s, z, eta, clipmax=0.999):
    """The length move from timestep t to s in float64 on the tables `alpha_bars`, `betas` [T+1]: x the current lengths, x0 the
    predicted clean lengths (pred_lengths_0 * num_atoms), z the draw (zero for t <= 1).  At eta = 0 z is not read."""
    c_x0, c_xt, c_z = length_coefficients(alpha_bars[t], alpha_bars[s], length_beta(alpha_bars, betas, t, s, clipmax), eta)
    out = c_x0 * np.asarray(x0, dtype=np.float64) + c_xt * np.asarray(x, dtype=np.float64)
    if eta > 0.0 and t > 1:
        out = out + c_z * np.asarray(z, dtype=np.float64)
    return out
