"""Second-order multistep sampling (DPM-Solver++ 2M; Lu et al. 2022): the eta = 0 step extrapolated with the previous step's
prediction, at the same one network evaluation per step.  The rules are stated in include/arreau_hip.h and run on the device
(arreau_sample_loop_multistep, arreau_reverse_step_multistep).  Here: the argument validation shared by sample(), the engine and
generate.py, the allocator of the history buffers, float64 numpy restatements of both moves and of a whole K-step trajectory on
the model's float32 tables, and the derived float32 error bound of each move.  Nothing here touches the engine.
"""
import math
from typing import Callable, List, Sequence, Tuple

import numpy as np

from . import ddim

R_MIN, R_MAX = 1.0 / 3.0, 3.0  # the step-size guard: outside it a move is first order
HISTORY_KEYS = ("hist_eps", "hist_x0", "hist_t_atom", "hist_t_len")


# ---- validation ---------------------------------------------------------------------------------------------------------
def check_multistep(multistep, *, eta=None, condition=None, corrector_steps=0, resample_passes=1, symmetry=None) -> bool:
    """`multistep` validated (a bool) together with what it is not combined with (rule 6 of the header section): a condition,
    corrector steps, resampling passes > 1, symmetry and an eta other than None or 0 raise ValueError.  Returns the bool."""
    if not isinstance(multistep, (bool, np.bool_)):
        raise ValueError(f"multistep must be True or False, got {multistep!r}")
    if not multistep:
        return False
    unsupported = [name for name, on in (("condition=", condition is not None), ("corrector_steps > 0", int(corrector_steps) > 0),
                                         ("resample_passes > 1", int(resample_passes) > 1), ("symmetry=", symmetry is not None),
                                         (f"eta={eta!r}", eta is not None and float(eta) != 0.0)) if on]
    if unsupported:
        raise ValueError("multistep=True is not combined with " + ", ".join(unsupported)
                         + " (the multistep step is the deterministic eta = 0 step, extrapolated)")
    return True


def allocate_history(N: int, B: int, device):
    """The four history buffers of a run on `device`, empty (every level 0): a dict of contiguous tensors hist_eps [N,3] and
    hist_x0 [B,3] (float32), hist_t_atom [N] and hist_t_len [B] (int32)."""
    import torch
    return {"hist_eps": torch.zeros((N, 3), device=device, dtype=torch.float32),
            "hist_x0": torch.zeros((B, 3), device=device, dtype=torch.float32),
            "hist_t_atom": torch.zeros((N,), device=device, dtype=torch.int32),
            "hist_t_len": torch.zeros((B,), device=device, dtype=torch.int32)}


def empty_history(history) -> None:
    """The caller's duty whenever the state changes outside a step: every level back to 0."""
    history["hist_t_atom"].zero_()
    history["hist_t_len"].zero_()


# ---- float64 restatements (rules 1 and 2 of the header section) ----------------------------------------------------------
def usable(p: int, t: int, T: int) -> bool:
    """A history level p is usable for the step that leaves t when t < p <= T (0: empty)."""
    return int(t) < int(p) <= int(T)


def _guard(p, t, s, T, r) -> bool:
    return usable(p, t, T) and int(s) >= 1 and math.isfinite(r) and R_MIN <= r <= R_MAX


def position_ratio(sigmas, p: int, t: int, s: int) -> float:
    """r = log(sig_p / sig_t) / log(sig_t / sig_s), the step-size ratio in log-sigma time."""
    return math.log(float(sigmas[p]) / float(sigmas[t])) / math.log(float(sigmas[t]) / float(sigmas[s]))


def position_step(sigmas, x, eps, hist_e, p: int, t: int, s: int, wrap: bool = True) -> Tuple[np.ndarray, np.ndarray, bool]:
    """The position move from t to s on the table `sigmas` [T+1] with the history (hist_e, level p): returns (x_s, e, second)
    -- the new positions (wrapped into [0, 1) unless wrap is False), e = sig_t eps (what the history takes) and whether the move
    was second order."""
    T = len(sigmas) - 1
    sig_t, sig_s = float(sigmas[t]), float(sigmas[s])
    x, e = np.asarray(x, dtype=np.float64), np.asarray(eps, dtype=np.float64) * sig_t
    second = usable(p, t, T) and _guard(p, t, s, T, position_ratio(sigmas, p, t, s))
    if second:
        d = e + (e - np.asarray(hist_e, dtype=np.float64)) / (2.0 * position_ratio(sigmas, p, t, s))
        out = x - (sig_t - sig_s) * d
    else:  # the eta = 0 move (ddim.ve_step without its wrap)
        out = x - e * (sig_t - sig_s)
    return (np.remainder(out, 1.0) if wrap else out), e, second


def half_log_snr(ab: float) -> float:
    """lam = 0.5 (log abar - log(1 - abar)); -inf / +inf at abar = 0 / 1."""
    ab = float(ab)
    with np.errstate(divide="ignore"):
        return float(0.5 * (np.log(np.float64(ab)) - np.log(np.float64(1.0 - ab))))


def length_ratio(alpha_bars, p: int, t: int, s: int) -> float:
    """r = (lam_t - lam_p) / (lam_s - lam_t), the step-size ratio in half-log-SNR time (nan / 0 where a lam is infinite)."""
    lam_t, lam_p, lam_s = (half_log_snr(alpha_bars[u]) for u in (t, p, s))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((np.float64(lam_t) - lam_p) / (np.float64(lam_s) - lam_t))


def length_step(alpha_bars, l, x0, hist_x0, p: int, t: int, s: int) -> Tuple[np.ndarray, bool]:
    """The length move from t to s on the table `alpha_bars` [T+1] with the history (hist_x0, level p): l the lengths at t, x0
    the predicted clean lengths (pred_lengths_0 * num_atoms, or the tied group's mean).  Returns (l_s, second).  The history
    then takes x0.  At eta = 0 neither beta nor the clip enters."""
    T = len(alpha_bars) - 1
    ab_t, ab_s = float(alpha_bars[t]), float(alpha_bars[s])
    l, x0 = np.asarray(l, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    c_x0, k, _ = ddim.length_coefficients(ab_t, ab_s, 0.0, 0.0)
    second = usable(p, t, T) and _guard(p, t, s, T, length_ratio(alpha_bars, p, t, s))
    D = x0 + (x0 - np.asarray(hist_x0, dtype=np.float64)) / (2.0 * length_ratio(alpha_bars, p, t, s)) if second else x0
    return c_x0 * D + k * l, second


def tie_inputs(x0, l, hist_x0, codes):
    """Tie rule on the inputs of the length move ([B,3] arrays, codes per crystal): the axes of a tied group take the leader's
    x_t and history value and the group's mean x0 (summed in axis order)."""
    x0, l, h = (np.array(a, dtype=np.float64) for a in (x0, l, hist_x0))
    for b, code in enumerate(codes if codes is not None else []):
        if code > 0:
            n = int(code) + 1
            x0[b, :n] = sum(x0[b, j] for j in range(n)) / n
            l[b, :n], h[b, :n] = l[b, 0], h[b, 0]
    return x0, l, h


def _pairs(schedule: Sequence[int]):
    ts = [int(t) for t in schedule]
    return list(zip(ts, ts[1:] + [0]))


def position_trajectory(sigmas, schedule: Sequence[int], x, predict: Callable[[np.ndarray, int], np.ndarray],
                        multistep: bool = True, wrap: bool = False) -> Tuple[np.ndarray, List[bool]]:
    """A whole run of the position moves along `schedule` (t_1 > ... > t_K, the last step to level 0) from x, eps = predict(x, t)
    at every step, starting with an empty history.  multistep False: every move the eta = 0 move.  Returns the final positions
    (unwrapped unless wrap) and, per step, whether it was second order."""
    x = np.asarray(x, dtype=np.float64)
    hist, p, orders = np.zeros_like(x), 0, []
    for t, s in _pairs(schedule):
        x, e, second = position_step(sigmas, x, predict(x, t), hist, p if multistep else 0, t, s, wrap)
        hist, p = e, t
        orders.append(second)
    return x, orders


def length_trajectory(alpha_bars, schedule: Sequence[int], l, predict: Callable[[np.ndarray, int], np.ndarray],
                      multistep: bool = True) -> Tuple[np.ndarray, List[bool]]:
    """The same for the lengths: x0 = predict(l, t)."""
    l = np.asarray(l, dtype=np.float64)
    hist, p, orders = np.zeros_like(l), 0, []
    for t, s in _pairs(schedule):
        x0 = np.asarray(predict(l, t), dtype=np.float64)
        l, second = length_step(alpha_bars, l, x0, hist, p if multistep else 0, t, s)
        hist, p = x0, t
        orders.append(second)
    return l, orders


# ---- the analytic case: Gaussian data, closed-form predictions and probability-flow map -----------------------------------
def gaussian_eps(sigmas, mean: float, var: float):
    """Data N(mean, var) under the VE process: eps(x, t) = (x - mean) / (var + sig_t^2), the predictor's convention
    (x0 estimate x - sig_t^2 eps), unwrapped."""
    return lambda x, t: (np.asarray(x, dtype=np.float64) - mean) / (var + float(sigmas[t]) ** 2)


def gaussian_position_flow(sigmas, mean: float, var: float, x, t: int, s: int):
    """The probability-flow image at level s of x at level t: (x_s - mean) / sqrt(var + sig_s^2) is constant."""
    return mean + (np.asarray(x, dtype=np.float64) - mean) * math.sqrt((var + float(sigmas[s]) ** 2) / (var + float(sigmas[t]) ** 2))


def gaussian_x0(alpha_bars, mean: float, var: float):
    """Data N(mean, var) under the VP process: x0(l, t) = E[l_0 | l_t] = mean + sqrt(abar) var (l - sqrt(abar) mean) /
    (abar var + 1 - abar)."""
    def predict(l, t):
        ab = float(alpha_bars[t])
        return mean + math.sqrt(ab) * var * (np.asarray(l, dtype=np.float64) - math.sqrt(ab) * mean) / (ab * var + 1.0 - ab)
    return predict


def gaussian_length_flow(alpha_bars, mean: float, var: float, l, t: int, s: int):
    """The probability-flow image at level s of l at level t: (l_s - sqrt(abar_s) mean) / sqrt(abar_s var + 1 - abar_s) is
    constant."""
    ab_t, ab_s = float(alpha_bars[t]), float(alpha_bars[s])
    scale = math.sqrt((ab_s * var + 1.0 - ab_s) / (ab_t * var + 1.0 - ab_t))
    return math.sqrt(ab_s) * mean + (np.asarray(l, dtype=np.float64) - math.sqrt(ab_t) * mean) * scale


# ---- the float32 bounds of the two moves ---------------------------------------------------------------------------------
F32_UNIT_ROUNDOFF = 2.0 ** -24
LOGF_ROUNDINGS = 2.0   # the device logf is accurate to 1 ulp, i.e. a relative error of at most 2 u
BOUND_MARGIN = 1.25    # the second-order terms in u (each below u times a first-order one) and the restatement's own rounding
X0_ROUNDINGS = 4.0     # x0 = pooled * n, and for a tied group two additions and a division: at most four roundings
# Both bounds are derived the way inversion.py derives its length bound: the float32 move against its exact value on the same
# float32 inputs and tables, to first order in u = 2^-24, every operation correctly rounded (IEEE add / multiply; the library is
# built with correctly rounded float32 division and square root) and contributing a factor (1 + d), |d| <= u; logf contributes
# LOGF_ROUNDINGS u relative.  A fused multiply-add, where the compiler forms one, removes a rounding and only lowers them.
#
# The conditioning of r.  L = logf(fl(a / b)): the quotient's rounding moves the logarithm by u ABSOLUTE, logf's own error is
# LOGF_ROUNDINGS u |L|, so L has the relative error u / |L| + LOGF_ROUNDINGS u.  On the geometric sigma ladder 1e-3..1 the
# logarithm of adjacent levels is ln(1000) / T: 0.069 at T = 100, 0.0069 at T = 1000, where 1 / |L| = 145.  Positions:
#   r = fl(L1 / L2):   rho_r = u (1 / |L1| + 1 / |L2| + 2 LOGF_ROUNDINGS + 1)       (295 u at adjacent timesteps of T = 1000, 34 u at T = 100)
# Lengths, lam_u = 0.5 fl(fl(log abar_u) - fl(log fl(1 - abar_u))), with a1 = |log abar_u|, a2 = |log(1 - abar_u)|: logf's errors
# LOGF_ROUNDINGS u (a1 + a2), the rounding of 1 - abar_u moves its logarithm by u, the subtraction rounds 2 |lam_u|:
#   E_u = 0.5 u (LOGF_ROUNDINGS (a1 + a2) + 1 + 2 |lam_u|)      (absolute)
#   r = fl(fl(lam_t - lam_p) / fl(lam_s - lam_t)):   rho_r = (E_t + E_p) / |lam_t - lam_p| + (E_s + E_t) / |lam_s - lam_t| + 3 u
# At adjacent timesteps of T = 1000 of the cosine schedule (length_ratio_error evaluated on the model's table) rho_r is 140 u at
# the top (t = 998), 2400 u = 1.4e-4 through mid-schedule (t = 900 .. 100, where lam moves by about 2e-3 per level against E of
# about u) and 150 u at t = 2; at T = 100, 90 to 120 u.  It multiplies only the extrapolation term (x0 - x0_p) / (2 r), which is
# itself the small difference of two consecutive predictions.
#
# Positions, out = remainder(x - h d, 1), h = fl(sig_t - sig_s), e = fl(eps sig_t) (u |e|), second order:
#   g = fl(e - e_p)            u |e| + u |g|
#   c = fl(g / fl(2 r))        dg / (2 r) + |c| (rho_r + u)                              (2 r is exact)
#   d = fl(e + c)              u |e| + dc + u |d|
#   v = fl(x - fl(h d))        h dd + 2 u h |d| (h's rounding, the product's) + u |v|
#   remainder: fmodf is exact; the shift of a negative value up by one rounds once: u
# first order: d = e, c = g = 0.  position_error_bound returns BOUND_MARGIN times the sum.
#
# Lengths, out = cA D + k x_t with A = fl(sqrt(abar_s)), Q = fl(sqrt(abar_t)) (u each), k = fl(sqrt(fl(fl(1 - abar_s) / fl(1 -
# abar_t)))) (2.5 u relative, k <= 1 for s < t), cA = fl(A - fl(k Q)): u A + 4.5 u k Q + u |cA| <= 6.5 u (A, k Q <= 1):
#   x0                          X0_ROUNDINGS u |x0| against the float64 x0 of the same pooled outputs
#   g = fl(x0 - x0_p)           dx0 + u |g|                                               (x0_p is an input: the history as stored)
#   c = fl(g / fl(2 r))         dg / (2 r) + |c| (rho_r + u)
#   D = fl(x0 + c)              dx0 + dc + u |D|
#   out = fl(fl(cA D) + fl(k x_t))   6.5 u |D| + |cA| dD + u |cA D| + 3.5 u k |x_t| + u |out|
# first order: D = x0.  length_error_bound returns BOUND_MARGIN times the sum.


def position_ratio_error(sigmas, p: int, t: int, s: int) -> float:
    """rho_r of the position move: the relative error bound of the float32 r (the comment above)."""
    l1 = abs(math.log(float(sigmas[p]) / float(sigmas[t])))
    l2 = abs(math.log(float(sigmas[t]) / float(sigmas[s])))
    return F32_UNIT_ROUNDOFF * (1.0 / l1 + 1.0 / l2 + 2.0 * LOGF_ROUNDINGS + 1.0)


def _lam_error(ab: float) -> float:
    a1, a2 = abs(math.log(ab)), abs(math.log(1.0 - ab))
    return 0.5 * F32_UNIT_ROUNDOFF * (LOGF_ROUNDINGS * (a1 + a2) + 1.0 + 2.0 * abs(half_log_snr(ab)))


def length_ratio_error(alpha_bars, p: int, t: int, s: int) -> float:
    """rho_r of the length move (the comment above); p, t, s levels with finite lam (a second-order move has them)."""
    e_p, e_t, e_s = (_lam_error(float(alpha_bars[u])) for u in (p, t, s))
    lam_p, lam_t, lam_s = (half_log_snr(alpha_bars[u]) for u in (p, t, s))
    return (e_t + e_p) / abs(lam_t - lam_p) + (e_s + e_t) / abs(lam_s - lam_t) + 3.0 * F32_UNIT_ROUNDOFF


def position_error_bound(sigmas, x, eps, hist_e, p: int, t: int, s: int):
    """The bound of the float32 position move against position_step on the same inputs, elementwise (on the circle)."""
    u = F32_UNIT_ROUNDOFF
    T = len(sigmas) - 1
    sig_t, sig_s = float(sigmas[t]), float(sigmas[s])
    h = abs(sig_t - sig_s)
    x, e = np.abs(np.asarray(x, dtype=np.float64)), np.asarray(eps, dtype=np.float64) * sig_t
    second = usable(p, t, T) and _guard(p, t, s, T, position_ratio(sigmas, p, t, s))
    if second:
        r = position_ratio(sigmas, p, t, s)
        g = e - np.asarray(hist_e, dtype=np.float64)
        c = g / (2.0 * r)
        d = e + c
        dc = (u * np.abs(e) + u * np.abs(g)) / (2.0 * r) + np.abs(c) * (position_ratio_error(sigmas, p, t, s) + u)
    else:
        d, dc = e, 0.0
    dd = u * np.abs(e) + dc + u * np.abs(d)
    return BOUND_MARGIN * (h * dd + 2.0 * u * h * np.abs(d) + u * (x + h * np.abs(d)) + u)


def length_error_bound(alpha_bars, l, x0, hist_x0, p: int, t: int, s: int):
    """The bound of the float32 length move against length_step on the same inputs, elementwise."""
    u = F32_UNIT_ROUNDOFF
    T = len(alpha_bars) - 1
    ab_t, ab_s = float(alpha_bars[t]), float(alpha_bars[s])
    l, x0 = np.abs(np.asarray(l, dtype=np.float64)), np.asarray(x0, dtype=np.float64)
    c_x0, k, _ = ddim.length_coefficients(ab_t, ab_s, 0.0, 0.0)
    dx0 = X0_ROUNDINGS * u * np.abs(x0)
    second = usable(p, t, T) and _guard(p, t, s, T, length_ratio(alpha_bars, p, t, s))
    if second:
        r = length_ratio(alpha_bars, p, t, s)
        g = x0 - np.asarray(hist_x0, dtype=np.float64)
        c = g / (2.0 * r)
        D = x0 + c
        dc = (dx0 + u * np.abs(g)) / (2.0 * r) + np.abs(c) * (length_ratio_error(alpha_bars, p, t, s) + u)
    else:
        D, dc = x0, 0.0
    dD = dx0 + dc + u * np.abs(D)
    out = np.abs(c_x0 * D) + k * l
    return BOUND_MARGIN * (6.5 * u * np.abs(D) + abs(c_x0) * dD + u * np.abs(c_x0 * D) + 3.5 * u * k * l + u * out)
