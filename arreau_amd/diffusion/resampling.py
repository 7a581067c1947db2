"""RePaint resampling (Lugmayr et al., CVPR 2022, section 4.2): the visited steps in blocks of J, every block run R times, and
every pass after the first starts with a forward jump of the whole state from the block's bottom back up to its top.  The
rules are stated in include/arreau_hip.h ("RePaint resampling") and run on the device (arreau_sample_loop_resampled,
arreau_resample_jump).  Here: the argument validation shared by sample() and generate.py, the ordered event list of a run
(what the host-noise modes execute and the tests compare against), and a float64 numpy restatement of the jump for the tests.
Nothing here touches the engine.
"""
from numbers import Integral
from typing import List, NamedTuple, Sequence

import numpy as np

MAX_PASSES = 64  # ARREAU_MAX_RESAMPLE_PASSES
D3PM_EPS = 1e-6  # d3pm.py:23


def check_resampling(passes, jump_length):
    """(passes, jump_length) validated: integers 1 <= passes <= MAX_PASSES and jump_length >= 1.  Returns (int, int)."""
    for name, v in (("resample_passes", passes), ("jump_length", jump_length)):
        if not isinstance(v, Integral) or isinstance(v, bool):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    passes, jump_length = int(passes), int(jump_length)
    if not 1 <= passes <= MAX_PASSES:
        raise ValueError(f"resample_passes must lie in 1..{MAX_PASSES}, got {passes}")
    if jump_length < 1:
        raise ValueError(f"jump_length must be >= 1, got {jump_length}")
    return passes, jump_length


class Event(NamedTuple):
    """One event of a resampled run: kind "step" (the step that leaves t and produces s, in pass r) or "jump" (the forward
    jump from the block's bottom s up to its top t, in front of pass r)."""
    kind: str
    t: int
    s: int
    r: int


def plan(steps: Sequence[int], successor: int, passes: int, jump_length: int) -> List[Event]:
    """The ordered events of a run over the visited steps t_1 > ... > t_n (`steps`), where `successor` is t_{n+1}, the timestep
    the last step produces.  Block k covers steps kJ+1 .. min(kJ+J, n); every block runs `passes` passes, and passes 1..R-1
    start with a jump from the block's bottom t_{min(kJ+J,n)+1} up to its top t_{kJ+1}.  passes = 1: the plain list of steps."""
    passes, jump_length = check_resampling(passes, jump_length)
    steps = [int(t) for t in steps]
    after = steps[1:] + [int(successor)]
    out: List[Event] = []
    for a in range(0, len(steps), jump_length):
        b = min(a + jump_length, len(steps))
        top, bottom = steps[a], after[b - 1]
        for r in range(passes):
            if r > 0:
                out.append(Event("jump", top, bottom, r))
            out.extend(Event("step", steps[i], after[i], r) for i in range(a, b))
    return out


# ---- float64 restatement of the jump s -> t ------------------------------------------------------------------------------
def jump_positions(frac, s, t, sigmas, z):
    """VE_pbc.forward composed: remainder(x + sqrt(sig_t^2 - sig_s^2) z, 1).  s, t: scalars or per-row arrays [N]."""
    frac, z = np.asarray(frac, np.float64), np.asarray(z, np.float64)
    sig = np.asarray(sigmas, np.float64)
    st, ss = sig[np.asarray(t)], sig[np.asarray(s)]
    sd = np.sqrt((st - ss) * (st + ss))
    out = np.remainder(frac + np.reshape(sd, (-1, 1)) * z, 1.0)
    out[out >= 1.0] = 0.0  # (a tiny negative value rounds to 1.0 in float64)
    return out


def jump_lengths(lengths, s, t, alpha_bars, z):
    """VP_lattice.forward composed: sqrt(abar_t / abar_s) l + sqrt(1 - abar_t / abar_s) z, abar_0 = 1.  s, t per row [B]."""
    lengths, z = np.asarray(lengths, np.float64), np.asarray(z, np.float64)
    ab = np.asarray(alpha_bars, np.float64)
    s, t = np.broadcast_to(np.asarray(s), (len(lengths),)), np.broadcast_to(np.asarray(t), (len(lengths),))
    ab_s = np.where(s > 0, ab[s], 1.0)
    ratio = (ab[t] / ab_s)[:, None]
    return np.sqrt(ratio) * lengths + np.sqrt(1.0 - ratio) * z


def jump_species(types, s, t, q_mats, u, eps=D3PM_EPS):
    """D3PM.q_sample from x_s: argmax_c [log(Qbar_{t-s}[x, c] + eps) - log(-log(clip(u_c, eps, 1)))], Qbar_k = q_mats[k-1],
    the first index on ties.  s, t per row [N]."""
    types = np.asarray(types, np.int64)
    q = np.asarray(q_mats, np.float64)
    s, t = np.broadcast_to(np.asarray(s), types.shape), np.broadcast_to(np.asarray(t), types.shape)
    rows = q[t - s - 1, types]  # [N, S]
    u = np.clip(np.asarray(u, np.float64), eps, 1.0)
    return np.argmax(np.log(rows + eps) - np.log(-np.log(u)), axis=1)


def jump(frac, types, lengths, s, t, num_atoms, sigmas, alpha_bars, q_mats, z_frac, z_lengths, u_types, const_types=None,
         fixed_cell=False, type_known=None):
    """The whole jump of a batch in float64: s, t per crystal [B]; num_atoms [B] (atoms of a crystal contiguous).  Held, not
    jumped: every species when const_types is given, the lengths when fixed_cell, and the species of type_known [N] (bool).
    Returns (frac, types, lengths)."""
    num_atoms = np.asarray(num_atoms, np.int64)
    s_c, t_c = np.asarray(s, np.int64).reshape(-1), np.asarray(t, np.int64).reshape(-1)
    s_a, t_a = np.repeat(s_c, num_atoms), np.repeat(t_c, num_atoms)
    f = jump_positions(frac, s_a, t_a, sigmas, z_frac)
    ln = np.array(lengths, np.float64) if fixed_cell else jump_lengths(lengths, s_c, t_c, alpha_bars, z_lengths)
    ty = np.array(types, np.int64)
    if const_types is None:
        new = jump_species(ty, s_a, t_a, q_mats, u_types)
        keep = np.zeros(len(ty), bool) if type_known is None else np.asarray(type_known, bool)
        ty = np.where(keep, ty, new)
    return f, ty, ln
