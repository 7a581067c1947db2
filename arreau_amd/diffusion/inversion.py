"""Starting the sampler from given crystals: sampler states, forward noising to a level and DDIM inversion (Song, Meng & Ermon
2021, section 4.3).  The rules are stated in include/arreau_hip.h ("Starting the sampler from given crystals") and run on the
device (arreau_noise_state, arreau_invert_step, arreau_invert_loop).  Here: the state a run starts from, the argument
validation shared by sample(), noise_to(), encode() and generate.py, the ascending table of an inversion loop, float64 numpy
restatements of the two inversion moves for the tests, and the derived float32 error bound of the length move.  Nothing here
touches the engine.  The module imports without torch; `schedule_from` and `encode_levels` import `respacing`, which needs it.

Level convention: "a state at level t" is one whose first network evaluation is at timestep t; the prior draw of sample() is a
state at level T-1.
"""
from dataclasses import dataclass
from numbers import Integral
from typing import List, Optional, Sequence

import numpy as np


@dataclass
class SamplerState:
    """What a sampling run starts from, on the host: frac_x [N,3] fractional coordinates (unwrapped values are fine: the first
    step wraps), species [N] class indices, lengths [B,3] and angles [B,3] (radians) of the cells, num_atoms [B], and the level
    t in 1..T-1 the state is at.  length_tie: the lattice-system tie codes [B] the run keeps (lattice_systems.TIE_CODES), or
    None -- set by draw_initial_state / noise_to when they are given a lattice system."""
    frac_x: np.ndarray
    species: np.ndarray
    lengths: np.ndarray
    angles: np.ndarray
    num_atoms: np.ndarray
    t: int
    length_tie: Optional[np.ndarray] = None

    @property
    def B(self) -> int:
        return int(np.asarray(self.num_atoms).reshape(-1).shape[0])

    @property
    def N(self) -> int:
        return int(np.asarray(self.num_atoms).sum())


def _is_int(v) -> bool:
    return isinstance(v, Integral) and not isinstance(v, bool)


def check_level(T: int, t, what: str = "t") -> int:
    """A level a sampling run can enter at: an integer in 1..T-1."""
    if not _is_int(t) or not 1 <= int(t) <= int(T) - 1:
        raise ValueError(f"{what} must be an integer in 1..T-1 = {int(T) - 1}, got {t!r}")
    return int(t)


def check_state(state, T: int, num_atomic_states: Optional[int] = None) -> SamplerState:
    """A SamplerState whose arrays agree with each other and whose level lies in 1..T-1 (species in range when the number
    of classes is given).  Reads the arrays; draws nothing."""
    if not isinstance(state, SamplerState):
        raise ValueError(f"initial_state must be a SamplerState (noise_to, encode, draw_initial_state), got {type(state).__name__}")
    check_level(T, state.t, "initial_state.t")
    na = np.asarray(state.num_atoms).reshape(-1)
    if na.size < 1 or not np.issubdtype(na.dtype, np.integer) or int(na.min()) < 1:
        raise ValueError("initial_state.num_atoms must hold one positive integer per crystal")
    B, N = int(na.size), int(na.sum())
    for name, shape in (("frac_x", (N, 3)), ("species", (N,)), ("lengths", (B, 3)), ("angles", (B, 3))):
        if tuple(np.shape(getattr(state, name))) != shape:
            raise ValueError(f"initial_state.{name} must have shape {shape}, got {tuple(np.shape(getattr(state, name)))}")
    sp = np.asarray(state.species)
    if not np.issubdtype(sp.dtype, np.integer) or (N and (int(sp.min()) < 0 or (num_atomic_states is not None
                                                                                  and int(sp.max()) >= num_atomic_states))):
        raise ValueError("initial_state.species must hold class indices in 0..num_atomic_states-1")
    for name in ("frac_x", "lengths", "angles"):
        if not np.isfinite(np.asarray(getattr(state, name), dtype=np.float64)).all():
            raise ValueError(f"initial_state.{name} must be finite")
    if state.length_tie is not None:
        tie = np.asarray(state.length_tie).reshape(-1)
        if tie.shape != (B,) or not np.issubdtype(tie.dtype, np.integer) or int(tie.min()) < 0 or int(tie.max()) > 2:
            raise ValueError("initial_state.length_tie must hold one tie code in 0..2 per crystal")
    return state


def check_initial_state(state, T: int, *, condition=None, symmetry=None, lattice_system=None, num_atoms_per_sample=None,
                        num_samples_in_batch=None, num_atomic_states: Optional[int] = None) -> SamplerState:
    """What sample(initial_state=...) rejects before any work: a state together with a condition, symmetry specs or a lattice
    system (the state carries its own cell, angles and tie; the other two redraw or overwrite parts of it), a level outside
    1..T-1, arrays that disagree, and a batch that disagrees with num_atoms_per_sample / num_samples_in_batch when given."""
    with_state = [name for name, v in (("condition", condition), ("symmetry", symmetry), ("lattice_system", lattice_system))
                  if v is not None]
    if with_state:
        raise ValueError("initial_state= is not combined with " + ", ".join(f"{n}=" for n in with_state)
                         + " (the state decides positions, species, cell, angles and tie)")
    check_state(state, T, num_atomic_states)
    na = np.asarray(state.num_atoms).reshape(-1)
    if num_samples_in_batch is not None and int(num_samples_in_batch) != na.size:
        raise ValueError(f"num_samples_in_batch = {int(num_samples_in_batch)} disagrees with the initial state's {na.size} crystals")
    if num_atoms_per_sample is not None:
        if _is_int(num_atoms_per_sample):
            ok = bool((na == int(num_atoms_per_sample)).all())
        else:
            want = [int(v) for v in num_atoms_per_sample]
            ok = len(want) == na.size and bool((na == np.asarray(want)).all())
        if not ok:
            raise ValueError("num_atoms_per_sample disagrees with the initial state's atom counts")
    return state


def schedule_from(T: int, top: int, num_steps=None, timesteps=None) -> Optional[List[int]]:
    """The schedule of a run that enters at level `top`: respacing.resolve_schedule with that top; an explicit list must start
    at it.  None: every timestep top, top-1, ..., 1."""
    from . import respacing  # (imports torch for its device table)
    schedule = respacing.resolve_schedule(T, num_steps=num_steps, timesteps=timesteps, top=top)
    if timesteps is not None and schedule[0] != int(top):
        raise ValueError(f"timesteps must start at the initial state's level {int(top)}, got {schedule[0]}")
    return schedule


def encode_levels(T: int, t=None, num_steps=None, timesteps=None) -> List[int]:
    """The levels an encode() call visits, ascending: the schedule a sample() call would descend from level t (default T-1)
    with the same num_steps / timesteps (schedule_from), reversed -- so the decode visits exactly the levels the encode did.
    Without either keyword every level 1, 2, ..., t."""
    if timesteps is not None and t is None:
        try:
            t = list(timesteps)[0]
        except (TypeError, IndexError):
            raise ValueError("timesteps must be a non-empty sequence of integers") from None
    top = check_level(T, int(T) - 1 if t is None else t)
    schedule = schedule_from(T, top, num_steps=num_steps, timesteps=timesteps)
    return list(range(1, top + 1)) if schedule is None else schedule[::-1]


def check_levels(T: int, levels: Sequence[int]) -> List[int]:
    """The levels of an inversion loop, validated: integers, strictly ascending, within 1..T."""
    try:
        ls = list(levels)
    except TypeError:
        raise ValueError("levels must be a sequence of integers") from None
    if not ls:
        raise ValueError("levels must not be empty")
    if not all(_is_int(v) for v in ls):
        raise ValueError("levels must hold integers")
    ls = [int(v) for v in ls]
    if any(a >= b for a, b in zip(ls, ls[1:])):
        raise ValueError("levels must be strictly ascending")
    if ls[0] < 1 or ls[-1] > int(T):
        raise ValueError(f"levels must lie in 1..T = {int(T)}, got {ls[0]} .. {ls[-1]}")
    return ls


def ascending_table(T: int, levels: Sequence[int]) -> np.ndarray:
    """The device form of an inversion loop's levels u_0 < ... < u_n: int32 [T+1] with up[u_i] = u_{i+1}, and
    up[u_i - 1] = u_i for every u_i -- the "one below" entry a loop call entering at u_i advances from (it already holds when
    u_i - 1 is itself a level), mirroring the "one above" entry of respacing.next_table.  A climb may therefore be cut into calls
    at any of its levels.  Every other entry, the top's included, is 0: a level that does not climb, which the device clamps and
    flags if it is ever followed."""
    ls = check_levels(T, levels)
    up = np.zeros(int(T) + 1, dtype=np.int32)
    for u in ls:
        up[u - 1] = u
    for a, b in zip(ls, ls[1:]):
        up[a] = b
    return up


# ---- float64 restatements of the inversion step (rule 2 of the header section) ------------------------------------------
def invert_positions(sigmas, x, eps, s: int, t: int):
    """The position move from level s up to t on the table `sigmas` [T+1]: remainder(x + eps sig_s (sig_t - sig_s), 1)."""
    sig_s, sig_t = float(sigmas[s]), float(sigmas[t])
    return np.remainder(np.asarray(x, dtype=np.float64) + np.asarray(eps, dtype=np.float64) * sig_s * (sig_t - sig_s), 1.0)


def invert_rho(alpha_bars, s: int, t: int) -> float:
    """rho = sqrt((1 - abar_t) / (1 - abar_s)) >= 1 for s < t: 63 at T = 100 and 579 at T = 1000 from level 1 to T-1."""
    return float(np.sqrt((1.0 - float(alpha_bars[t])) / (1.0 - float(alpha_bars[s]))))


def invert_lengths(alpha_bars, l, x0, s: int, t: int):
    """The length move from level s up to t on the table `alpha_bars` [T+1]: l the lengths at s, x0 the predicted clean lengths
    (pred_lengths_0 * num_atoms): sqrt(abar_t) x0 + rho (l - sqrt(abar_s) x0)."""
    ab_s, ab_t = float(alpha_bars[s]), float(alpha_bars[t])
    x0 = np.asarray(x0, dtype=np.float64)
    return np.sqrt(ab_t) * x0 + invert_rho(alpha_bars, s, t) * (np.asarray(l, dtype=np.float64) - np.sqrt(ab_s) * x0)


F32_UNIT_ROUNDOFF = 2.0 ** -24
# The float32 length move against its exact value on the same float32 inputs and tables, to first order in u = 2^-24, with
# a = sqrt(abar_t), b = sqrt(abar_s) (a, b <= 1 <= rho), every operation correctly rounded (IEEE add / multiply; the library is
# built with correctly rounded float32 division and square root), each rounding a factor (1 + d), |d| <= u:
#   x0 = pooled * n                         one rounding:                                      u |x0|
#   A = fl(sqrt(abar_t)), B likewise        one rounding each
#   P1 = fl(A x0)                           three roundings (A, x0, the product):              3 u a |x0|
#   P2 = fl(B x0)                           likewise:                                          3 u b |x0|
#   D  = fl(l - P2)                         P2's error and one rounding of |D| <= |l| + b |x0|:   u |l| + 4 u b |x0|
#   R  = fl(sqrt(fl(fl(1 - abar_t) / fl(1 - abar_s))))   (u + u + u) / 2 + u:                  2.5 u rho
#   P3 = fl(R D)                            rho |D's error| + (2.5 + 1) u rho |D|:             u rho (4.5 |l| + 7.5 b |x0|)
#   out = fl(P1 + P3)                       both errors and one rounding of |out| <= a |x0| + rho (|l| + b |x0|):
#                                           u (4 a |x0| + rho (5.5 |l| + 8.5 b |x0|))  <=  12.5 u rho (|l| + |x0|).
# A fused multiply-add, where the compiler forms one, removes a rounding and only lowers this.  LENGTH_BOUND_ROUNDINGS rounds
# 12.5 up to 16 for the second-order terms (each below 16 u of the first-order ones) and the restatement's own float64
# rounding.  The bound grows with rho, not with the result: from level 1, abar_1 is close to 1 and rho (|l| + |x0|) is what the
# subtraction l - b x0 loses.
LENGTH_BOUND_ROUNDINGS = 16.0


def length_error_bound(alpha_bars, l, x0, s: int, t: int):
    """The bound of the float32 length move from s up to t against invert_lengths on the same inputs, elementwise:
    LENGTH_BOUND_ROUNDINGS * 2^-24 * rho * (|l| + |x0|) (the derivation is the comment above)."""
    mag = np.abs(np.asarray(l, dtype=np.float64)) + np.abs(np.asarray(x0, dtype=np.float64))
    return LENGTH_BOUND_ROUNDINGS * F32_UNIT_ROUNDOFF * invert_rho(alpha_bars, s, t) * mag
