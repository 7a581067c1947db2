"""Respaced sampling: the sampler on a subsequence of the trained timesteps (Nichol & Dhariwal 2021, section 4).

A schedule is a strictly descending list of timesteps t_1 > ... > t_K with t_1 <= T-1 and t_K = 1; the step that leaves
t_i produces the state at t_{i+1} (0 after t_K).  The device reads it as a next-timestep table (include/arreau_hip.h,
arreau_sample_schedule).  Host-side plumbing only: nothing here touches the engine.
"""
from numbers import Integral
from typing import List, Optional, Sequence

import torch


def _top(T: int, top) -> int:
    """The level a run enters at: T-1 (None: the prior draw), or a given level in 1..T-1 (a run started from a given state)."""
    if top is None:
        return int(T) - 1
    if not _is_int(top) or not 1 <= int(top) <= int(T) - 1:
        raise ValueError(f"top must be an integer in 1..T-1 = {int(T) - 1}, got {top!r}")
    return int(top)


def respaced_timesteps(T: int, num_steps: int, top: Optional[int] = None) -> List[int]:
    """The evenly spaced schedule of K = num_steps steps: t_i = (T-1) - (2 i (T-2) + (K-1)) // (2 (K-1)), i = 0..K-1
    (round-half-up of i (T-2) / (K-1) below T-1).  K = T-1 is T-1, T-2, ..., 1.  `top` (default T-1): the schedule of a run
    that enters at level top, the same formula with top in the place of T-1 (and top-1 in that of T-2): top, ..., 1."""
    T, K, top = int(T), int(num_steps), _top(T, top)
    if not 2 <= K <= top:
        raise ValueError(f"num_steps must lie in 2..{'T-1' if top == T - 1 else 'top'} = {top}, got {K}")
    return [top - (2 * i * (top - 1) + (K - 1)) // (2 * (K - 1)) for i in range(K)]


def _is_int(v) -> bool:
    return isinstance(v, Integral) and not isinstance(v, bool)


def check_timesteps(T: int, timesteps: Sequence[int], top: Optional[int] = None) -> List[int]:
    """An explicit schedule, validated: integers, strictly descending, first <= T-1 (<= top when given), last == 1."""
    try:
        ts = list(timesteps)
    except TypeError:
        raise ValueError("timesteps must be a sequence of integers") from None
    if not ts:
        raise ValueError("timesteps must not be empty")
    if not all(_is_int(t) for t in ts):
        raise ValueError("timesteps must hold integers")
    ts = [int(t) for t in ts]
    if any(a <= b for a, b in zip(ts, ts[1:])):
        raise ValueError("timesteps must be strictly descending")
    if top is not None and ts[0] > _top(T, top):
        raise ValueError(f"timesteps must start at or below top = {int(top)}, got {ts[0]}")
    if ts[0] > T - 1:
        raise ValueError(f"timesteps must start at or below T-1 = {T - 1}, got {ts[0]}")
    if ts[-1] != 1:
        raise ValueError(f"timesteps must end at 1, got {ts[-1]}")
    return ts


def resolve_schedule(T: int, num_steps=None, timesteps=None, top: Optional[int] = None) -> Optional[List[int]]:
    """The schedule of a sample() call: None (every timestep, the plain loop) when neither keyword is given.  `top` (default
    T-1): the level the run enters at."""
    if num_steps is not None and timesteps is not None:
        raise ValueError("give num_steps or timesteps, not both")
    if num_steps is not None:
        if not _is_int(num_steps):
            raise ValueError("num_steps must be an integer")
        return respaced_timesteps(T, num_steps, top)
    if timesteps is not None:
        return check_timesteps(T, timesteps, top)
    return None


def next_table(T: int, schedule: Sequence[int]) -> torch.Tensor:
    """The device form of a schedule: int32 [T+1] with next[t_i] = t_{i+1}, next[1] = 0, and next[t_i + 1] = t_i for every
    t_i (the "one above" entry a loop call starting at t_i advances from; it already holds when t_i + 1 is scheduled)."""
    nxt = torch.zeros(T + 1, dtype=torch.int32)
    for t in schedule:
        nxt[t + 1] = t
    for a, b in zip(schedule, list(schedule[1:]) + [0]):
        nxt[a] = b
    return nxt
