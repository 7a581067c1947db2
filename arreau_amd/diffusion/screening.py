"""Structural screen of generated crystals: shortest interatomic contact, cell volume, mask state (arreau_crystal_screen,
arreau_amd/csrc/screen.hip; the rules are written out in include/arreau_hip.h).  Here: the criteria and their validation, the
flag constants, the entry point that needs no engine (`screen`), and two numpy restatements of the kernel for the tests --
`screen_reference_f32`, one float32 operation at a time in the kernel's order (the bit-for-bit yardstick, as
tests/neighbor_reference.py is for the neighbour list), and `screen_reference_f64`, the same rules in float64 on an image
range one shell wider.  The restatements need numpy alone.

The rule, per crystal with cell rows a_0, a_1, a_2 (L), n atoms with fractional coordinates f:
  * cross products c_0 = a_1 x a_2, c_1 = a_2 x a_0, c_2 = a_0 x a_1 (each component u_p v_q - u_q v_p); det = (a_0x c_0x +
    a_0y c_0y) + a_0z c_0z; volume = |det|; plane spacing h_k = volume / sqrt((c_kx^2 + c_ky^2) + c_kz^2); number_density =
    n / volume; shells q_k = search_radius / h_k, n_k = max(1, ceil(q_k));
  * NONFINITE when a cell entry or a coordinate is not finite; CELL when not (volume >= min_volume), volume is not finite or
    not (q_k <= max_shells) for an axis;
  * w = f - floor(f), a result >= 1 becomes 0; p_d = (w_0 L_0d + w_1 L_1d) + w_2 L_2d;
  * shift of image (n_1, n_2, n_3), -n_k <= n_k' <= n_k: s_d = (n_1 L_0d + n_2 L_1d) + n_3 L_2d; images in lexicographic order,
    m = ((n_1 + N_1)(2 N_2 + 1) + (n_2 + N_2))(2 N_3 + 1) + (n_3 + N_3);
  * contacts: pairs i <= j; every image for i < j, the images after (0, 0, 0) in that order for i == j;
    disp = (p_j + s) - p_i, d2 = (dx dx + dy dy) + dz dz;
  * the reported contact is the smallest by (bits of d2, i, j, m); min_distance = sqrt(d2); n_close counts d2 <
    float32(double(min_distance)^2); BEYOND when not (d2_min <= float32(double(search_radius)^2)).
Every operation above is one float32 operation, rounded to nearest, no fused multiply-add.

Error bound of the float32 distance (DISTANCE_BOUND_FACTOR).  u = 2^-24 is the unit roundoff.  Write A = max_d sum_k |L_kd|
(positions: |w_k| < 1) and S = max_d sum_k n_k |L_kd| (shifts), G = A + S.
  * w: the subtraction f - floor(f) is exact except for a negative f above -1 (one rounding of a value below 1): |dw| <= u;
  * p_d: three products and two sums of terms bounded by A, plus dw carried through L: |dp_d| <= (3 + 1) u A = 4 u A;
  * s_d: the same three products and two sums on integers: |ds_d| <= 3 u S;
  * disp_d = (p_j + s) - p_i: the inputs' errors 4 u A + 3 u S + 4 u A, the sum's rounding u (A + S), the difference's rounding
    u (2 A + S): |d disp_d| <= u (11 A + 5 S) <= 11 u G;
  * the distance: the error vector has norm at most sqrt(3) 11 u G <= 19.1 u G; d2's three products and two sums and the square
    root add a relative (3 u) / 2 + u / 2 = 2 u on d, and d <= sqrt(3) (2 A + S) <= 3.5 G: at most 7 u G.
Together |d_f32 - d_exact| <= 26.1 u G; the float64 restatement's own error is 2^-29 of that.  DISTANCE_BOUND_FACTOR = 32
leaves the margin for the second-order terms: bound = 32 * 2^-24 * G, about 1e-4 A for a 10 A cell with one shell.  Two
coincident atoms give exactly 0 in both (equal bits in, equal p out)."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import crystal_batch as cb

NONFINITE, CELL, CLOSE, MASKED, BEYOND = 1, 2, 4, 8, 16
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (CLOSE, "CLOSE"), (MASKED, "MASKED"), (BEYOND, "BEYOND"))
INVALID_MASK = NONFINITE | CELL | CLOSE | MASKED  # BEYOND is informational
MAX_SHELLS = 8
STAGED_ATOMS = cb.STAGED_ATOMS
METRIC_KEYS = ("min_distance", "pair", "n_close", "volume", "number_density", "flags")  # arreau_screen_result, in its order
STORED_KEYS = METRIC_KEYS + ("valid",)  # what SampleResult.metrics and a crystals file hold
DISTANCE_BOUND_FACTOR = 32.0
F32 = np.float32


def describe(flags) -> str:
    """'CLOSE|MASKED' for 12, 'valid' for 0 or BEYOND alone ('valid (BEYOND)')."""
    flags = int(flags)
    names = [name for bit, name in FLAG_NAMES if flags & bit]
    if flags & INVALID_MASK:
        return "|".join(names)
    return "valid (BEYOND)" if flags & BEYOND else "valid"


def is_valid(flags):
    return (np.asarray(flags) & INVALID_MASK) == 0


@dataclass(frozen=True)
class ScreenCriteria:
    """Thresholds of the screen.  min_distance / search_radius in A, min_volume in A^3; mask_type is the class index of the
    D3PM mask state (-1: no species check; None: the caller's default -- the sampler's last class, none elsewhere);
    max_shells caps the periodic images per axis (1..8): a cell that needs more to cover search_radius is flagged CELL."""
    min_distance: float = 0.5
    min_volume: float = 0.1
    search_radius: float = 3.0
    mask_type: Optional[int] = None
    max_shells: int = MAX_SHELLS

    def __post_init__(self):
        for name in ("min_distance", "min_volume", "search_radius"):
            v = getattr(self, name)
            if not isinstance(v, Real) or isinstance(v, bool):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
            object.__setattr__(self, name, float(v))
        if not self.search_radius > 0.0:
            raise ValueError(f"search_radius must be > 0, got {self.search_radius}")
        if self.search_radius < self.min_distance:
            raise ValueError(f"search_radius ({self.search_radius}) must be at least min_distance ({self.min_distance})")
        if self.mask_type is not None:
            if not isinstance(self.mask_type, Integral) or isinstance(self.mask_type, bool) or int(self.mask_type) < -1:
                raise ValueError(f"mask_type must be None, -1 or a class index, got {self.mask_type!r}")
            object.__setattr__(self, "mask_type", int(self.mask_type))
        if not isinstance(self.max_shells, Integral) or isinstance(self.max_shells, bool) or not 1 <= int(self.max_shells) <= MAX_SHELLS:
            raise ValueError(f"max_shells must lie in 1..{MAX_SHELLS}, got {self.max_shells!r}")
        object.__setattr__(self, "max_shells", int(self.max_shells))

    def with_mask_type(self, default):
        """These criteria with mask_type resolved: its own value, or `default` when it is None."""
        if self.mask_type is not None:
            return self
        return ScreenCriteria(self.min_distance, self.min_volume, self.search_radius, int(default), self.max_shells)


def resolve(screen):
    """sample(screen=...): None / False -> None, True -> the defaults, a ScreenCriteria -> itself."""
    return cb.resolve(screen, ScreenCriteria, "screen")


def screen(frac, lattice, offsets, types=None, criteria=None):
    """Screen a batch on the GPU without an engine (arreau_crystal_screen, one launch).  frac [N,3] float32, lattice [B,3,3]
    float32 (rows a, b, c), offsets [B+1] int32 and types [N] int32 (optional) are contiguous tensors on one cuda device.
    Returns a dict of device tensors: min_distance [B], pair [B,5] (i, j, n1, n2, n3; i, j local to the crystal), n_close
    [B], volume [B], number_density [B], flags [B], valid [B] bool.  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    crit = (criteria if criteria is not None else ScreenCriteria()).with_mask_type(-1)
    dev, B, N = cb.check_batch("screen", frac, lattice, offsets, types, types_optional=True)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"min_distance": torch.empty(B, **f32), "pair": torch.empty((B, 5), **i32), "n_close": torch.empty(B, **i32),
           "volume": torch.empty(B, **f32), "number_density": torch.empty(B, **f32), "flags": torch.empty(B, **i32)}
    c = _hip.ScreenCriteriaC(crit.min_distance, crit.min_volume, crit.search_radius, crit.mask_type, crit.max_shells)
    r = _hip.ScreenResultC(*[_hip.ptr(out[k]).value if B else None for k in METRIC_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_screen(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(offsets), B, N,
                                                    ctypes.byref(c), ctypes.byref(r), _hip.stream_ptr(dev)), "arreau_crystal_screen")
    out["valid"] = (out["flags"] & INVALID_MASK) == 0
    return out


def metrics_to_numpy(metrics):
    """The dict of `screen` as host numpy arrays (synchronises)."""
    return {k: v.cpu().numpy() for k, v in metrics.items()}


def screen_sample_result(result, criteria=None, device="cuda"):
    """Screen a SampleResult (or a loaded crystals file: generated crystals or a training set) on the GPU: its float64 arrays
    are cast to float32.  A file holds atomic numbers, not class indices; the mask state is atomic number 2001 in every table
    (AtomicNumberTable.MASK_ATOMIC_NUMBER), so unless the criteria name a mask_type of their own (-1: none) the species check
    looks for that number.  Returns the metrics as numpy arrays."""
    import torch

    from .tools.atomic_number_table import AtomicNumberTable
    crit = criteria if criteria is not None else ScreenCriteria()
    frac, lattice, off, types = cb.upload(result, device)
    if crit.mask_type is None:  # 1 where the atom is the mask state, looked for as class 1
        types = (types == AtomicNumberTable.MASK_ATOMIC_NUMBER).to(torch.int32)
        crit = crit.with_mask_type(1)
    out = screen(frac, lattice, off, types, crit)
    return metrics_to_numpy(out)


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(flags, rank=0, requested=None, rounds=None):
    """What a summary line needs: attempted, accepted and the count per flag, of one rank's attempts."""
    flags = np.asarray(flags, dtype=np.int64).reshape(-1)
    out = {"rank": int(rank), "attempted": int(flags.size), "accepted": int(is_valid(flags).sum()),
           "flags": cb.flag_counts(flags, FLAG_NAMES)}
    if requested is not None:
        out["requested"] = int(requested)
    if rounds is not None:
        out["rounds"] = int(rounds)
    return out


def total_stats(parts):
    out = {"rank": "total", "attempted": sum(p["attempted"] for p in parts), "accepted": sum(p["accepted"] for p in parts),
           "flags": {name: sum(p["flags"][name] for p in parts) for _, name in FLAG_NAMES}}
    if all("requested" in p for p in parts) and parts:
        out["requested"] = sum(p["requested"] for p in parts)
    return out


def format_stats(st) -> str:
    line = f"screen {cb.who(st)}: accepted {st['accepted']} / attempted {st['attempted']}; " + \
        ", ".join(f"{name} {st['flags'][name]}" for _, name in FLAG_NAMES)
    if "requested" in st:
        line += f"; requested {st['requested']}"
        if st["accepted"] < st["requested"]:
            line += f" (short by {st['requested'] - st['accepted']})"
    if "rounds" in st:
        line += f"; rounds {st['rounds']}"
    return line


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------- the numpy restatements
def _cutoff2(x):
    """float32(double(x)^2) of the float32 threshold the C entry point receives."""
    return F32(np.float64(F32(x)) ** 2)


def _empty_result(B):
    return SimpleNamespace(min_distance=np.full(B, np.nan, F32), pair=np.full((B, 5), -1, np.int32), n_close=np.zeros(B, np.int32),
                           volume=np.full(B, np.nan, F32), number_density=np.full(B, np.nan, F32), flags=np.zeros(B, np.int32))


def _finish(out):
    out.valid = is_valid(out.flags)
    return out


def screen_reference_f32(frac, lattice, counts, types=None, criteria=None):
    """The kernel's rule in numpy float32, one operation at a time in the kernel's order (numpy never contracts to an FMA):
    frac [N,3], lattice [B,3,3], counts [B] atoms per crystal, types [N] or None.  Returns a namespace of the six outputs
    (+ valid), to be compared with the kernel's bit for bit."""
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    crit = (criteria if criteria is not None else ScreenCriteria()).with_mask_type(-1)
    out = _empty_result(len(counts))
    md2, r2 = _cutoff2(crit.min_distance), _cutoff2(crit.search_radius)
    for b, n in enumerate(counts):
        L, f = lattice[b], frac[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        vol, q, bad = cb.cell_f32(L, crit.search_radius, crit.min_volume, crit.max_shells)
        out.volume[b] = vol
        with np.errstate(all="ignore"):
            out.number_density[b] = F32(n) / vol
        if types is not None and crit.mask_type >= 0 and (types[first[b]:first[b + 1]] == crit.mask_type).any():
            out.flags[b] |= MASKED
        if bad:
            out.flags[b] |= CELL
            continue
        nk = [max(1, int(np.ceil(qk))) for qk in q]
        p, g, centre, s = cb.positions_and_shifts(f, L, nk, F32)
        best, close = None, 0
        for i, j, m, d2 in cb.contacts(p, s, centre, F32):
            close += int((d2 < md2).sum())
            if d2.size:
                e = int(np.argmin(d2))  # the first of equal minima: the enumeration order is (i, j, m)
                if best is None or d2[e] < best[0]:
                    best = (d2[e], int(i[e]), int(j[e]), int(m[e]))
        out.n_close[b] = close
        if close:
            out.flags[b] |= CLOSE
        if best is None:
            out.min_distance[b] = np.inf
            out.flags[b] |= BEYOND
            continue
        out.min_distance[b] = np.sqrt(best[0])
        out.pair[b] = (best[1], best[2]) + tuple(int(v) for v in g[best[3]])
        if not best[0] <= r2:
            out.flags[b] |= BEYOND
    return _finish(out)


def distance_bound(lattice, shells):
    """The derived bound on |d_float32 - d_exact| of one crystal (module docstring): 32 * 2^-24 * G, G = max_d sum_k
    (1 + n_k) |L_kd|."""
    L = np.abs(np.asarray(lattice, dtype=np.float64).reshape(3, 3))
    nk = np.asarray(shells, dtype=np.float64).reshape(3, 1)
    return DISTANCE_BOUND_FACTOR * 2.0 ** -24 * float(((1.0 + nk) * L).sum(axis=0).max())


def screen_reference_f64(frac, lattice, counts, types=None, criteria=None, widen=1, details=False):
    """The same rules in float64 from the same float32 inputs, without the operation-order detail; the image range is n_k +
    `widen` per axis (one shell wider than the kernel's by default: a range that missed a contact within search_radius would
    show).  Outputs are float64 / integers.  details=True adds `shells` [B,3] (n_k without the widening), `bound` [B]
    (distance_bound), `q` [B,3] (search_radius / h_k), `nearest` (per crystal, the up to 8 smallest contact distances) and
    `near_threshold` [B] (contacts whose distance lies within 2 bound of min_distance: n_close may differ in float32)."""
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    crit = (criteria if criteria is not None else ScreenCriteria()).with_mask_type(-1)
    B = len(counts)
    out = _empty_result(B)
    out.min_distance, out.volume, out.number_density = (np.full(B, np.nan) for _ in range(3))
    out.shells, out.bound, out.q, out.nearest = np.zeros((B, 3), np.int64), np.full(B, np.nan), np.full((B, 3), np.nan), [None] * B
    out.near_threshold = np.zeros(B, np.int64)
    md, R = float(F32(crit.min_distance)), float(F32(crit.search_radius))
    for b, n in enumerate(counts):
        L, f = lattice[b].astype(np.float64), frac[first[b]:first[b + 1]].astype(np.float64)
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        vol, q = cb.cell_f64(L, R)
        out.volume[b] = vol
        with np.errstate(all="ignore"):
            out.number_density[b] = n / vol if vol > 0 else np.inf
        out.q[b] = q
        if types is not None and crit.mask_type >= 0 and (types[first[b]:first[b + 1]] == crit.mask_type).any():
            out.flags[b] |= MASKED
        if not vol >= float(F32(crit.min_volume)) or not np.isfinite(vol) or not (q <= crit.max_shells).all():
            out.flags[b] |= CELL
            continue
        nk = np.maximum(1, np.ceil(q).astype(np.int64))
        out.shells[b], out.bound[b] = nk, distance_bound(L, nk)
        p, g, centre, s = cb.positions_and_shifts(f, L, nk + int(widen), np.float64)
        best, close, nearest = None, 0, np.empty(0)
        for i, j, m, d2 in cb.contacts(p, s, centre, np.float64):
            close += int((d2 < md * md).sum())
            out.near_threshold[b] += int((np.abs(np.sqrt(d2) - md) <= 2 * out.bound[b]).sum())
            if d2.size:
                nearest = np.sort(np.concatenate([nearest, np.sqrt(np.partition(d2, min(8, d2.size) - 1)[:8])]))[:8]
                e = int(np.argmin(d2))
                if best is None or d2[e] < best[0]:
                    best = (d2[e], int(i[e]), int(j[e]), int(m[e]))
        out.n_close[b], out.nearest[b] = close, nearest
        if close:
            out.flags[b] |= CLOSE
        if best is None:
            out.min_distance[b] = np.inf
            out.flags[b] |= BEYOND
            continue
        out.min_distance[b] = math.sqrt(best[0])
        out.pair[b] = (best[1], best[2]) + tuple(int(v) for v in g[best[3]])
        if not out.min_distance[b] <= R:
            out.flags[b] |= BEYOND
    if not details:
        del out.shells, out.bound, out.q, out.nearest, out.near_threshold
    return _finish(out)
