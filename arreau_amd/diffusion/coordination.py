"""Coordination environments of generated crystals: per atom its nearest distance, its neighbours and their number, per crystal
the sums and extremes (arreau_crystal_coordination, arreau_amd/csrc/coordination.hip; the rules are written out in
include/arreau_hip.h).  Here: the parameters and their validation, the flag constants, the entry point that needs no engine
(`coordination`), the statistics, `bond_segments` (the Cartesian end points of the stored bonds: what the reference's
predict_bonds returns) and two numpy restatements of the kernel for the tests -- `coordination_reference_f32`, one float32
operation at a time in the kernel's order (the bit-for-bit yardstick), and `coordination_reference_f64`, the same rules in
float64, which also returns per atom the smallest relative margin of every comparison that decides a result.  Needs numpy alone
at import.

The rule is the table-free one pymatgen ships as MinimumDistanceNN: the neighbours of atom i are all atoms and images within
(1 + tol) times i's own nearest distance, and within a cutoff.  Per crystal with cell rows L, wrapped positions p (screening.py's
rules) and image shifts s_m, m in lexicographic order over |n_k'| <= n_k = max(1, ceil(cutoff / h_k)):
  * d2(i; j, m) = |(p_j + s_m) - p_i|^2, (dx dx + dy dy) + dz dz, for every j and m but (j = i, m = (0, 0, 0));
  * d2min(i) = the minimum of the bits of d2; thr2(i) = f2 * d2min(i), f2 = float32((1 + double(tol))^2); r2 =
    float32(double(cutoff)^2);
  * (j, m) is a neighbour of i iff d2 <= thr2(i) and d2 <= r2; cn(i) their number; the first max_neighbors in ascending (j, m)
    are stored as (j, n_1, n_2, n_3); nearest = sqrt(d2min), farthest = sqrt(max neighbour d2) (0 at cn = 0);
  * mutual(i) = the neighbours with d2 <= thr2(j): the bonds both ends agree on;
  * per crystal n_bonds = sum cn, n_mutual = sum mutual, min_cn, max_cn, mean_cn = float32(n_bonds) / float32(n).
Every operation above is one float32 operation, rounded to nearest, no fused multiply-add.

Relative error bound of the float32 d2 (D2_BOUND_FACTOR).  screening.py derives |d_f32 - d_exact| <= 26.1 u G for the same
arithmetic (u = 2^-24, G = max_d sum_k (1 + n_k) |L_kd|), the square root's half ulp included.  d2 = d^2, so |d2_f32 - d2_exact|
<= (d_f32 + d_exact) 26.1 u G, and relative to d2: at most 2 * 26.1 u G / d <= 52.2 u G / d_min for every d >= d_min, the
crystal's shortest nearest distance (every d2 that enters a comparison is at least its receiver's d2min).  D2_BOUND_FACTOR = 64
leaves the margin of screening.py's 32: rel_bound = 64 * 2^-24 * G / d_min.  A comparison d2 <= thr2 has an error on both sides:
thr2's is d2min's plus the two roundings of f2 and of the product (2 u, far inside the margin); r2 is exact but for its own
rounding (u).  So a crystal whose smallest margin exceeds FOUR rel_bound (two sides, and a factor two to spare) decides every
comparison in float32 as in float64: its integers are equal.  At tol = 0 the nearest contact sits on its own threshold and no
crystal is guarded; two coincident atoms give d_min = 0 and no bound."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from . import screening

NONFINITE, CELL, EMPTY, OVERLAP, ISOLATED, OVERFLOW = 1, 2, 4, 8, 16, 32
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (OVERLAP, "OVERLAP"), (ISOLATED, "ISOLATED"), (OVERFLOW, "OVERFLOW"))
FLAGS = FLAG_NAMES
MAX_NEIGHBORS = 64
MAX_SHELLS = screening.MAX_SHELLS
COORD_KEYS = ("n_bonds", "n_mutual", "min_cn", "max_cn", "mean_cn", "flags")  # one row per crystal
RESULT_KEYS = COORD_KEYS + ("cn", "neighbors", "nearest", "farthest", "mutual", "nearest_d2")  # arreau_coordination_result, in its order
ATOM_KEYS = ("cn", "neighbors", "nearest", "farthest", "mutual", "species")  # one row per atom; species: the atoms' atomic numbers
STORED_KEYS = COORD_KEYS + ATOM_KEYS  # what SampleResult.coordination and a crystals file hold
D2_BOUND_FACTOR = 64.0
F32 = np.float32


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class CoordinationParams:
    """tol: a neighbour lies within (1 + tol) times the atom's nearest distance (0.1: a starting value, not a claim); cutoff in A:
    nothing beyond it is a neighbour, and the image search covers it; max_neighbors: the neighbours stored per atom (1..64; cn
    counts them all); max_shells caps the periodic images per axis (1..8): a cell that needs more is flagged CELL."""
    tol: float = 0.1
    cutoff: float = 6.0
    max_neighbors: int = 24
    max_shells: int = MAX_SHELLS

    def __post_init__(self):
        for name in ("tol", "cutoff"):
            v = getattr(self, name)
            if not isinstance(v, Real) or isinstance(v, bool):
                raise ValueError(f"{name} must be a number, got {v!r}")
            with np.errstate(over="ignore"):
                if not (math.isfinite(v) and np.isfinite(F32(v)) and v >= 0.0):
                    raise ValueError(f"{name} must be finite (in float32) and >= 0, got {v}")
            object.__setattr__(self, name, float(v))
        if not float(F32(self.cutoff)) > 0.0:
            raise ValueError(f"cutoff must be > 0, got {self.cutoff}")
        for name, top in (("max_neighbors", MAX_NEIGHBORS), ("max_shells", MAX_SHELLS)):
            v = getattr(self, name)
            if not isinstance(v, Integral) or isinstance(v, bool) or not 1 <= int(v) <= top:
                raise ValueError(f"{name} must lie in 1..{top}, got {v!r}")
            object.__setattr__(self, name, int(v))


def resolve(coordination):
    """sample(coordination=...): None / False -> None, True -> the defaults, a CoordinationParams -> itself."""
    return cb.resolve(coordination, CoordinationParams, "coordination")


# ------------------------------------------------------------------------------------------------------- the device call
def coordination(frac, lattice, offsets, params=None):
    """The coordination environments of a batch on the GPU without an engine (arreau_crystal_coordination, one launch).  frac
    [N,3] float32, lattice [B,3,3] float32 (rows a, b, c) and offsets [B+1] int32 are contiguous tensors on one cuda device.
    Returns a dict of device tensors (RESULT_KEYS): n_bonds, n_mutual, min_cn, max_cn, mean_cn, flags [B]; cn, nearest, farthest,
    mutual, nearest_d2 [N]; neighbors [N, max_neighbors, 4] (j local to the crystal, n_1, n_2, n_3; -1 beyond cn).  Does not
    synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else CoordinationParams()
    dev, B, N = cb.check_batch("coordination", frac, lattice, offsets, None, types_optional=True)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {k: torch.empty(B, **(f32 if k == "mean_cn" else i32)) for k in COORD_KEYS}
    out.update({"cn": torch.empty(N, **i32), "neighbors": torch.empty((N, p.max_neighbors, 4), **i32), "nearest": torch.empty(N, **f32),
                "farthest": torch.empty(N, **f32), "mutual": torch.empty(N, **i32), "nearest_d2": torch.empty(N, **f32)})
    c = _hip.CoordinationParamsC(p.tol, p.cutoff, p.max_neighbors, p.max_shells)
    r = _hip.CoordinationResultC(*[_hip.ptr(out[k]).value if out[k].numel() else None for k in RESULT_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_coordination(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(offsets), B, N, ctypes.byref(c),
                                                          ctypes.byref(r), _hip.stream_ptr(dev)), "arreau_crystal_coordination")
    return out


def result_to_numpy(result):
    """The dict of `coordination` as host numpy arrays (synchronises)."""
    return cb.to_numpy(result)


def sample_arrays(result, atomic_numbers):
    """What SampleResult.coordination and a crystals file hold (STORED_KEYS) of a `result_to_numpy` dict: its arrays but
    nearest_d2, and `species`, the atomic numbers of the atoms (what the mean per element is taken over)."""
    out = {k: np.asarray(result[k]) for k in STORED_KEYS if k != "species"}
    out["species"] = np.rint(np.asarray(atomic_numbers, dtype=np.float64).reshape(-1)).astype(np.int64)
    if out["species"].shape != out["cn"].shape:
        raise ValueError("coordination: one atomic number per atom is needed")
    return out


def coordination_sample_result(result, params=None, device="cuda"):
    """The coordination environments of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32:
    the dict of `sample_arrays`."""
    frac, lattice, off, _ = cb.upload(result, device)
    return sample_arrays(result_to_numpy(coordination(frac, lattice, off, params)), result.atomic_numbers)


def bond_segments(result, crystals, b):
    """The Cartesian end points [K, 2, 3] (float64) of crystal b's stored bonds: from atom i's wrapped position to the wrapped
    position of its neighbour j shifted by the image (n_1, n_2, n_3), atoms in order, each atom's neighbours in stored order.
    `result` holds cn and neighbors (numpy), `crystals` frac_x, lattice and num_atoms (a SampleResult or a loaded file)."""
    num_atoms = np.asarray(crystals.num_atoms, dtype=np.int64)
    first = int(num_atoms[:b].sum())
    n = int(num_atoms[b])
    L = np.asarray(crystals.lattice, dtype=np.float64).reshape(-1, 3, 3)[b]
    f = np.asarray(crystals.frac_x, dtype=np.float32).reshape(-1, 3)[first:first + n]  # (the kernel saw the float32 coordinates)
    w = (f - np.floor(f)).astype(np.float32)
    w[w >= 1] = 0
    w = w.astype(np.float64)
    nb = np.asarray(result["neighbors"])[first:first + n]
    out = []
    for i in range(n):
        for j, n1, n2, n3 in nb[i]:
            if j >= 0:
                out.append((w[i] @ L, (w[j] + np.array([n1, n2, n3], dtype=np.float64)) @ L))
    return np.asarray(out, dtype=np.float64).reshape(-1, 2, 3)


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the histogram of cn over the atoms of the crystals
    that were searched, per element the atoms and their summed cn (`species` given), the bonds and the mutual ones, the count per
    flag."""
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    cn = np.asarray(result["cn"], dtype=np.int64).reshape(-1)
    done = np.asarray(result["nearest"], dtype=np.float64).reshape(-1)
    done = ~np.isnan(done)  # (NONFINITE / CELL crystals: nothing was computed for their atoms)
    out = {"rank": cb.rank_of(rank), "crystals": int(flags.size), "atoms": int(done.sum()),
           "cn": {int(v): int((cn[done] == v).sum()) for v in np.unique(cn[done])},
           "n_bonds": int(np.asarray(result["n_bonds"], dtype=np.int64).sum()), "n_mutual": int(np.asarray(result["n_mutual"], dtype=np.int64).sum()),
           "elements": {}, "flags": cb.flag_counts(flags, FLAG_NAMES)}
    if result.get("species") is not None:
        z = np.asarray(result["species"], dtype=np.int64).reshape(-1)
        out["elements"] = {int(v): [int(((z == v) & done).sum()), int(cn[(z == v) & done].sum())] for v in np.unique(z[done])}
    return out


def total_stats(parts):
    hist, elements = {}, {}
    for p in parts:
        for k, v in p["cn"].items():
            hist[int(k)] = hist.get(int(k), 0) + v
        for k, (a, s) in p["elements"].items():
            have = elements.get(int(k), [0, 0])
            elements[int(k)] = [have[0] + a, have[1] + s]
    return {"rank": "total", "crystals": sum(p["crystals"] for p in parts), "atoms": sum(p["atoms"] for p in parts),
            "cn": dict(sorted(hist.items())), "n_bonds": sum(p["n_bonds"] for p in parts), "n_mutual": sum(p["n_mutual"] for p in parts),
            "elements": dict(sorted(elements.items())), "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'coordination rank 0: 16 crystals, 320 atoms; cn 4: 12, 6: 308; mean cn 5.92 (Z 11: 6.00, Z 17: 5.85); mutual 1800 / 1896
    bonds (94.9 %); flags ISOLATED 1'."""
    hist = cb.some(dict(sorted((int(k), v) for k, v in st["cn"].items())), ": ")
    mean = f"{st['n_bonds'] / st['atoms']:.2f}" if st["atoms"] else "n/a"
    per = ", ".join(f"Z {int(k)}: {s / a:.2f}" for k, (a, s) in sorted((int(k), v) for k, v in st["elements"].items()) if a)
    share = f" ({100.0 * st['n_mutual'] / st['n_bonds']:.1f} %)" if st["n_bonds"] else ""
    return f"coordination {cb.who(st)}: {st['crystals']} crystals, {st['atoms']} atoms; cn {hist}; mean cn {mean}" + \
        (f" ({per})" if per else "") + f"; mutual {st['n_mutual']} / {st['n_bonds']} bonds{share}; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------- the numpy restatements
def thresholds_f32(params):
    """(f2, r2) as the C entry point forms them from the float32 tol and cutoff it receives: (1 + tol)^2 and cutoff^2 in double,
    each rounded once to float32."""
    return F32((1.0 + np.float64(F32(params.tol))) ** 2), F32(np.float64(F32(params.cutoff)) ** 2)


def _empty_result(B, N, max_nb, real):
    return SimpleNamespace(n_bonds=np.zeros(B, np.int32), n_mutual=np.zeros(B, np.int32), min_cn=np.full(B, -1, np.int32),
                           max_cn=np.full(B, -1, np.int32), mean_cn=np.full(B, np.nan, real), flags=np.zeros(B, np.int32),
                           cn=np.zeros(N, np.int32), neighbors=np.full((N, max_nb, 4), -1, np.int32), nearest=np.full(N, np.nan, real),
                           farthest=np.full(N, np.nan, real), mutual=np.zeros(N, np.int32), nearest_d2=np.full(N, np.nan, real))


def _d2_table(p, s, dtype):
    """d2 [n, n M] of one crystal, column e = j M + m: disp = (p_j + s_m) - p_i, d2 = (dx dx + dy dy) + dz dz, every operation
    rounded to `dtype`."""
    n, M = p.shape[0], s.shape[0]
    ps = (p[:, None, :] + s[None, :, :]).astype(dtype)
    disp = (ps[None, :, :, :] - p[:, None, None, :]).astype(dtype)
    sq = (disp * disp).astype(dtype)
    return ((sq[..., 0] + sq[..., 1]).astype(dtype) + sq[..., 2]).astype(dtype).reshape(n, n * M)


def _crystal(out, a0, n, d2, g, centre, f2, r2, max_nb, real, margins=None):
    """The rules from d2 [n, n M] on: fills rows a0 .. a0 + n of the per-atom arrays and returns (n_bonds, n_mutual, min_cn,
    max_cn, flags).  `margins` [n] (float64 restatement) receives the smallest relative margin of the deciding comparisons."""
    M = g.shape[0]
    own = np.arange(n) * M + centre
    masked = d2.copy()
    masked[np.arange(n), own] = np.inf
    if real == F32:  # the minimum of the bits: +inf where no finite d2 (NaN bits lie above inf's and are never chosen)
        d2min = np.minimum(masked.view(np.uint32).min(axis=1), np.uint32(0x7f800000)).view(F32)
    else:
        d2min = masked.min(axis=1)
    with np.errstate(all="ignore"):
        thr2 = (real(f2) * d2min).astype(real)
        in_thr, in_r = d2 <= thr2[:, None], d2 <= real(r2)
        in_thr[np.arange(n), own] = False  # the atom itself
        hit = in_thr & in_r
        j_of = np.repeat(np.arange(n), M)
        agreed = hit & (d2 <= thr2[j_of][None, :])
        out.nearest_d2[a0:a0 + n], out.nearest[a0:a0 + n] = d2min, np.sqrt(d2min)
    flags = 0
    for i in range(n):
        e = np.flatnonzero(hit[i])
        out.cn[a0 + i], out.mutual[a0 + i] = e.size, int(agreed[i].sum())
        out.farthest[a0 + i] = np.sqrt(d2[i, e].max()) if e.size else 0
        k = min(e.size, max_nb)
        out.neighbors[a0 + i, :k, 0] = e[:k] // M
        out.neighbors[a0 + i, :k, 1:] = g[e[:k] % M]
        flags |= (OVERLAP if d2min[i] == 0 else 0) | (ISOLATED if e.size == 0 else 0) | (OVERFLOW if e.size > max_nb else 0)
    if margins is not None:
        with np.errstate(all="ignore"):
            rel = lambda a, b: np.nan_to_num(np.abs(a - b) / np.maximum(a, b), nan=0.0)  # (0 against 0: no margin)
            m_thr, m_r, m_j = rel(d2, thr2[:, None]), rel(d2, np.float64(r2)), rel(d2, thr2[j_of][None, :])
            # a neighbour: every comparison it passed (the mutual one either way); otherwise the ones it failed (one suffices)
            miss = np.maximum(np.where(in_thr, 0.0, m_thr), np.where(in_r, 0.0, m_r))
            m = np.where(hit, np.minimum(np.minimum(m_thr, m_r), m_j), miss)
            m[np.arange(n), own] = np.inf
            margins[:] = m.min(axis=1)
    cn = out.cn[a0:a0 + n]
    return int(cn.sum()), int(out.mutual[a0:a0 + n].sum()), int(cn.min()), int(cn.max()), flags


def coordination_reference_f32(frac, lattice, counts, params=None):
    """The kernel's rule in numpy float32, one operation at a time in the kernel's order (numpy never contracts to an FMA): frac
    [N,3], lattice [B,3,3], counts [B] atoms per crystal.  Returns a namespace of the twelve outputs (RESULT_KEYS), to be compared
    with the kernel's bit for bit."""
    frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    p_ = params if params is not None else CoordinationParams()
    out = _empty_result(len(counts), frac.shape[0], p_.max_neighbors, F32)
    f2, r2 = thresholds_f32(p_)
    for b, n in enumerate(counts):
        L, f = lattice[b], frac[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        _, q, bad = cb.cell_f32(L, p_.cutoff, 0.0, p_.max_shells)
        if bad:
            out.flags[b] = CELL
            continue
        if n == 0:
            out.flags[b] = EMPTY
            continue
        nk = [max(1, int(np.ceil(qk))) for qk in q]
        p, g, centre, s = cb.positions_and_shifts(f, L, nk, F32)
        bonds, mutual, lo, hi, flags = _crystal(out, first[b], n, _d2_table(p, s, F32), g, centre, f2, r2, p_.max_neighbors, F32)
        out.n_bonds[b], out.n_mutual[b], out.min_cn[b], out.max_cn[b], out.flags[b] = bonds, mutual, lo, hi, flags
        out.mean_cn[b] = F32(bonds) / F32(n)
    return out


def d2_relative_bound(lattice, shells, d_min):
    """The derived bound on |d2_float32 - d2_exact| / d2 of one crystal (module docstring): 64 * 2^-24 * G / d_min, G = max_d sum_k
    (1 + n_k) |L_kd|; inf for d_min = 0."""
    G = screening.distance_bound(lattice, shells) / (screening.DISTANCE_BOUND_FACTOR * 2.0 ** -24)
    return D2_BOUND_FACTOR * 2.0 ** -24 * G / d_min if d_min > 0 else np.inf


def coordination_reference_f64(frac, lattice, counts, params=None, widen=0):
    """The same rules in float64 from the same float32 inputs and thresholds, without the operation-order detail; `widen` adds
    shells to the image range per axis (a range that missed a neighbour within the cutoff would show in cn; the stored (j, n_1,
    n_2, n_3) keep their order, which is lexicographic).  Returns the twelve outputs (reals float64) and `margin` [N] (per atom the
    smallest relative margin |a - b| / max(a, b) of the comparisons that decide its results: of a neighbour d2 against thr2(i),
    r2 and thr2(j), of any other contact the largest margin among the comparisons it fails), `shells` [B,3], `bound` [B]
    (screening.distance_bound: on nearest and farthest), `rel_bound` [B] (d2_relative_bound) and `guarded` [B]: the crystal was
    searched, and min margin > 4 rel_bound, so float32 decides every comparison alike."""
    frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    p_ = params if params is not None else CoordinationParams()
    B = len(counts)
    out = _empty_result(B, frac.shape[0], p_.max_neighbors, np.float64)
    out.margin, out.shells = np.full(frac.shape[0], np.nan), np.zeros((B, 3), np.int64)
    out.bound, out.rel_bound, out.guarded = np.full(B, np.nan), np.full(B, np.nan), np.zeros(B, bool)
    f2, r2 = (np.float64(v) for v in thresholds_f32(p_))
    R = float(F32(p_.cutoff))
    for b, n in enumerate(counts):
        L, f = lattice[b].astype(np.float64), frac[first[b]:first[b + 1]].astype(np.float64)
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        vol, q = cb.cell_f64(L, R)
        if not np.isfinite(vol) or not (q <= p_.max_shells).all():
            out.flags[b] = CELL
            continue
        if n == 0:
            out.flags[b] = EMPTY
            continue
        nk = np.maximum(1, np.ceil(q).astype(np.int64))
        out.shells[b], out.bound[b] = nk, screening.distance_bound(L, nk)
        p, g, centre, s = cb.positions_and_shifts(f, L, nk + int(widen), np.float64)
        bonds, mutual, lo, hi, flags = _crystal(out, first[b], n, _d2_table(p, s, np.float64), g, centre, f2, r2, p_.max_neighbors,
                                                np.float64, out.margin[first[b]:first[b + 1]])
        out.n_bonds[b], out.n_mutual[b], out.min_cn[b], out.max_cn[b], out.flags[b] = bonds, mutual, lo, hi, flags
        out.mean_cn[b] = bonds / n
        out.rel_bound[b] = d2_relative_bound(L, nk, float(out.nearest[first[b]:first[b + 1]].min()))
        out.guarded[b] = bool(out.margin[first[b]:first[b + 1]].min() > 4.0 * out.rel_bound[b])
    return out
