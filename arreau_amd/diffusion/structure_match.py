"""Structure match of generated crystals against target structures: for a pair (x, y) the change of basis W and the translation
under which y's atoms fall next to x's, the atom-to-atom map and the root-mean-square displacement in A and normalised as
pymatgen's StructureMatcher normalises it (arreau_structure_match, arreau_amd/csrc/match.hip; the rules are written out in
include/arreau_hip.h, "structure match").  Here: the parameters and their validation, the flag constants, the entry point that
needs no engine (`match`), the host pairing helpers (`paired`, `same_composition`, `best_per_x`), `match_crystals` for two
SampleResults or loaded files, the statistics lines and a float64 numpy restatement of rules 1-7 (`structure_match_reference_f64`).
The restatement and the helpers need numpy alone.

The assignment.  By default (`assignment="nearest"`) a candidate whose nearest-partner map is not one-to-one is skipped (where
the map is a permutation it is the optimal assignment).  With `assignment="optimal"` such a candidate gets the one-to-one,
species-preserving map of the smallest sum of squared distances at its unrefined translation (the header's rule 6b; the linear
assignment StructureMatcher solves), so no pair ends NO_PERMUTATION; the flag ASSIGNED says the winner's map came from that step.

What this is not.  No supercell, formula-reduced or anonymous-species matching: the species multisets are
compared exactly, run cell_reduction first.  No rescaling of the two cells to one volume.  A mapping W with an entry outside
{-1, 0, 1} is not found (complete for two Delaunay-reduced cells).  And nothing is said about a trained model.

float32 against float64 (rule 8).  Every arithmetic step of the kernel is one rounded float32 operation, never contracted; no
float32 restatement is kept.  The integer outputs are compared with the float64 restatement on GUARDED inputs: the length and
angle deviation of every lattice candidate and the best rms_norm at most half their tolerance or at least twice it, and for
every candidate and atom the nearest and the second-nearest partner a stated margin apart.  The reals are held to derived bounds.
u = 2^-24; n atoms; l_1 = (1 + ltol) x the longest edge of x's cell (an accepted image vector of y is no longer, and neither is
an edge of the mean metric G_m: every entry of G_m lies within l_1^2, its largest eigenvalue within 3 l_1^2); D = the largest
|component| of a difference e'_i of the best candidate (from the restatement: a property of the input); rho = l_1^6 / det G_m.
  * a wrapped coordinate carries u.  v' = wrap(V v), V integer with entries up to +-2 (exact products): 6 u from v, two roundings
    of sums below 8 (4 u each), the wrap u: 15 u.  t = wrap(w_p0 - v'_q): 16 u, its rounding u, the wrap u: 18 u.
  * e = (v'_j + t) - w_i: 33 u, the sum's rounding (below 2) u, w_i u, the difference's rounding u: 36 u; the nearest integer
    and the image shift are exact (|e| <= 1.5).  The sum of n such below n D: n D u; the division D u.  t' = t - mean: 18 u +
    36 u + (n + 1) D u + u: TRANSLATION_BOUND = (64 + (n + 1) D) u, compared modulo 1.  e' = (v'_p + t') - w_i: 15 u + that + 3 u:
    E_e = (88 + (n + 1) D) u per component (`difference_bound`).
  * G' = W^T G_y W through the image vectors: each entry within 25 u l_1^2 (diffusion/symmetrize.py's derivation); G_x has exact
    images; their sum's rounding 2 u l_1^2 halved: every entry of G_m within 26 u l_1^2 -- 32 u l_1^2 is used.
  * d^2 = e G_m e^T with |e_k| <= D_e = D + E_e: the nine terms below l_1^2 D_e^2 each; six roundings on every path: 54 u l_1^2
    D_e^2; G_m's error 9 x 32 u l_1^2 D_e^2.  The sum over the atoms in order and the division: (n + 1) u x 9 l_1^2 D_e^2.
    |mean d^2_f32 - mean d^2(e_f32)| <= E_2 = (351 + 9 n) u l_1^2 D_e^2 (`msd_bound`); a single d^2 likewise.
  * sqrt(mean d^2) is a norm of the differences: moving every component by E_e moves it by at most sqrt(3 l_1^2 x 3 E_e^2) = 3 l_1
    E_e =: lin.  |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)) with b >= (value - lin)^2.  The square root and the
    division round once more: 4 u value.  DISTANCE_BOUND(value) = lin + min(sqrt(E_2), E_2 / (value - lin)) + 4 u value, for rms
    and for max_dist (`distance_bound`).  The minimum over the 27 images moves no further than its arguments.
  * l = cbrt(sqrt(det G_m) / n): det's six triple products below l_1^6, each within (3 x 32 + 2) u l_1^6, five roundings of partial
    sums below 6 l_1^6: |det_f32 - det| <= (6 x 98 + 30) u l_1^6 = 618 u rho det; the square root and cube root divide that by 6
    and add u, the division u, the device's cbrt 4 u: l within (103 rho + 8) u l.  rms_norm = rms / l: DISTANCE_BOUND(rms) / l +
    rms_norm ((103 rho + 8) u + u) (`norm_bound`).
  * the assignment step (rule 6b).  A cost entry c = d^2 of e = (v'_j + t) - w_i at the unrefined t.  Given the float32 e, d^2
    carries the 54 + 288 = 342 u l_1^2 |e|^2 of the bullet above (no sum over atoms), and |e|^2 <= c / lambda, lambda the smallest
    eigenvalue of G_m: a c with a = 342 u l_1^2 / lambda.  e itself carries 36 u per component, which moves d by at most 3 l_1 x
    36 u = 108 u l_1 and d^2 by 2 d x that plus its square: b sqrt(c) + (108 u l_1)^2 with b = 216 u l_1.  The kernel rounds c to
    a multiple of 2^-24 A^2 (2^-25) and from there adds and compares 64-bit integers exactly: its solver returns a true optimum
    of the rounded matrix, whatever the order of its operations.  |c_f32 - c| <= a c + b sqrt(c) + c_0, c_0 = (108 u l_1)^2 +
    2^-25 (`cost_bound`).  Over a map of n rows with exact sum S: f(S) = a S + b sqrt(n S) + n c_0 (Cauchy-Schwarz).  If the
    kernel's map has the exact sum S* + x, S* the true optimum, then its rounded sum is no larger than the optimum's rounded
    sum: x <= f(S* + x) + f(S*) <= 2 f(S*) + a x + b sqrt(n x), so sqrt(x) <= (b sqrt(n) + sqrt(b^2 n + 8 (1 - a) f(S*))) /
    (2 (1 - a)): SOLVER_BOUND(S*) is the square of that (`solver_bound`), the most by which the kernel's map can miss the true
    optimum sum.  A test case is decided where the GAP to the runner-up assignment (the smallest optimum with one edge of the
    optimal map forbidden, minus the optimum) is at least four times SOLVER_BOUND and at least 1e-3 A^2; then the kernel's map
    is the restatement's.  For a given map the bounds on rms, max_dist, rms_norm and translation above hold as they stand."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from . import symmetry_search as ss

NONFINITE, CELL, EMPTY, DIFFERENT, BAD_PAIR, NO_MAPPING, OVERFLOW, NO_PERMUTATION = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (DIFFERENT, "DIFFERENT"), (BAD_PAIR, "BAD_PAIR"),
              (NO_MAPPING, "NO_MAPPING"), (OVERFLOW, "OVERFLOW"), (NO_PERMUTATION, "NO_PERMUTATION"))
ASSIGNED = 256  # informational (rule 6b): the winner's map came from the assignment step; not in NO_RESULT_MASK, nor in `matched`
# FLAG_NAMES: the flags of rules 1-7; ALL_FLAG_NAMES: those and ASSIGNED, what `describe` and the statistics count
ALL_FLAG_NAMES = FLAG_NAMES + ((ASSIGNED, "ASSIGNED"),)
ASSIGNMENTS = {"nearest": 0, "optimal": 1}  # arreau_hip.h: ARREAU_SM_ASSIGN_NEAREST / ARREAU_SM_ASSIGN_OPTIMAL
ASSIGN_LDS_ATOMS, ASSIGN_STATE_ROWS = 24, 6  # arreau_hip.h: ARREAU_SM_ASSIGN_LDS_ATOMS / ARREAU_SM_ASSIGN_STATE_ROWS
# `match` with assignment "optimal": the cost scratch of one launch stays below this many bytes (4 x (stride + 6) x stride floats
# per pair); a longer pair list is split into consecutive launches
COST_BUDGET_BYTES = 256 << 20
NO_RESULT_MASK = NONFINITE | CELL | EMPTY | DIFFERENT | BAD_PAIR | NO_MAPPING | NO_PERMUTATION  # rms = +inf, mapping = -1
MAX_MAPPINGS_CAP = 4096  # match.hip / arreau_hip.h: ARREAU_SM_MAX_MAPPINGS_CAP
DEFAULT_LTOL, DEFAULT_ANGLE_TOL, DEFAULT_STOL, DEFAULT_MAX_MAPPINGS = 0.2, 5.0, 0.3, 192
WAVES = 4  # crystal_dev.h: CRYSTAL_WAVES (the rows of scratch per pair)
PAIR_KEYS = ("rms", "rms_norm", "max_dist", "mapping", "translation", "partner", "n_mappings", "n_candidates", "n_permutations",
             "matched", "flags")  # arreau_structure_match_result's arrays, in its order (then scratch and partner_stride)
# what SampleResult.match and a crystals file hold: one row per crystal of x (partner: one row per atom of x)
MATCH_KEYS = ("target", "n_comparable", "rms", "rms_norm", "max_dist", "mapping", "translation", "partner", "n_mappings", "n_candidates",
              "n_permutations", "matched", "flags")
ATOM_KEYS = ("partner",)
U = 2.0 ** -24
F32 = np.float32


def describe(flags) -> str:
    return cb.describe(flags, ALL_FLAG_NAMES)


@dataclass(frozen=True)
class StructureMatchParams:
    """ltol: the relative tolerance on the cell lengths; angle_tol: on the cell angles, in DEGREES (the C struct takes radians);
    stol: on rms_norm = rms / (V / n)^(1/3) -- the three of pymatgen's StructureMatcher, with its defaults (starting values, not a
    claim).  max_mappings: the lattice mappings tried per pair (1..4096); n_mappings counts them all.  assignment: "nearest" -- a
    candidate whose nearest-partner map is not one-to-one is dropped; "optimal" -- it gets the optimal assignment (rule 6b)."""
    ltol: float = DEFAULT_LTOL
    angle_tol: float = DEFAULT_ANGLE_TOL
    stol: float = DEFAULT_STOL
    max_mappings: int = DEFAULT_MAX_MAPPINGS
    assignment: str = "nearest"

    def __post_init__(self):
        for name in ("ltol", "angle_tol", "stol"):
            v = getattr(self, name)
            if not isinstance(v, Real) or isinstance(v, bool) or not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
            object.__setattr__(self, name, float(v))
        v = self.max_mappings
        if not isinstance(v, Integral) or isinstance(v, bool) or not 1 <= int(v) <= MAX_MAPPINGS_CAP:
            raise ValueError(f"max_mappings must lie in 1..{MAX_MAPPINGS_CAP}, got {v!r}")
        object.__setattr__(self, "max_mappings", int(v))
        if not isinstance(self.assignment, str) or self.assignment not in ASSIGNMENTS:
            raise ValueError(f"assignment must be 'nearest' or 'optimal', got {self.assignment!r}")

    @property
    def angle_tol_rad(self) -> float:
        """What the kernel compares with: the float32 of the tolerance in radians."""
        return float(F32(math.radians(self.angle_tol)))


def resolve(match_to):
    """sample(match_to=...): None -> None; targets -> (targets, the defaults, None); (targets, StructureMatchParams) and (targets,
    StructureMatchParams, mode) -> themselves.  Targets are a SampleResult or a loaded crystals file (anything with frac_x,
    lattice, num_atoms and atomic_numbers); mode None pairs crystal b with target b when there are as many targets as crystals
    and takes the best target of a crystal's composition otherwise; "paired" / "any" say which."""
    if match_to is None or match_to is False:
        return None
    params, mode = StructureMatchParams(), None
    if isinstance(match_to, tuple):
        if len(match_to) not in (2, 3) or not isinstance(match_to[1], StructureMatchParams):
            raise ValueError("match_to as a tuple is (targets, StructureMatchParams) or (targets, StructureMatchParams, mode)")
        mode = match_to[2] if len(match_to) == 3 else None
        match_to, params = match_to[:2]
    if mode not in (None, "paired", "any"):
        raise ValueError(f"match mode must be None, 'paired' or 'any', got {mode!r}")
    for k in ("frac_x", "lattice", "num_atoms", "atomic_numbers"):
        if getattr(match_to, k, None) is None:
            raise ValueError(f"match_to: the targets hold no {k} (a SampleResult or a loaded crystals file is expected)")
    return match_to, params, mode


# ------------------------------------------------------------------------------------------------------- pairing (numpy)
def _counts_types(crystals):
    """(counts [B], types [N]) of a SampleResult / loaded file, or of a (counts, types) pair."""
    if isinstance(crystals, (tuple, list)):
        counts, types = crystals
    else:
        counts, types = crystals.num_atoms, np.rint(np.asarray(crystals.atomic_numbers).reshape(-1))
    return np.asarray(counts, dtype=np.int64).reshape(-1), np.asarray(types, dtype=np.int64).reshape(-1)


def paired(Bx):
    """The pair list [Bx, 2] int32 that matches crystal b against target b."""
    k = np.arange(int(Bx), dtype=np.int32)
    return np.ascontiguousarray(np.stack([k, k], axis=1))


def compositions(crystals):
    """The species multiset of every crystal as a sorted tuple of (species, count)."""
    counts, types = _counts_types(crystals)
    first = np.concatenate([[0], np.cumsum(counts)])
    out = []
    for b in range(len(counts)):
        ids, cnt = np.unique(types[first[b]:first[b + 1]], return_counts=True)
        out.append(tuple(zip(ids.tolist(), cnt.tolist())))
    return out


def same_composition(x, y):
    """The pair list [P, 2] int32 of every (x, y) with an equal, non-empty species multiset, x ascending, then y ascending."""
    by = {}
    for j, c in enumerate(compositions(y)):
        by.setdefault(c, []).append(j)
    rows = [(i, j) for i, c in enumerate(compositions(x)) if c for j in by.get(c, [])]
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))


def best_per_x(pairs, result, Bx):
    """A pair list's results (numpy dict of `result_to_numpy`) reduced to the best y of every x: `best` [Bx] (the y of the smallest
    rms_norm, the earliest pair on ties; -1 where no pair gave a finite one), `best_rms_norm` [Bx] (+inf there), `n_comparable` [Bx]
    (the pairs x appears in) and `row` [Bx] (the pair that gave the best, -1)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    norm = np.asarray(result["rms_norm"], dtype=np.float64).reshape(-1)
    best, row = np.full(Bx, -1, np.int32), np.full(Bx, -1, np.int64)
    best_norm, n_comparable = np.full(Bx, np.inf), np.zeros(Bx, np.int32)
    for k, (i, j) in enumerate(pairs):
        if not 0 <= i < Bx:
            continue
        n_comparable[i] += 1
        if np.isfinite(norm[k]) and norm[k] < best_norm[i]:
            best[i], row[i], best_norm[i] = j, k, norm[k]
    return {"best": best, "best_rms_norm": best_norm, "n_comparable": n_comparable, "row": row}


# ------------------------------------------------------------------------------------------------------- the device call
def match(x_batch, y_batch, pairs, params=None, stride=None, cost_budget=None):
    """Match pairs of crystals on the GPU without an engine (arreau_structure_match, one launch; with assignment "optimal"
    arreau_structure_match_assigned, whose cost scratch above ASSIGN_LDS_ATOMS atoms is kept below `cost_budget` bytes --
    COST_BUDGET_BYTES by default -- by consecutive launches over slices of the pair list: pairs are independent, the result is one
    launch's bit for bit).  x_batch, y_batch: (frac [N,3]
    float32, lattice [B,3,3] float32, offsets [B+1] int32, types [N] int32) contiguous tensors on one cuda device (crystal_batch's
    `upload` makes them; y_batch may be x_batch); pairs [P,2] int32 (x, y) indices, a tensor on that device or a host array.
    Returns a dict of device tensors: rms, rms_norm, max_dist, mapping, n_mappings, n_candidates, n_permutations, matched, flags
    [P], translation [P,3], partner [P, stride] (stride: the largest atom count of x_batch; -1 beyond a crystal's atoms) and
    `pairs`.  Without `stride` the largest atom count of x is read back (one small copy); the launch itself is not waited for."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else StructureMatchParams()
    dev, Bx, Nx = cb.check_batch("match (x)", *x_batch)
    dev_y, By, Ny = cb.check_batch("match (y)", *y_batch)
    if dev_y != dev:
        raise ValueError("match: the two batches must be on one device")
    if not hasattr(pairs, "data_ptr"):
        pairs = torch.as_tensor(np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2)), device=dev)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32 or pairs.device != dev or not pairs.is_contiguous():
        raise ValueError("match: pairs must be a contiguous int32 tensor of shape (P, 2) on the device of the batches")
    P = int(pairs.shape[0])
    if stride is None:
        stride = int(torch.diff(x_batch[2]).max().item()) if Bx else 0
    stride = max(int(stride), 1)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"rms": torch.empty(P, **f32), "rms_norm": torch.empty(P, **f32), "max_dist": torch.empty(P, **f32), "mapping": torch.empty(P, **i32),
           "translation": torch.empty((P, 3), **f32), "partner": torch.empty((P, stride), **i32), "n_mappings": torch.empty(P, **i32),
           "n_candidates": torch.empty(P, **i32), "n_permutations": torch.empty(P, **i32), "matched": torch.empty(P, **i32),
           "flags": torch.empty(P, **i32)}
    scratch = torch.empty((P, WAVES, stride), **i32) if stride > cb.STAGED_ATOMS else None
    c = _hip.StructureMatchParamsC(p.ltol, p.angle_tol_rad, p.stol, p.max_mappings)
    r = _hip.StructureMatchResultC(*[_hip.ptr(out[k]).value if P else None for k in PAIR_KEYS],
                                   _hip.ptr(scratch).value if scratch is not None and P else None, stride)
    side = lambda b, B, N: [_hip.ptr(b[0]) if N else None, _hip.ptr(b[3]) if N else None, _hip.ptr(b[1]) if B else None, _hip.ptr(b[2]), B, N]
    with torch.cuda.device(dev):
        if p.assignment == "nearest":
            _hip.check(_hip.lib().arreau_structure_match(*side(x_batch, Bx, Nx), *side(y_batch, By, Ny), _hip.ptr(pairs) if P else None, P,
                                                         ctypes.byref(c), ctypes.byref(r), _hip.stream_ptr(dev)), "arreau_structure_match")
        else:
            per_pair = WAVES * (stride + ASSIGN_STATE_ROWS) * stride * 4 if stride > ASSIGN_LDS_ATOMS else 0
            budget = COST_BUDGET_BYTES if cost_budget is None else int(cost_budget)
            chunk = max(1, min(P, budget // per_pair)) if per_pair else max(P, 1)
            cost = torch.empty(chunk * per_pair // 4, **f32) if per_pair and P else None  # (one buffer: the launches run in stream order)
            for a in range(0, max(P, 1), chunk):
                b = min(a + chunk, P)
                r = _hip.StructureMatchResultC(*[_hip.ptr(out[k][a:b]).value if P else None for k in PAIR_KEYS],
                                               _hip.ptr(scratch[a:b]).value if scratch is not None and P else None, stride)
                _hip.check(_hip.lib().arreau_structure_match_assigned(
                    *side(x_batch, Bx, Nx), *side(y_batch, By, Ny), _hip.ptr(pairs[a:b]) if P else None, b - a, ctypes.byref(c), ctypes.byref(r),
                    ASSIGNMENTS[p.assignment], _hip.ptr(cost), _hip.stream_ptr(dev)), "arreau_structure_match_assigned")
    out["pairs"] = pairs
    return out


def result_to_numpy(result):
    """The dict of `match` as host numpy arrays (synchronises)."""
    return cb.to_numpy(result)


def per_crystal(result, pairs, counts, mode):
    """The numpy dict of a pair list's results as MATCH_KEYS arrays, one row per crystal of x (partner: one row per atom of x):
    mode "paired" -- pair b is crystal b's; mode "any" -- the best pair of every crystal (`best_per_x`), and a crystal no target
    shares its composition with reports DIFFERENT, rms +inf, no target."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    Bx, pairs = len(counts), np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if mode == "paired":
        assert len(pairs) == Bx
        row, target, n_comparable = np.arange(Bx), pairs[:, 1].astype(np.int32), np.ones(Bx, np.int32)
    else:
        best = best_per_x(pairs, result, Bx)
        row, n_comparable = best["row"].copy(), best["n_comparable"]
        first_row = np.full(Bx, -1, np.int64)  # (a crystal whose pairs all failed reports its first pair's flags)
        for k in range(len(pairs) - 1, -1, -1):
            first_row[pairs[k, 0]] = k
        row = np.where(row >= 0, row, first_row)
        target = np.where(best["row"] >= 0, best["best"], -1).astype(np.int32)
    have = row >= 0
    safe = np.where(have, row, 0)
    fill = {"rms": np.inf, "rms_norm": np.inf, "max_dist": np.inf, "mapping": -1, "translation": 0.0, "n_mappings": 0, "n_candidates": 0,
            "n_permutations": 0, "matched": 0, "flags": DIFFERENT}
    out = {"target": target, "n_comparable": n_comparable.astype(np.int32)}
    for k, v in fill.items():
        a = np.asarray(result[k])
        got = a[safe] if len(a) else np.zeros((Bx,) + a.shape[1:], a.dtype)
        mask = have.reshape((-1,) + (1,) * (got.ndim - 1))
        out[k] = np.where(mask, got, np.asarray(v, dtype=a.dtype)).astype(a.dtype)
    part = np.asarray(result["partner"])
    out["partner"] = np.concatenate([part[row[b], :counts[b]] if have[b] else np.full(counts[b], -1, np.int32) for b in range(Bx)]
                                    + [np.empty(0, np.int32)]).astype(np.int32)
    return out


def match_batches(x_batch, x_counts, x_species, y, params=None, mode=None):
    """Device batch x (its host atom counts and species ids alongside) against the targets y (a SampleResult or a loaded file,
    uploaded here): paired when y has as many crystals as x (or mode "paired"), else every pair of equal composition reduced to
    the best target per crystal (mode "any").  Returns the MATCH_KEYS dict of numpy arrays and `mode`."""
    x_counts = np.asarray(x_counts, dtype=np.int64).reshape(-1)
    By = int(np.asarray(y.num_atoms).reshape(-1).shape[0])
    if mode is None:
        mode = "paired" if By == len(x_counts) else "any"
    if mode not in ("paired", "any"):
        raise ValueError(f"match mode must be 'paired' or 'any', got {mode!r}")
    if mode == "paired" and By != len(x_counts):
        raise ValueError(f"a paired match needs as many targets as crystals: {By} targets, {len(x_counts)} crystals")
    pairs = paired(len(x_counts)) if mode == "paired" else same_composition((x_counts, x_species), y)
    y_batch = cb.upload(y, x_batch[0].device)
    out = per_crystal(result_to_numpy(match(x_batch, y_batch, pairs, params)), pairs, x_counts, mode)
    out["mode"] = mode
    return out


def match_crystals(x, y, params=None, mode=None, device="cuda"):
    """`match_batches` for two SampleResults or loaded crystals files: float64 arrays cast to float32, atomic numbers as species."""
    counts, types = _counts_types(x)
    return match_batches(cb.upload(x, device), counts, types, y, params, mode)


def sample_arrays(matched):
    """What SampleResult.match and a crystals file hold (MATCH_KEYS) of a `match_batches` dict."""
    return {k: np.asarray(matched[k]) for k in MATCH_KEYS}


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) per-crystal arrays: attempted, matched, the sum of rms_norm
    and of rms over the matched, and the count per flag."""
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    ok = np.asarray(result["matched"], dtype=np.int64).reshape(-1) != 0
    norm, rms = np.asarray(result["rms_norm"], dtype=np.float64).reshape(-1), np.asarray(result["rms"], dtype=np.float64).reshape(-1)
    return {"rank": cb.rank_of(rank), "attempted": int(flags.size), "matched": int(ok.sum()),
            "sum_rms_norm": float(norm[ok].sum()), "sum_rms": float(rms[ok].sum()),
            "flags": cb.flag_counts(flags, ALL_FLAG_NAMES)}


def total_stats(parts):
    return {"rank": "total", "attempted": sum(p["attempted"] for p in parts), "matched": sum(p["matched"] for p in parts),
            "sum_rms_norm": sum(p["sum_rms_norm"] for p in parts), "sum_rms": sum(p["sum_rms"] for p in parts),
            "flags": {n: sum(p["flags"].get(n, 0) for p in parts) for _, n in ALL_FLAG_NAMES}}


def match_rate(st) -> float:
    return st["matched"] / st["attempted"] if st["attempted"] else 0.0


def format_stats(st) -> str:
    """'match rank 0: matched 14 / attempted 16 (rate 0.875); mean rms_norm 0.0412, mean rms 0.103 A; flags DIFFERENT 2'."""
    mean = f"mean rms_norm {st['sum_rms_norm'] / st['matched']:.4g}, mean rms {st['sum_rms'] / st['matched']:.4g} A" if st["matched"] \
        else "mean rms_norm n/a"
    return f"match {cb.who(st)}: matched {st['matched']} / attempted {st['attempted']} (rate {match_rate(st):.4g}); {mean}; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------------ the derived bounds
def longest_edge(lattice_x, ltol):
    """l_1 = (1 + ltol) x the longest edge of x's cell (module docstring)."""
    return (1.0 + float(ltol)) * float(np.linalg.norm(np.asarray(lattice_x, dtype=np.float64).reshape(3, 3), axis=1).max())


def difference_bound(n, D):
    """E_e: |float32 - exact| of a component of a difference e'_i formed with the refined translation."""
    return (88.0 + (n + 1.0) * D) * U


def translation_bound(n, D):
    """|float32 - exact| of a component of the refined translation t', modulo 1."""
    return (64.0 + (n + 1.0) * D) * U


def msd_bound(n, l1, D):
    """E_2: |float32 - exact| of a d^2 or of their mean, for differences with components within D + E_e."""
    De = D + difference_bound(n, D)
    return (351.0 + 9.0 * n) * U * l1 * l1 * De * De


def distance_bound(n, l1, D, value):
    """|float32 - exact| of rms or max_dist, `value` the restatement's (module docstring)."""
    lin, E2 = 3.0 * l1 * difference_bound(n, D), msd_bound(n, l1, D)
    root = math.sqrt(E2)
    if value - lin > 0.0:
        root = min(root, E2 / (value - lin))
    return lin + root + 4.0 * U * value


def norm_bound(n, l1, D, rms, ell, det_gm):
    """|float32 - exact| of rms_norm = rms / l; det_gm the determinant of the mean metric of the best candidate."""
    rho = l1 ** 6 / det_gm
    return distance_bound(n, l1, D, rms) / ell + (rms / ell) * (103.0 * rho + 9.0) * U


def cost_bound(l1, lam, c):
    """|float32 - exact| of one entry c (A^2) of a candidate's cost matrix, lam the smallest eigenvalue of its mean metric."""
    return 342.0 * U * l1 * l1 / lam * c + 216.0 * U * l1 * math.sqrt(c) + (108.0 * U * l1) ** 2 + 2.0 ** -25


def solver_bound(n, l1, lam, optimum):
    """SOLVER_BOUND: the most by which the exact sum of the kernel's assignment can exceed the true optimum sum (module docstring)."""
    a, b, c0 = 342.0 * U * l1 * l1 / lam, 216.0 * U * l1, (108.0 * U * l1) ** 2 + 2.0 ** -25
    f = a * optimum + b * math.sqrt(n * optimum) + n * c0
    root = (b * math.sqrt(n) + math.sqrt(b * b * n + 8.0 * (1.0 - a) * f)) / (2.0 * (1.0 - a))
    return root * root


# ------------------------------------------------------------------------------------------------- the assignment (numpy)
def linear_assignment(cost):
    """The one-to-one map rows -> columns of the smallest sum of a square cost matrix (+inf: the pair is excluded), by shortest
    augmenting paths as rule 6b states them: column duals 0, a row keeps the column of its row minimum (the smallest j on
    ties: the nearest partner) when it is the smallest row that claims it, the free rows are augmented in ascending order, the
    unscanned column of the smallest reduced distance is scanned next, ties to the smallest j.  Returns (columns [n], column duals
    [n]); a ValueError where no one-to-one map avoids the excluded pairs."""
    C = np.asarray(cost, dtype=np.float64)
    n = C.shape[0]
    assert C.shape == (n, n)
    start = C.argmin(axis=1)  # (the row duals are the row minima, implicitly: what makes the start dual feasible)
    x, y, v = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.zeros(n)
    for i in range(n):
        if np.isfinite(C[i, start[i]]) and y[start[i]] < 0:
            x[i], y[start[i]] = start[i], i
    for f in np.nonzero(x < 0)[0]:
        with np.errstate(invalid="ignore"):
            d = C[f] - v
        pred, open_ = np.full(n, f, np.int64), np.isfinite(d)
        while True:
            if not open_.any():
                raise ValueError("linear_assignment: no one-to-one map avoids the excluded pairs")
            j1 = int(np.where(open_, d, np.inf).argmin())
            lowest, open_[j1] = d[j1], False
            if not np.isfinite(lowest):
                raise ValueError("linear_assignment: no one-to-one map avoids the excluded pairs")
            i = int(y[j1])
            if i < 0:
                break
            with np.errstate(invalid="ignore"):
                nd = C[i] - v - (C[i, j1] - v[j1] - lowest)
            better = open_ & (nd < d)
            d[better], pred[better] = nd[better], i
        scanned = ~open_ & np.isfinite(d)
        v[scanned] += d[scanned] - lowest
        j = j1
        while True:
            i = int(pred[j])
            y[j], x[i], j = i, j, int(x[i])
            if i == f:
                break
    return x, v


def assignment_gap(cost, columns, duals):
    """The gap of an optimal assignment to the runner-up: the smallest optimum with one edge (i, columns[i]) forbidden, minus the
    optimum (+inf where there is no other map).  With the optimal duals the reduced costs R >= 0 vanish on the map; forbidding
    (i, columns[i]) costs the shortest path from row i back to its column through the other rows: R[i, j] + dist(j -> columns[i]),
    dist the shortest paths between columns under R[row of j, j'] (Floyd-Warshall)."""
    C = np.asarray(cost, dtype=np.float64)
    n = C.shape[0]
    if n < 2:
        return float("inf")
    x = np.asarray(columns, dtype=np.int64)
    rows = np.empty(n, np.int64)
    rows[x] = np.arange(n)
    u = C[np.arange(n), x] - duals[x]
    R = np.maximum(C - u[:, None] - duals[None, :], 0.0)
    D = R[rows].copy()  # [j, j']: leave column j through its row
    np.fill_diagonal(D, 0.0)
    for k in range(n):
        D = np.minimum(D, D[:, k, None] + D[None, k, :])
    R = R.copy()
    R[np.arange(n), x] = np.inf  # the forbidden edge itself
    return float((R + D[:, x].T).min())


# -------------------------------------------------------------------------------------------------- the numpy restatement
_IMAGES = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(27, 3).astype(np.float64)  # s_0 slowest


def _nearest_image(e, Gm):
    """Rule 4 on an array of differences [..., 3]: (d^2 [...], the difference of the image that attains it [..., 3])."""
    r = e - np.rint(e)
    cand = r[..., None, :] + _IMAGES  # [..., 27, 3]
    d2 = np.maximum(np.einsum("...a,ab,...b->...", cand, Gm, cand), 0.0)
    k = d2.argmin(axis=-1)  # (the first minimum)
    return np.take_along_axis(d2, k[..., None], -1)[..., 0], np.take_along_axis(cand, k[..., None, None], -2)[..., 0, :]


def metric_params(G):
    """(lengths [..., 3], angles [..., 3] in radians) of metrics [..., 3, 3]: angle i between the other two vectors, the quotient clamped."""
    with np.errstate(all="ignore"):
        ln = np.sqrt(np.stack([G[..., 0, 0], G[..., 1, 1], G[..., 2, 2]], -1))
        cos = np.stack([G[..., 1, 2] / (ln[..., 1] * ln[..., 2]), G[..., 0, 2] / (ln[..., 0] * ln[..., 2]), G[..., 0, 1] / (ln[..., 0] * ln[..., 1])], -1)
        return ln, np.arccos(np.clip(cos, -1.0, 1.0))


def mapping_deviations(Lx, Ly):
    """Rule 2 in float64: (codes [M], W [M,3,3], length_dev [M], angle_dev [M], G' [M,3,3]) over every candidate of det +-1:
    the largest | |a'_i| - |a^x_i| | / |a^x_i| and the largest |angle'_i - angle^x_i| in radians."""
    codes, W = ss._all_candidates()
    Lx, Ly = np.asarray(Lx, dtype=np.float64).reshape(3, 3), np.asarray(Ly, dtype=np.float64).reshape(3, 3)
    Wf = W.astype(np.float64)
    Gp = np.einsum("mki,kl,mlj->mij", Wf, Ly @ Ly.T, Wf)
    lx, ax = metric_params(Lx @ Lx.T)
    lp, ap = metric_params(Gp)
    with np.errstate(all="ignore"):
        return codes, W, (np.abs(lp - lx) / lx).max(axis=1), np.abs(ap - ax).max(axis=1), Gp


def evaluate_candidate(w, v, tx, ty, Gx, Gp, W, t=None, q=None, p0=None, partner=None, assignment="nearest"):
    """Rules 3, 4, 6 in float64 for one mapping W (G' = Gp) and either a start atom q (the search: t = wrap(w_p0 - v'_q), nearest
    partners; with assignment "optimal" the optimal assignment where those are not one-to-one, rule 6b) or a given translation t'
    and partner map (the check of a device's choice).  Returns a namespace: partner [n], permutation (bool: the nearest-partner
    map is one-to-one), nearest / second [n] (A; the search only), translation t' [3], e [n,3] (the differences under t'), rms,
    max_dist, ell, det_gm, lam (the smallest eigenvalue of G_m); solved (bool) and, where it is, optimum (the smallest sum, A^2)
    and gap (to the runner-up assignment, A^2)."""
    n = len(w)
    V = np.rint(np.linalg.inv(W.astype(np.float64)))
    vp = ss._wrap01(v @ V.T)
    Gm = (Gx + Gp) / 2.0
    out = SimpleNamespace(nearest=None, second=None, permutation=True, solved=False, optimum=None, gap=None)
    if partner is None:
        t0 = ss._wrap01(w[p0] - vp[q])
        d2, e = _nearest_image((vp[None, :, :] + t0[None, None, :]) - w[:, None, :], Gm)  # [i, j]
        d2 = np.where(tx[:, None] != ty[None, :], np.inf, d2)
        partner = d2.argmin(axis=1)
        srt = np.sqrt(np.sort(d2, axis=1))
        out.nearest, out.second = srt[:, 0], (srt[:, 1] if n > 1 else np.full(n, np.inf))
        out.permutation = len(set(partner.tolist())) == n
        if not out.permutation and assignment == "optimal":
            partner, duals = linear_assignment(d2)
            out.solved, out.optimum = True, float(d2[np.arange(n), partner].sum())
            out.gap = assignment_gap(d2, partner, duals)
        t = t0 - e[np.arange(n), partner].mean(axis=0)
    out.partner, out.translation = np.asarray(partner, dtype=np.int64), np.asarray(t, dtype=np.float64)
    d2, out.e = _nearest_image((vp[out.partner] + out.translation[None, :]) - w, Gm)
    out.rms, out.max_dist = math.sqrt(float(d2.mean())), math.sqrt(float(d2.max()))
    out.det_gm, out.lam = float(np.linalg.det(Gm)), float(np.linalg.eigvalsh(Gm)[0])
    out.ell = (math.sqrt(out.det_gm) / n) ** (1.0 / 3.0) if out.det_gm > 0 else float("nan")
    return out


def structure_match_reference_f64(x, y, pairs, params=None, details=False):
    """Rules 1-7 in float64 from the same float32 inputs: x, y = (frac [N,3], lattice [B,3,3], counts [B], types [N]) each, pairs
    [P,2].  Returns a namespace of the kernel's outputs (the reals float64; partner [P, stride], stride the largest atom count of
    x) and per pair `D` (the largest |component| of a difference under the best candidate's t'), `ell`, `det_gm`, `l1`.
    details=True adds, per pair (None where the decision is not reached): `length_dev` and `angle_dev` (of every candidate of det
    +-1), `nearest` and `second` ([candidates, n], A: the nearest and second-nearest partner distance of every candidate and atom)
    and `survivors`, the list of (rms, code, q) of every candidate whose map is a permutation, sorted; and, what params.assignment
    "optimal" adds, `contenders` (the sorted (rms, code, q) of every candidate that stands for the minimum: the survivors and the
    solved ones) and `solved`, one dict per candidate the assignment step solved: code, q, n, optimum, gap, lam, rms."""
    p = params if params is not None else StructureMatchParams()
    fx, Lx, cx, tx, firstx = cb.inputs(*x)
    fy, Ly, cy, ty, firsty = cb.inputs(*y)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P, stride = len(pairs), max([1] + cx)
    ltol, atol, stol = float(F32(p.ltol)), p.angle_tol_rad, float(F32(p.stol))
    out = SimpleNamespace(rms=np.full(P, np.inf), rms_norm=np.full(P, np.inf), max_dist=np.full(P, np.inf), mapping=np.full(P, -1, np.int32),
                          translation=np.zeros((P, 3)), partner=np.full((P, stride), -1, np.int32), n_mappings=np.zeros(P, np.int32),
                          n_candidates=np.zeros(P, np.int32), n_permutations=np.zeros(P, np.int32), matched=np.zeros(P, np.int32),
                          flags=np.zeros(P, np.int32), D=np.zeros(P), ell=np.full(P, np.nan), det_gm=np.full(P, np.nan), l1=np.zeros(P),
                          length_dev=[None] * P, angle_dev=[None] * P, nearest=[None] * P, second=[None] * P, survivors=[None] * P,
                          contenders=[None] * P, solved=[None] * P)
    for k, (bx, by) in enumerate(pairs):
        if not (0 <= bx < len(cx) and 0 <= by < len(cy)):
            out.flags[k] = BAD_PAIR
            continue
        A, B = Lx[bx].astype(np.float64), Ly[by].astype(np.float64)
        f, g = fx[firstx[bx]:firstx[bx + 1]].astype(np.float64), fy[firsty[by]:firsty[by + 1]].astype(np.float64)
        sx, sy = tx[firstx[bx]:firstx[bx + 1]], ty[firsty[by]:firsty[by + 1]]
        if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(f).all() and np.isfinite(g).all()):
            out.flags[k] = NONFINITE
            continue
        vols = [abs(float(np.dot(M[0], np.cross(M[1], M[2])))) for M in (A, B)]
        if any(not vol > 0.0 or not np.isfinite(vol) for vol in vols):
            out.flags[k] |= CELL
        if len(f) == 0 or len(g) == 0:
            out.flags[k] |= EMPTY
        if len(f) != len(g) or sorted(sx.tolist()) != sorted(sy.tolist()):
            out.flags[k] |= DIFFERENT
        if out.flags[k]:
            continue
        n = len(f)
        out.l1[k] = longest_edge(A, ltol)
        codes, W, ldev, adev, Gp = mapping_deviations(A, B)
        out.length_dev[k], out.angle_dev[k] = ldev, adev
        keep = np.nonzero((ldev <= ltol) & (adev <= atol))[0]
        out.n_mappings[k] = len(keep)
        if not len(keep):
            out.flags[k] = NO_MAPPING
            continue
        if len(keep) > p.max_mappings:
            out.flags[k] |= OVERFLOW
            keep = keep[:p.max_mappings]
        w, v, Gx = ss._wrap01(f.copy()), ss._wrap01(g.copy()), A @ A.T
        species, cnt = np.unique(sx, return_counts=True)
        rare = species[int(np.argmin(cnt))]  # the fewest atoms, the smallest id on ties
        p0, qs = int(np.nonzero(sx == rare)[0][0]), np.nonzero(sy == rare)[0]
        out.n_candidates[k] = len(keep) * len(qs)
        nearest, second, survivors, contenders, solved, best = [], [], [], [], [], None
        for m in keep:
            for q in qs:
                c = evaluate_candidate(w, v, sx, sy, Gx, Gp[m], W[m], q=int(q), p0=p0, assignment=p.assignment)
                nearest.append(c.nearest)
                second.append(c.second)
                key = (c.rms, int(codes[m]), int(q))
                if c.permutation:
                    survivors.append(key)
                if c.solved:
                    solved.append({"code": int(codes[m]), "q": int(q), "n": n, "optimum": c.optimum, "gap": c.gap, "lam": c.lam, "rms": c.rms})
                if c.permutation or c.solved:
                    contenders.append(key)
                    if best is None or key < best[0]:
                        best = (key, c)
        out.nearest[k], out.second[k], out.survivors[k] = np.array(nearest), np.array(second), sorted(survivors)
        out.contenders[k], out.solved[k] = sorted(contenders), solved
        out.n_permutations[k] = len(survivors)
        if best is None:
            out.flags[k] |= NO_PERMUTATION
            continue
        (rms, code, _), c = best
        out.rms[k], out.max_dist[k], out.mapping[k], out.translation[k] = rms, c.max_dist, code, c.translation
        out.partner[k, :n] = c.partner
        out.rms_norm[k], out.ell[k], out.det_gm[k], out.D[k] = rms / c.ell, c.ell, c.det_gm, float(np.abs(c.e).max())
        out.matched[k] = int(out.rms_norm[k] <= stol)
        if c.solved:
            out.flags[k] |= ASSIGNED
    if not details:
        del out.length_dev, out.angle_dev, out.nearest, out.second, out.survivors, out.contenders, out.solved
    return out
