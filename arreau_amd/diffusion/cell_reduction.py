"""Cell reduction of generated crystals: the pure translations a crystal has in the cell it is given, the primitive cell they
imply, a Delaunay-reduced (Selling) basis of that cell made of its shortest vectors, and one atom per translation class
expressed in it (arreau_crystal_reduce, arreau_amd/csrc/reduce.hip; the rules are written out in include/arreau_hip.h, "cell
reduction").  Here: the parameters and their validation, the flag constants, the entry point that needs no engine
(`reduce_cells`), `reduce_sample_result` for a SampleResult or a loaded file, `sample_arrays` / `reduced_crystals`, the statistics lines and a
float64 numpy restatement of rules 1-5 that reports the margin of every decision it takes (`reduce_reference_f64`).  The
restatement needs numpy alone.

What this is not: no Niggli form, no conventional or standardised setting, no space-group number.  The reduced basis is the
three shortest independent vectors among the seven a Selling-reduced superbase offers: for a given lattice its lengths are the
same whatever basis the cell came in, its choice among vectors of equal length is not.

Conventions.  The cell rows are a_0, a_1, a_2 (L); a fractional row x has the Cartesian position r = x L.  `transform` T holds the
reduced basis in the input basis, L_red = T L, det T = 1 / m; a position is x_red = w T^-1, and T^-1 = Q is an integer matrix.

float32 against float64.  Every arithmetic step of the kernel is one rounded float32 operation, never contracted; no float32
restatement of the whole is kept.  The float64 restatement takes every decision the kernel takes and reports its margin, the
distance of the decided quantity from its threshold, beside a bound on |float32 - exact| of that quantity; on a GUARDED input
(every margin above GUARD x its bound) the two agree on every discrete output, and the reals are held to the bounds below.
u = 2^-24, A = max_d sum_k |L_kd|.
  * a distance (rule 2, 5): w is exact up to u; t = wrap(w_q - w_p0): 2 u from its inputs, u from the difference, u from the wrap,
    4 u; y = w_i + t: 5 u and the sum's u (a value below 2), 6 u; delta = y - w_j: u + u more, 8 u; delta - rint(delta) is exact;
    e + s (below 1.5 in size): u, 9 u per component.  c_d = (e_0 L_0d + e_1 L_1d) + e_2 L_2d: 9 u A from the inputs and five
    roundings of values below 1.5 A, 16.5 u A per component, 29 u A in norm; the length's three products, two sums and square
    root add a relative 2 u of a length below 2.6 A: 5.2 u A.  |d_f32 - d_exact| <= 35 u A; DISTANCE_BOUND_FACTOR = 64 (the symmetry
    search's factor): bound = 64 u A.  A minimum or maximum moves no further than its arguments; a closure distance (of t_a + t_b
    - t_c) has fewer steps.
  * a vector (rules 3, 4) with coefficients c_k = num_k / m: the division and each product are relative u, each of the two sums
    rounds a value below S_d = sum_k |c_k| |L_kd|: 4 u S_d per component, 7 u S in norm, S = max_d S_d; VECTOR_BOUND_FACTOR = 8:
    B(v) = 8 u S.  A scalar product: B(v_i) |v_j| + B(v_j) |v_i| + B(v_i) B(v_j) from the vectors and 4 u |v_i| |v_j| from its own
    five operations (`scalar_bound`); a squared length likewise.  A determinant of three vectors of lengths l and bounds B:
    sum_i B_i l_j l_k for the vectors and 16 u l_0 l_1 l_2 for its fourteen operations; the volume test compares ||det| - V / m|
    with V / (4 m): V's own error (A^3 terms: 16 u |a_0| |a_1| |a_2|) enters both sides (`volume_bound`).
  * lattice_out row r = T_r L: 4 u max_d sum_k |T_rk| |L_kd| per component, LATTICE_BOUND = 8 u times that maximum.
  * frac_out = wrap((w_0 Q_0c + w_1 Q_1c) + w_2 Q_2c): u |Q_kc| from each w_k, u |Q_kc| from each product, two sums below S_c =
    sum_k |Q_kc|: 4 u S_c, and u for the wrap; POSITION_BOUND = (8 max_c S_c + 2) u, compared modulo 1.
Two squared lengths that are equal in float64 AND in the kernel's float32 operations (restated here for this one quantity) are an
exact tie: both sides decide it by index, no margin is asked of it (v and -v, the axes of a cubic cell).  Likewise a Selling
scalar whose float32 operations, restated here, give the float64 value itself carries no error (the zeros of a cubic lattice):
only tol's own rounding, 4 u tol, is asked of its margin."""
import math
from dataclasses import dataclass
from numbers import Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb

NONFINITE, CELL, EMPTY, AMBIGUOUS, NOT_CONVERGED = 1, 2, 4, 8, 16
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (AMBIGUOUS, "AMBIGUOUS"), (NOT_CONVERGED, "NOT_CONVERGED"))
COPIED_MASK = NONFINITE | CELL | EMPTY | AMBIGUOUS  # such a crystal is copied through unchanged
MAX_TRANSLATIONS = 64   # reduce.hip / arreau_hip.h: ARREAU_RED_MAX_TRANSLATIONS
MAX_STEPS = 64          # ARREAU_RED_MAX_STEPS
SELLING_TOL = 1e-5
DEFAULT_SYMPREC = 0.1
CRYSTAL_KEYS = ("multiplicity", "n_translations", "lattice_out", "transform", "n_out", "flags", "selling_steps")
ATOM_KEYS = ("frac_out", "types_out", "keep")
RED_KEYS = CRYSTAL_KEYS + ATOM_KEYS
U = 2.0 ** -24
DISTANCE_BOUND_FACTOR = 64.0
VECTOR_BOUND_FACTOR = 8.0
GUARD = 10.0
F32 = np.float32
PAIRS = ((0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 1, 2), (1, 2, 0, 3), (1, 3, 0, 2), (2, 3, 0, 1))  # (i, j, k, l) of a Selling step
_SHIFTS = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)  # lexicographic, s_0 slowest


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class CellReductionParams:
    """symprec: the tolerance in A on the distance between an atom's translated image and its partner (0.1, the symmetry
    search's default: a starting value, not a claim)."""
    symprec: float = DEFAULT_SYMPREC

    def __post_init__(self):
        v = self.symprec
        if not isinstance(v, Real) or isinstance(v, bool) or not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"symprec must be a finite number > 0, got {v!r}")
        object.__setattr__(self, "symprec", float(v))


def resolve(reduce_cell):
    """sample(reduce_cell=...): None / False -> None, True -> the defaults, a CellReductionParams -> itself."""
    return cb.resolve(reduce_cell, CellReductionParams, "reduce_cell")


# ------------------------------------------------------------------------------------------------------- the device call
def reduce_cells(frac, lattice, offsets, types, params=None):
    """Reduce a batch on the GPU without an engine (arreau_crystal_reduce, one launch).  frac [N,3] float32, lattice [B,3,3]
    float32 (rows a, b, c), offsets [B+1] int32 and types [N] int32 (species ids) are contiguous tensors on one cuda device.
    Returns a dict of device tensors: multiplicity, n_translations, n_out, flags, selling_steps, symprec [B]; lattice_out,
    transform [B,3,3]; frac_out [N,3], types_out [N], keep [N] (crystal b's n_out[b] atoms from offsets[b] on; keep -1 beyond
    them); and `offsets` (the input's).  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else CellReductionParams()
    dev, B, N = cb.check_batch("reduce_cells", frac, lattice, offsets, types)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"multiplicity": torch.empty(B, **i32), "n_translations": torch.empty(B, **i32), "lattice_out": torch.empty((B, 3, 3), **f32),
           "transform": torch.empty((B, 3, 3), **f32), "n_out": torch.empty(B, **i32), "flags": torch.empty(B, **i32),
           "selling_steps": torch.empty(B, **i32), "frac_out": torch.empty((N, 3), **f32), "types_out": torch.empty(N, **i32),
           "keep": torch.empty(N, **i32)}
    c = _hip.ReduceParamsC(p.symprec)
    r = _hip.ReduceResultC(*[_hip.ptr(out[k]).value if out[k].numel() else None for k in RED_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_reduce(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(offsets), B, N,
                                                    ctypes.byref(c), ctypes.byref(r), _hip.stream_ptr(dev)),
                   "arreau_crystal_reduce")
    out["symprec"] = torch.full((B,), float(F32(p.symprec)), **f32)
    out["offsets"] = offsets
    return out


def result_to_numpy(result):
    """The dict of `reduce_cells` as host numpy arrays (synchronises), with the reduced crystals beside them as a ragged batch
    (crystal_batch.compact_ragged): num_atoms [B] = n_out, frac_x [sum n_out, 3], types [sum n_out], lattice [B,3,3] = lattice_out."""
    out = cb.to_numpy(result)
    _, (out["frac_x"], out["types"]) = cb.compact_ragged(out["offsets"], out["n_out"], out["frac_out"], out["types_out"])
    out["num_atoms"], out["lattice"] = out["n_out"].astype(np.int64), out["lattice_out"]
    return out


def reduce_sample_result(result, params=None, device="cuda"):
    """The reduction of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32 and its atomic
    numbers taken as species ids: the dict of `result_to_numpy`."""
    return result_to_numpy(reduce_cells(*cb.upload(result, device), params))


REDUCED_KEYS = ("multiplicity", "n_translations", "lattice", "transform", "num_atoms", "flags", "selling_steps", "symprec", "frac_x",
                "atomic_numbers", "keep")
PER_ATOM_KEYS = ("frac_x", "atomic_numbers", "keep")  # [sum num_atoms, ...]: the reduced crystals' atoms, crystal after crystal


def sample_arrays(reduced, atomic_numbers=None):
    """What SampleResult.reduced and a crystals file hold (REDUCED_KEYS) of a `result_to_numpy` dict: one row per crystal, and the
    reduced crystals' atoms as a dense ragged batch.  atomic_numbers: of the reduced atoms (the species ids unless given)."""
    _, (keep,) = cb.compact_ragged(reduced["offsets"], reduced["n_out"], reduced["keep"])
    out = {k: np.asarray(reduced[k]) for k in ("multiplicity", "n_translations", "lattice", "transform", "num_atoms", "flags",
                                               "selling_steps", "symprec", "frac_x")}
    out["atomic_numbers"] = np.asarray(reduced["types"] if atomic_numbers is None else atomic_numbers)
    out["keep"] = keep
    return out


def reduced_crystals(reduced, atomic_numbers=None):
    """The reduced crystals of a `result_to_numpy` dict as the arrays of a crystals file: frac_x and lattice float64, atomic_numbers
    (the species ids unless given), num_atoms, idx_start."""
    z = (reduced["atomic_numbers"] if "atomic_numbers" in reduced else reduced["types"]) if atomic_numbers is None else atomic_numbers
    return cb.crystal_arrays(reduced["frac_x"], reduced["lattice"], z, reduced["num_atoms"])


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the count per multiplicity and per flag."""
    m = np.asarray(result["multiplicity"], dtype=np.int64).reshape(-1)
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    return {"rank": cb.rank_of(rank), "attempted": int(m.size), "reduced": int(((flags & COPIED_MASK) == 0).sum()),
            "multiplicity": {int(k): int((m == k).sum()) for k in np.unique(m)},
            "flags": cb.flag_counts(flags, FLAG_NAMES)}


def total_stats(parts):
    mult = {}
    for p in parts:
        for k, v in p["multiplicity"].items():
            mult[int(k)] = mult.get(int(k), 0) + v
    return {"rank": "total", "attempted": sum(p["attempted"] for p in parts), "reduced": sum(p["reduced"] for p in parts),
            "multiplicity": dict(sorted(mult.items())), "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'cell reduction rank 0: reduced 16 / attempted 16; multiplicity 1: 14, 2: 2; flags none'."""
    mult = cb.some(dict(sorted((int(k), v) for k, v in st["multiplicity"].items())), ": ")
    return f"cell reduction {cb.who(st)}: reduced {st['reduced']} / attempted {st['attempted']}; multiplicity {mult}; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# -------------------------------------------------------------------------------------------------- the numpy restatement
def _wrap01(v):
    w = v - np.floor(v)
    w[w >= 1.0] = 0.0
    return w


def min_image_distance(delta, L):
    """dist of the header: delta [...,3] fractional, each component minus its nearest integer, then the shortest of the 27 images."""
    e = delta - np.rint(delta)
    return np.linalg.norm((e[..., None, :] + _SHIFTS) @ L, axis=-1).min(axis=-1)


def column_sum(L):
    return float(np.abs(np.asarray(L, dtype=np.float64).reshape(3, 3)).sum(axis=0).max())


def distance_bound(L):
    """|d_float32 - d_exact| of a minimum-image distance in this cell (module docstring): 64 u A."""
    return DISTANCE_BOUND_FACTOR * U * column_sum(L)


def vector_bound(coef, L):
    """B(v) = 8 u max_d sum_k |c_k| |L_kd| of a vector v = c L."""
    return VECTOR_BOUND_FACTOR * U * float((np.abs(np.asarray(coef, dtype=np.float64)) @ np.abs(L)).max())


def scalar_bound(ci, cj, L):
    """|float32 - exact| of v_i . v_j for v = c L (module docstring)."""
    li, lj = np.linalg.norm(np.asarray(ci) @ L), np.linalg.norm(np.asarray(cj) @ L)
    bi, bj = vector_bound(ci, L), vector_bound(cj, L)
    return bi * lj + bj * li + bi * bj + 4.0 * U * li * lj


def volume_bound(coefs, L):
    """|float32 - exact| of ||det| - V / m| - V / (4 m) for the triple of vectors c L."""
    ln = [float(np.linalg.norm(np.asarray(c) @ L)) for c in coefs]
    bv = [vector_bound(c, L) for c in coefs]
    cell = 16.0 * U * float(np.prod(np.linalg.norm(L, axis=1))) * 1.25 + 4.0 * U * abs(float(np.linalg.det(L)))
    return bv[0] * ln[1] * ln[2] + bv[1] * ln[0] * ln[2] + bv[2] * ln[0] * ln[1] + 16.0 * U * ln[0] * ln[1] * ln[2] + cell


def lattice_bound(transform, L):
    return VECTOR_BOUND_FACTOR * U * float((np.abs(transform) @ np.abs(L)).max())


def position_bound(Q):
    return (8.0 * float(np.abs(Q).sum(axis=0).max()) + 2.0) * U


def _len2_f32(num, m, L32):
    """|v|^2 of the vector with numerators `num` over m in the kernel's float32 operations (for the exact-tie rule only)."""
    c = np.asarray(num, dtype=F32) / F32(m)
    v = (c[0] * L32[0] + c[1] * L32[1]) + c[2] * L32[2]
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def _vec_f32(num, m, L32):
    c = np.asarray(num, dtype=F32) / F32(m)
    return (c[0] * L32[0] + c[1] * L32[1]) + c[2] * L32[2]


def _scalar_f32(num_i, num_j, m, L32):
    """v_i . v_j in the kernel's float32 operations (for the exact-value rule only)."""
    a, b = _vec_f32(num_i, m, L32), _vec_f32(num_j, m, L32)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _ranked(nums, m, L, L32, margins):
    """The order of vectors (numerators [K,3] over m) by |v|^2, ties to the lower index; the gap of every neighbouring pair of the
    order that is not an exact tie goes to margins['length']."""
    nums = np.asarray(nums, dtype=np.int64)
    l64 = ((nums / m) @ L)
    l64 = (l64 * l64).sum(axis=1)
    l32 = np.array([_len2_f32(x, m, L32) for x in nums])
    order = sorted(range(len(nums)), key=lambda k: (l64[k], k))
    for a, b in zip(order, order[1:]):
        if l64[a] == l64[b] and l32[a] == l32[b]:
            continue
        bound = sum(2.0 * vector_bound(nums[k] / m, L) * math.sqrt(l64[k]) + vector_bound(nums[k] / m, L) ** 2 + 4.0 * U * l64[k] for k in (a, b))
        margins["length"].append((float(l64[b] - l64[a]), bound))
    return order


def _idet(a, b, c):
    return int(round(float(np.linalg.det(np.array([a, b, c], dtype=np.float64)))))


def reduce_reference_f64(frac, lattice, counts, types, params=None):
    """Rules 1-5 in float64 from the same float32 inputs: frac [N,3], lattice [B,3,3], counts [B] atoms per crystal, types [N].
    Returns a namespace of the ten outputs (the reals float64, laid out as the kernel's) and `margins`: per crystal a dict of
    lists of (margin, bound) pairs under 'residual' (rule 2's residuals and closure distances against symprec), 'volume' (the
    volume test's slack), 'selling' (every Selling scalar against tol at the step it was tested), 'length' (the gaps between
    squared lengths that decide an order) and 'partner' (rule 5: the gap between the nearest and the second atom).  `guarded(b)`
    of the module reads them."""
    p = params if params is not None else CellReductionParams()
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    assert frac.shape[0] == types.shape[0]
    B, N, symprec = len(counts), frac.shape[0], float(F32(p.symprec))
    out = SimpleNamespace(multiplicity=np.ones(B, np.int32), n_translations=np.zeros(B, np.int32), lattice_out=lattice.astype(np.float64),
                          transform=np.tile(np.eye(3), (B, 1, 1)), n_out=np.array(counts, np.int32), flags=np.zeros(B, np.int32),
                          selling_steps=np.zeros(B, np.int32), frac_out=frac.astype(np.float64), types_out=types.astype(np.int32),
                          keep=np.concatenate([np.arange(n) for n in counts] + [np.empty(0)]).astype(np.int32),
                          margins=[{k: [] for k in ("residual", "volume", "selling", "length", "partner")} for _ in range(B)],
                          inverse=np.tile(np.eye(3, dtype=np.int64), (B, 1, 1)))
    for b, n in enumerate(counts):
        L32 = lattice[b]
        L, f, ty = L32.astype(np.float64), frac[first[b]:first[b + 1]].astype(np.float64), types[first[b]:first[b + 1]]
        mg = out.margins[b]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        V = abs(float(np.dot(L[0], np.cross(L[1], L[2]))))
        if not V > 0.0 or not np.isfinite(V):
            out.flags[b] |= CELL
        if n == 0:
            out.flags[b] |= EMPTY
        if out.flags[b]:
            continue
        dbound = distance_bound(L)
        w = _wrap01(f)
        species, cnt = np.unique(ty, return_counts=True)
        qs = np.nonzero(ty == species[int(np.argmin(cnt))])[0]
        other = ty[:, None] != ty[None, :]
        trans = []
        for q in qs:
            t = _wrap01((w[q] - w[qs[0]])[None, :])[0]
            d = min_image_distance((w[:, None, :] + t) - w[None, :, :], L)
            d[other] = np.inf
            res = float(d.min(axis=1).max())
            mg["residual"].append((abs(res - symprec), dbound))
            if res <= symprec:
                trans.append(t)
        m = len(trans)
        out.n_translations[b] = m
        ambiguous = m > MAX_TRANSLATIONS or n % m != 0
        if not ambiguous:
            tr = np.array(trans)
            for ta in tr:
                dmin = min_image_distance((ta[None, :] + tr)[:, None, :] - tr[None, :, :], L).min(axis=1)
                mg["residual"].extend((abs(float(x) - symprec), dbound) for x in dmin)
                ambiguous |= bool((dmin > symprec).any())
        if ambiguous:
            out.flags[b] |= AMBIGUOUS
            continue
        # rule 3
        nums = [np.array(v) for v in ((m, 0, 0), (0, m, 0), (0, 0, m))]
        for t in trans[1:]:
            base = np.rint(m * (t - np.rint(t))).astype(np.int64)
            cand = base[None, :] + m * _SHIFTS
            l2 = (((cand / m) @ L) ** 2).sum(axis=1)
            order = _ranked(cand, m, L, L32, {"length": []})  # the order alone; only the gap behind the winner decides
            win = order[0]
            rivals = [k for k in order[1:] if not (l2[k] == l2[win] and _len2_f32(cand[k], m, L32) == _len2_f32(cand[win], m, L32))]
            if rivals:
                k = rivals[0]
                bound = sum(2.0 * vector_bound(cand[x] / m, L) * math.sqrt(l2[x]) + 4.0 * U * l2[x] for x in (win, k))
                mg["length"].append((float(l2[k] - l2[win]), bound))
            nums.append(cand[win])
        nums = np.array(nums, dtype=np.int64)
        K = len(nums)
        order = _ranked(nums, m, L, L32, mg)
        vec = (nums / m) @ L
        prim = None
        for i in range(K):
            for j in range(i + 1, K):
                for k in range(j + 1, K):
                    tri = [order[i], order[j], order[k]]
                    det = float(np.linalg.det(vec[tri]))
                    dev = abs(abs(det) - V / m)
                    mg["volume"].append((abs(dev - V / (4 * m)), volume_bound(nums[tri] / m, L)))
                    if dev <= V / (4 * m):
                        prim = nums[tri] * (-1 if det < 0 else 1)
                        break
                if prim is not None:
                    break
            if prim is not None:
                break
        if prim is None:
            out.flags[b] |= AMBIGUOUS
            continue
        # rule 4
        c = [np.array(r, dtype=np.int64) for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, -1, -1))]
        cart = lambda ci: ((ci @ prim) / m) @ L
        coef = lambda ci: (ci @ prim) / m
        tol = SELLING_TOL * max(float(np.dot(cart(x), cart(x))) for x in c[:3])
        steps = 0
        while steps < MAX_STEPS:
            hit = None
            for i, j, k, l in PAIRS:
                s = float(np.dot(cart(c[i]), cart(c[j])))
                exact = float(_scalar_f32(c[i] @ prim, c[j] @ prim, m, L32)) == s  # the float32 operations were exact: no error
                mg["selling"].append((abs(s - tol), (0.0 if exact else scalar_bound(coef(c[i]), coef(c[j]), L)) + 4.0 * U * tol))
                if s > tol:
                    hit = (i, k, l)
                    break
            if hit is None:
                break
            i, k, l = hit
            c[k], c[l], c[i] = c[k] + c[i], c[l] + c[i], -c[i]
            steps += 1
        seven = c + [c[0] + c[1], c[1] + c[2], c[2] + c[0]]
        order = _ranked(np.array([x @ prim for x in seven]), m, L, L32, mg)
        pick = [order[0]]
        for x in order[1:]:
            if len(pick) == 1 and np.any(np.cross(seven[pick[0]], seven[x]) != 0):
                pick.append(x)
            elif len(pick) == 2 and _idet(seven[pick[0]], seven[pick[1]], seven[x]) != 0:
                pick.append(x)
        sign = -1 if _idet(*[seven[x] for x in pick]) < 0 else 1
        R = np.array([sign * (seven[x] @ prim) for x in pick], dtype=np.int64)
        adj = np.rint(np.linalg.inv(R.astype(np.float64)) * _idet(*R)).astype(np.int64)
        if _idet(*R) != m * m or (adj % m != 0).any():
            out.flags[b] |= AMBIGUOUS
            continue
        Q = adj // m
        # rule 5
        rep = np.ones(n, dtype=bool)
        for t in trans[1:]:
            d = min_image_distance((w[:, None, :] + t) - w[None, :, :], L)
            d[other] = np.inf
            partner = d.argmin(axis=1)
            srt = np.sort(d, axis=1)
            if n > 1:
                mg["partner"].extend((float(x), 2.0 * dbound) for x in (srt[:, 1] - srt[:, 0]) if np.isfinite(x))
            rep &= partner >= np.arange(n)
        kept = np.nonzero(rep)[0]
        if kept.size != n // m:
            out.flags[b] |= AMBIGUOUS
            continue
        a0 = first[b]
        out.multiplicity[b], out.n_out[b], out.selling_steps[b] = m, kept.size, steps
        out.flags[b] |= NOT_CONVERGED if steps >= MAX_STEPS else 0
        out.transform[b], out.lattice_out[b], out.inverse[b] = R / m, (R / m) @ L, Q
        out.frac_out[a0:a0 + n], out.types_out[a0:a0 + n], out.keep[a0:a0 + n] = 0.0, -1, -1
        out.frac_out[a0:a0 + kept.size] = _wrap01(w[kept] @ Q.astype(np.float64))
        out.types_out[a0:a0 + kept.size], out.keep[a0:a0 + kept.size] = ty[kept], kept
    return out


def guard_ratio(margins):
    """The smallest margin / bound over every decision of one crystal's `margins` dict (inf when it took none)."""
    ratios = [mgn / bound for pairs in margins.values() for mgn, bound in pairs]
    return min(ratios) if ratios else math.inf


def guarded(margins) -> bool:
    """True when every decision's margin exceeds GUARD x its float32 bound: the kernel then takes the same decisions."""
    return guard_ratio(margins) > GUARD
