"""Conventional cells of generated crystals: from the primitive, Delaunay-reduced cell of a crystal (cell_reduction.py) and the
rotations the symmetry search finds in it (symmetry_search.py), the conventional cell with the atoms in it, its centring, its
Bravais lattice (aP, mP, mS, oP, oS, oI, oF, tP, tI, hR, hP, cP, cI, cF) and the Pearson symbol (arreau_crystal_conventional,
arreau_amd/csrc/conventional.hip; the rules are written out in include/arreau_hip.h, "conventional cell").  Here: the parameters
(the search's) and their validation, the flag constants, the names, the entry point that needs no engine (`conventional_cell`:
reduce -> search on the reduced batch -> conventional, three launches), `result_to_numpy`, `sample_arrays` /
`conventional_crystals`, the statistics lines and a float64 numpy restatement (`conventional_stage_f64` of the last launch on a
reduced batch, `conventional_reference_f64` of the chain, built on cell_reduction.reduce_reference_f64 and
symmetry_search.symmetry_reference_f64).  The restatement needs numpy alone.

What this is not: no space-group number, no origin shift, no ITA standard choice among the monoclinic centrings (A, C and I all
count as mS), no idealised metric -- the cell keeps its noise; to idealise, symmetrize the written crystals afterwards.

Conventions.  The reduced cell has rows a_0, a_1, a_2 (L); a lattice vector is an integer row v, v L in space; a rotation W of the
search acts on columns, v' = W v.  `transform` P holds the conventional vectors as rows in the reduced basis, L_conv = P L, det P
= n_points > 0; a position is x_conv = w adj(P) / det P.  In the conventional basis a rotation is (P^T)^-1 W P^T, which must be an
integer matrix.

float32 against float64.  All group arithmetic is on integers and exact.  Floats decide only which of several lattice vectors
is the shorter (and, in the monoclinic plane, the sign of a . c): squared lengths (v_0 L_0d + v_1 L_1d) + v_2 L_2d, (x x + y y) +
z z, one rounding per operation, relative error below 16 u (u = 2^-24; |v_k| <= 3 makes each component's absolute error at most
4 u sum_k |v_k L_kd|, which is a relative error only for vectors that are not much shorter than the cell rows they are made of:
the guard below is 1e-3, three orders above).  Vectors the crystal's own rotations map onto each other are exactly as long in exact
arithmetic: among them the integers decide (the lexicographically smallest P), never a float.  `decision_margins` gives the
relative gap of every float comparison that decided; on GUARDED crystals (every gap >= GUARD_MARGIN = 1e-3, and the reduction
and the search guarded by their own rules) the kernel takes the restatement's decisions and every integer output agrees.  The
reals, with S_r = max_d sum_k |P_rk| |L_kd| and BOUND_MARGIN = 1.25 for the second-order terms:
  * lattice row r = (P_r0 L_0d + P_r1 L_1d) + P_r2 L_2d: the products by small integers are relative u, the two sums round values
    below S_r: 4 u S_r per component (`lattice_bound`), B_r = 7 u S_r in norm;
  * lengths_r = sqrt((x x + y y) + z z) of that row: B_r from the row, 2.5 u l_r from the five operations and the root, l_r <= 1.8
    S_r: (7 + 4.5) u S_r -> 12 u S_r (`length_bound`);
  * cos(angle_i) = (v_j . v_k) / (l_j l_k): the scalar product B_j l_k + B_k l_j + 2.5 u l_j l_k, relative to l_j l_k that is e_jk
    = B_j / l_j + B_k / l_k + 2.5 u; the lengths' relative errors B_j / l_j + B_k / l_k + 5 u, the product and the quotient 2 u:
    |d cos| <= 2 (B_j / l_j + B_k / l_k) + 9.5 u; the angle: that over sin(angle), and 16 u for the device's acos (`angle_bound`);
  * positions: w is the float32 wrap on both sides (exact); q_c = ((w_0 A_0c + w_1 A_1c) + w_2 A_2c) + num_c, A = adj(P): three
    products (u |A_kc| each), three sums of values below S_c + 3, S_c = sum_k |A_kc|; the quotient by det P and the wrap, u each:
    ((4 S_c + 9) / det + 2) u, compared modulo 1 (`position_bound`)."""
import math
from dataclasses import dataclass
from itertools import permutations, product
from types import SimpleNamespace

import numpy as np

from . import cell_reduction as cr
from . import crystal_batch as cb
from . import symmetry_search as ss

NONFINITE, CELL, EMPTY, NO_GROUP, NO_BASIS = 1, 2, 4, 8, 16
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (NO_GROUP, "NO_GROUP"), (NO_BASIS, "NO_BASIS"))
BRAVAIS_NAMES = ("aP", "mP", "mS", "oP", "oS", "oI", "oF", "tP", "tI", "hR", "hP", "cP", "cI", "cF")
CENTRING_NAMES = ("P", "A", "B", "C", "I", "F", "R")  # the centring code is the position
CENTRING_P, CENTRING_A, CENTRING_B, CENTRING_C, CENTRING_I, CENTRING_F, CENTRING_R = range(7)
FAMILIES = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "hexagonal", "cubic")  # trigonal counts as hexagonal
# (family, centring) -> bravais code: what rule 5 admits
BRAVAIS_OF = {(0, CENTRING_P): 0, (1, CENTRING_P): 1, (1, CENTRING_A): 2, (1, CENTRING_C): 2, (1, CENTRING_I): 2, (2, CENTRING_P): 3,
              (2, CENTRING_C): 4, (2, CENTRING_I): 5, (2, CENTRING_F): 6, (3, CENTRING_P): 7, (3, CENTRING_I): 8, (4, CENTRING_R): 9,
              (4, CENTRING_P): 10, (5, CENTRING_P): 11, (5, CENTRING_I): 12, (5, CENTRING_F): 13}
ENUM_RANGE = 3          # conventional.hip: CONV_RANGE -- plane vectors are searched among integer rows with entries in -3..3
MAX_POINTS = 4
CRYSTAL_KEYS = ("lattice", "lengths", "angles", "transform", "centring", "bravais", "n_points", "num_atoms", "flags")
ATOM_KEYS_RAW = ("frac_out", "types_out", "source")
RESULT_KEYS = CRYSTAL_KEYS + ATOM_KEYS_RAW  # arreau_conventional_result, in its order
ATOM_KEYS = ("frac_x", "atomic_numbers", "source")  # [sum num_atoms, ...]: the conventional crystals' atoms, crystal after crystal
# what SampleResult.conventional and a crystals file hold; reduce_flags: the reduction's flags (cell_reduction.FLAG_NAMES) -- a
# crystal the reduction flagged is handed on in the cell it came in, and its conventional cell is that cell's
CONVENTIONAL_KEYS = CRYSTAL_KEYS + ("reduce_flags",) + ATOM_KEYS
U = 2.0 ** -24
BOUND_MARGIN = 1.25     # the second-order terms in u and the restatement's own rounding
GUARD_MARGIN = 1e-3     # the relative gap a deciding length comparison must have for the float32 kernel to decide alike
_FAMILY_OF_SYSTEM = {"triclinic": 0, "monoclinic": 1, "orthorhombic": 2, "tetragonal": 3, "trigonal": 4, "hexagonal": 4, "cubic": 5}
_ORDER_OF_TRACE = {3: 1, -1: 2, 0: 3, 1: 4, 2: 6}
# the centring translations as sorted numerators over n_points
_CENTRINGS = {1: {((0, 0, 0),): CENTRING_P},
              2: {((0, 0, 0), (0, 1, 1)): CENTRING_A, ((0, 0, 0), (1, 0, 1)): CENTRING_B, ((0, 0, 0), (1, 1, 0)): CENTRING_C,
                  ((0, 0, 0), (1, 1, 1)): CENTRING_I},
              3: {((0, 0, 0), (1, 2, 2), (2, 1, 1)): CENTRING_R},  # obverse; the reverse setting is no listed set
              4: {((0, 0, 0), (0, 2, 2), (2, 0, 2), (2, 2, 0)): CENTRING_F}}


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


def pearson_symbol(bravais, num_atoms) -> str:
    """'cF8' for the face-centred cubic lattice with 8 atoms in the conventional cell; 'none' for bravais -1."""
    return f"{BRAVAIS_NAMES[int(bravais)]}{int(num_atoms)}" if int(bravais) >= 0 else "none"


@dataclass(frozen=True)
class ConventionalCellParams(ss.SymmetrySearchParams):
    """The symmetry search's parameters: symprec, the tolerance in A the reduction and the search run with (0.1 by default), and
    max_ops, the operations stored per crystal -- a crystal with more is flagged NO_GROUP and copied through."""

    def search(self) -> ss.SymmetrySearchParams:
        return ss.SymmetrySearchParams(symprec=self.symprec, max_ops=self.max_ops)

    def reduction(self) -> cr.CellReductionParams:
        return cr.CellReductionParams(symprec=self.symprec)


def resolve(conventional_cell):
    """sample(conventional_cell=...): None / False -> None, True -> the defaults, a ConventionalCellParams -> itself."""
    return cb.resolve(conventional_cell, ConventionalCellParams, "conventional_cell")


def check_shared(conventional_params, reduce_params=None, find_symmetry_params=None, symmetrize_params=None):
    """sample(conventional_cell=..., reduce_cell=..., find_symmetry=...): the reduction's launch is shared, and the tolerances of
    every step that reads symmetry must be one: their parameters must agree."""
    a = conventional_params
    if a is None:
        return
    if reduce_params is not None and reduce_params.symprec != a.symprec:
        raise ValueError(f"conventional_cell and reduce_cell share one reduction: symprec {a.symprec} and {reduce_params.symprec} disagree")
    for name, b in (("find_symmetry", find_symmetry_params), ("symmetrize", symmetrize_params)):
        if b is not None and (a.symprec, a.max_ops) != (b.symprec, b.max_ops):
            raise ValueError(f"conventional_cell and {name} search with one tolerance: symprec / max_ops {a.symprec} / {a.max_ops} and "
                             f"{b.symprec} / {b.max_ops} disagree")


# ------------------------------------------------------------------------------------------------------- the device calls
def conventional_stage(frac, lattice, offsets, types, found):
    """The last launch alone (arreau_crystal_conventional): frac [N,3] float32, lattice [B,3,3] float32, offsets [B+1] int32 and
    types [N] int32 hold a batch that is ALREADY primitive and Delaunay-reduced, `found` is the dict of
    symmetry_search.find_symmetry on the same tensors.  Returns a dict of device tensors: lattice [B,3,3], lengths, angles [B,3],
    transform [B,3,3] int32, centring, bravais, n_points, num_atoms, flags [B]; frac_out [4N,3], types_out, source [4N] (crystal
    b's num_atoms[b] atoms from 4 offsets[b] on; source -1 beyond them); and `offsets`.  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    dev, B, N = cb.check_batch("conventional_cell", frac, lattice, offsets, types)
    M = int(found["ops_rotation"].shape[1])
    if int(found["ops_rotation"].shape[0]) != B or found["ops_rotation"].device != dev:
        raise ValueError("conventional_cell: `found` is not the search of this batch")
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"lattice": torch.empty((B, 3, 3), **f32), "lengths": torch.empty((B, 3), **f32), "angles": torch.empty((B, 3), **f32),
           "transform": torch.empty((B, 3, 3), **i32), "centring": torch.empty(B, **i32), "bravais": torch.empty(B, **i32),
           "n_points": torch.empty(B, **i32), "num_atoms": torch.empty(B, **i32), "flags": torch.empty(B, **i32),
           "frac_out": torch.empty((MAX_POINTS * N, 3), **f32), "types_out": torch.empty(MAX_POINTS * N, **i32),
           "source": torch.empty(MAX_POINTS * N, **i32)}
    s = _hip.SymmetryResultC(*[_hip.ptr(found[k]).value if B else None for k in ss.SYM_KEYS[:-1]])
    r = _hip.ConventionalResultC(*[_hip.ptr(out[k]).value if out[k].numel() else None for k in RESULT_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_conventional(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(offsets), B, N,
                                                          ctypes.byref(s), M, ctypes.byref(r), _hip.stream_ptr(dev)),
                   "arreau_crystal_conventional")
    out["offsets"] = offsets
    return out


def reduced_batch(reduced):
    """The reduced crystals of a cell_reduction.reduce_cells dict as a dense ragged device batch (frac, lattice, offsets, types):
    crystal b's first n_out[b] slots, gathered on the device (one synchronisation, for the number of atoms)."""
    import torch
    n_out, off = reduced["n_out"].to(torch.int64), reduced["offsets"].to(torch.int64)
    ends = torch.cumsum(n_out, 0)
    total = int(ends[-1]) if n_out.numel() else 0
    starts = ends - n_out
    rows = torch.arange(total, device=n_out.device) + torch.repeat_interleave(off[:-1] - starts, n_out, output_size=total)
    new_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=n_out.device), ends]).to(torch.int32)
    return (reduced["frac_out"][rows].contiguous(), reduced["lattice_out"].contiguous(), new_off.contiguous(),
            reduced["types_out"][rows].contiguous())


def conventional_cell(frac, lattice, offsets, types, params=None, reduced=None):
    """The conventional cells of a batch on the GPU without an engine: arreau_crystal_reduce (unless `reduced`, the dict of
    cell_reduction.reduce_cells on the same tensors, is handed in), arreau_crystal_symmetry on the reduced batch, then
    arreau_crystal_conventional.  The batch as for cell_reduction.reduce_cells.  Returns the dict of `conventional_stage`, with
    `reduced` and `found` (the dicts of the two earlier launches) beside it."""
    p = params if params is not None else ConventionalCellParams()
    cb.check_batch("conventional_cell", frac, lattice, offsets, types)
    if reduced is None:
        reduced = cr.reduce_cells(frac, lattice, offsets, types, p.reduction())
    batch = reduced_batch(reduced)
    found = ss.find_symmetry(*batch, p.search())
    out = conventional_stage(*batch, found)
    out["reduced"], out["found"] = reduced, found
    return out


def result_to_numpy(result):
    """The dict of `conventional_cell` (or `conventional_stage`) as host numpy arrays (synchronises), with the conventional crystals
    beside them as a dense ragged batch: frac_x [sum num_atoms, 3], types and source [sum num_atoms]."""
    out = cb.to_numpy({k: v for k, v in result.items() if k not in ("found", "reduced")})
    wide = MAX_POINTS * np.asarray(out["offsets"], dtype=np.int64)
    _, (out["frac_x"], out["types"], out["source"]) = cb.compact_ragged(wide, out["num_atoms"], out["frac_out"], out["types_out"], out["source"])
    reduced = result.get("reduced")
    out["reduce_flags"] = reduced["flags"].cpu().numpy() if reduced is not None else np.zeros_like(out["flags"])
    return out


def conventional_sample_result(result, params=None, device="cuda"):
    """The conventional cells of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32 and its
    atomic numbers taken as species ids: the dict of `result_to_numpy`."""
    return result_to_numpy(conventional_cell(*cb.upload(result, device), params))


def sample_arrays(conventional, atomic_numbers=None):
    """What SampleResult.conventional and a crystals file hold (CONVENTIONAL_KEYS) of a `result_to_numpy` dict.  atomic_numbers:
    of the conventional atoms (the species ids unless given)."""
    out = {k: np.asarray(conventional[k]) for k in CRYSTAL_KEYS + ("reduce_flags", "frac_x", "source")}
    out["atomic_numbers"] = np.asarray(conventional["types"] if atomic_numbers is None else atomic_numbers)
    return {k: out[k] for k in CONVENTIONAL_KEYS}


def conventional_crystals(conventional, atomic_numbers=None):
    """The conventional crystals as the arrays of a crystals file: frac_x and lattice float64, atomic_numbers (the stored ones
    unless given), num_atoms, idx_start."""
    z = (conventional["atomic_numbers"] if "atomic_numbers" in conventional else conventional["types"]) if atomic_numbers is None else atomic_numbers
    return cb.crystal_arrays(conventional["frac_x"], conventional["lattice"], z, conventional["num_atoms"])


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the count per Bravais lattice and per flag."""
    bravais = np.asarray(result["bravais"], dtype=np.int64).reshape(-1)
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    return {"rank": cb.rank_of(rank), "attempted": int(bravais.size), "classified": int((bravais >= 0).sum()),
            "bravais": {name: int((bravais == k).sum()) for k, name in enumerate(BRAVAIS_NAMES)},
            "flags": cb.flag_counts(flags, FLAG_NAMES)}


def total_stats(parts):
    return {"rank": "total", "attempted": sum(p["attempted"] for p in parts), "classified": sum(p["classified"] for p in parts),
            "bravais": {n: sum(p["bravais"][n] for p in parts) for n in BRAVAIS_NAMES},
            "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'conventional cell rank 0: classified 15 / attempted 16; aP 12, cF 3; flags NO_GROUP 1'."""
    return f"conventional cell {cb.who(st)}: classified {st['classified']} / attempted {st['attempted']}; {cb.some(st['bravais'])}; " \
           f"flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------------ the derived bounds
def _row_sums(P, L):
    return (np.abs(np.asarray(P, dtype=np.float64)) @ np.abs(np.asarray(L, dtype=np.float64).reshape(3, 3))).max(axis=1)  # S_r [3]


def lattice_bound(P, L):
    """|float32 - exact| of a component of the conventional lattice (module docstring): 4 u max_r S_r, with the margin."""
    return BOUND_MARGIN * 4.0 * U * float(_row_sums(P, L).max())


def length_bound(P, L):
    """|float32 - exact| of a conventional cell length: 12 u max_r S_r, with the margin."""
    return BOUND_MARGIN * 12.0 * U * float(_row_sums(P, L).max())


def angle_bound(P, L, angles):
    """|float32 - exact| of a conventional cell angle: ((2 (B_j / l_j + B_k / l_k) + 9.5 u) / sin + 16 u), B_r = 7 u S_r, the worst
    pair of rows and the smallest sine of the restatement's `angles` [3], with the margin."""
    S = _row_sums(P, L)
    ln = np.linalg.norm(np.asarray(P, dtype=np.float64) @ np.asarray(L, dtype=np.float64).reshape(3, 3), axis=1)
    rel = np.sort(7.0 * S / ln)[1:].sum()
    return BOUND_MARGIN * ((2.0 * rel + 9.5) / float(np.sin(np.asarray(angles, dtype=np.float64)).min()) + 16.0) * U


def position_bound(P):
    """|float32 - exact| of a component of a conventional position, modulo 1: ((4 S_c + 9) / det + 2) u, with the margin."""
    P = np.asarray(P, dtype=np.int64)
    return BOUND_MARGIN * ((4.0 * float(np.abs(_adjugate(P)).sum(axis=0).max()) + 9.0) / abs(_idet(P)) + 2.0) * U


# -------------------------------------------------------------------------------------------------- the numpy restatement
def _idet(M):
    M = np.asarray(M, dtype=np.int64)
    return int(M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
               + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def _adjugate(M):
    """adj(M) with M adj(M) = det(M) I, on integers."""
    M = np.asarray(M, dtype=np.int64)
    c = lambda i, j: M[(i + 1) % 3, (j + 1) % 3] * M[(i + 2) % 3, (j + 2) % 3] - M[(i + 1) % 3, (j + 2) % 3] * M[(i + 2) % 3, (j + 1) % 3]
    return np.array([[c(j, i) for j in range(3)] for i in range(3)], dtype=np.int64)


def _primitive(v):
    """An integer vector divided by the gcd of its entries, the first non-zero entry made positive."""
    v = np.asarray(v, dtype=np.int64)
    g = int(np.gcd.reduce(np.abs(v)))
    v = v // g
    return -v if v[np.nonzero(v)[0][0]] < 0 else v


def proper_part(W):
    """(W' = det(W) W, its order from its trace; 0 when the trace is none of 3, -1, 0, 1, 2)."""
    W = np.asarray(W, dtype=np.int64)
    Wp = W * _idet(W)
    return Wp, _ORDER_OF_TRACE.get(int(np.trace(Wp)), 0)


def axis_of(Wp, order):
    """(axis, normal) of a proper part of order > 1: S = sum_{j < order} W'^j has rank 1; the axis is its first non-zero column
    and the normal of the perpendicular lattice plane {v : S v = 0} its first non-zero row, both made primitive."""
    S, M = np.zeros((3, 3), dtype=np.int64), np.eye(3, dtype=np.int64)
    for _ in range(order):
        S, M = S + M, M @ Wp
    cols = [j for j in range(3) if S[:, j].any()]
    rows = [i for i in range(3) if S[i].any()]
    if not cols:
        return None, None
    return _primitive(S[:, cols[0]]), _primitive(S[rows[0]])


_ENUM = None


def _enumeration(rng=ENUM_RANGE):
    """The integer rows with entries in -rng..rng in lexicographic order, v_0 slowest."""
    global _ENUM
    if rng != ENUM_RANGE:
        return np.stack(np.meshgrid(*[np.arange(-rng, rng + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    if _ENUM is None:
        _ENUM = np.stack(np.meshgrid(*[np.arange(-rng, rng + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return _ENUM


def _shortest(cand, len2, margins, equivalent):
    """The first candidate of the smallest squared length (strict comparison in enumeration order); the relative gap to the
    shortest candidate that is not `equivalent` to it goes to margins."""
    k = int(np.argmin(len2))  # (the first minimum)
    rivals = [j for j in range(len(cand)) if not equivalent(cand[k], cand[j])]
    if rivals:
        margins.append(float((len2[rivals].min() - len2[k]) / len2[k]))
    return cand[k]


def _centring(P):
    """(n_points, centring code or -1, the sorted numerators [n_points, 3] over n_points) of a transform of positive determinant."""
    det = _idet(P)
    if not 1 <= det <= MAX_POINTS:
        return det, -1, np.zeros((1, 3), dtype=np.int64)
    A = _adjugate(P)
    pts = sorted({tuple(int(x) for x in ((i * A[0] + j * A[1] + k * A[2]) % det)) for i in range(det) for j in range(det) for k in range(det)})
    if len(pts) != det:
        return det, -1, np.zeros((1, 3), dtype=np.int64)
    return det, _CENTRINGS[det].get(tuple(pts), -1), np.array(pts, dtype=np.int64)


def _smallest(Ps):
    """The lexicographically smallest (row-major) of the right-handed candidates; None without one."""
    Ps = [P for P in Ps if _idet(P) > 0]
    return min(Ps, key=lambda P: tuple(int(x) for x in np.asarray(P).reshape(-1))) if Ps else None


def conventional_basis(L, rotations, family, enum_range=ENUM_RANGE):
    """Rules 2-4 for one reduced cell L [3,3] float64 and the distinct rotations of its group, in code order: (P or None, margins)."""
    margins = []
    parts = [proper_part(W) for W in rotations]
    if any(order == 0 for _, order in parts):
        return None, margins
    of_order = lambda n: [Wp for Wp, order in parts if order == n]
    len2 = lambda v: ((np.asarray(v, dtype=np.float64) @ L) ** 2).sum(axis=-1)
    enum = _enumeration(enum_range)

    def plane(normal):
        c = enum[(enum @ normal == 0) & enum.any(axis=1)]
        return c, len2(c)

    def orbit(v, gens):
        seen, todo = {tuple(int(x) for x in v)}, [np.asarray(v, dtype=np.int64)]
        while todo:
            x = todo.pop()
            for g in gens:
                for y in (g @ x, -(g @ x)):
                    if tuple(int(t) for t in y) not in seen:
                        seen.add(tuple(int(t) for t in y))
                        todo.append(y)
        return seen

    def distinct_axes(ws, order):
        axes = []
        for Wp in ws:
            ax, _ = axis_of(Wp, order)
            if ax is None:
                return None
            if not any((ax == a).all() for a in axes):
                axes.append(ax)
        return axes

    if family == 0:
        return np.eye(3, dtype=np.int64), margins
    if family == 1:
        twos = of_order(2)
        if not twos:
            return None, margins
        b, normal = axis_of(twos[0], 2)
        if b is None:
            return None, margins
        cand, l2 = plane(normal)
        if not len(cand):
            return None, margins
        a = _shortest(cand, l2, margins, lambda x, y: (x == y).all() or (x == -y).all())
        free = np.cross(cand, a).any(axis=1)
        if not free.any():
            return None, margins
        c = _shortest(cand[free], l2[free], margins, lambda x, y: (x == y).all() or (x == -y).all())
        dot = float((a.astype(np.float64) @ L) @ (c.astype(np.float64) @ L))
        margins.append(abs(dot) / math.sqrt(float(len2(a) * len2(c))) if dot != 0.0 else math.inf)
        if dot > 0.0:
            c = -c
        return _smallest([np.array([s * a, t * b, s * c]) for s in (1, -1) for t in (1, -1)]), margins
    if family == 2:
        axes = distinct_axes(of_order(2), 2)
        if axes is None or len(axes) != 3:
            return None, margins
        l2 = [float(len2(v)) for v in axes]
        order = sorted(range(3), key=lambda k: (l2[k], k))
        for x, y in zip(order, order[1:]):
            margins.append((l2[y] - l2[x]) / l2[x])
        s = [axes[k] for k in order]
        P = np.array(s)
        _, centring, _ = _centring(P * (1 if _idet(P) > 0 else -1))
        if centring == CENTRING_A:
            s = [s[1], s[2], s[0]]
        elif centring == CENTRING_B:
            s = [s[0], s[2], s[1]]
        return _smallest([np.array([p * s[0], q * s[1], r * s[2]]) for p in (1, -1) for q in (1, -1) for r in (1, -1)]), margins
    if family in (3, 4):
        n = 4 if family == 3 else 3
        main = of_order(4) if family == 3 else (of_order(6) or of_order(3))
        rot = of_order(n)
        if not main or not rot:
            return None, margins
        c, normal = axis_of(main[0], 4 if family == 3 else (6 if of_order(6) else 3))
        if c is None:
            return None, margins
        R = rot[0]
        Rinv = np.linalg.matrix_power(R, n - 1)
        cand, l2 = plane(normal)
        if not len(cand):
            return None, margins
        mates = None

        def equivalent(x, y):
            nonlocal mates
            if mates is None:
                mates = orbit(x, [R])
            return tuple(int(t) for t in y) in mates
        a0 = _shortest(cand, l2, margins, equivalent)
        Ps = []
        for a in sorted(orbit(a0, [R])):
            a = np.array(a, dtype=np.int64)
            for Rk in (R, Rinv):
                P = np.array([a, Rk @ a, c])
                if _idet(P) > 0 and (family == 3 or _idet(P) != 3 or _centring(P)[1] == CENTRING_R):
                    Ps.append(P)
        return _smallest(Ps), margins
    fours = of_order(4)
    axes = distinct_axes(fours, 4) if fours else distinct_axes(of_order(2), 2)
    if axes is None or len(axes) != 3:
        return None, margins
    return _smallest([np.array([p * axes[i], q * axes[j], r * axes[k]]) for i, j, k in permutations(range(3))
                      for p, q, r in product((1, -1), repeat=3)]), margins


def params_of_lattice(L):
    """(lengths [3], angles [3] in radians) of cell rows: angle i lies between the other two vectors."""
    with np.errstate(all="ignore"):
        ln = np.linalg.norm(L, axis=1)
        ang = np.array([np.arccos(np.clip(L[(i + 1) % 3] @ L[(i + 2) % 3] / (ln[(i + 1) % 3] * ln[(i + 2) % 3]), -1.0, 1.0)) for i in range(3)])
    return ln, ang


def conventional_stage_f64(frac, lattice, counts, types, found, enum_range=ENUM_RANGE):
    """The rules of arreau_crystal_conventional in float64 from the same float32 inputs: a reduced batch frac [N,3], lattice
    [B,3,3], counts [B], types [N] and `found`, the search of that batch (the namespace of symmetry_search.symmetry_reference_f64
    or the numpy dict of a device search).  Returns a namespace of the kernel's outputs as dense ragged arrays (frac_x, types,
    source of the conventional atoms; the reals float64) and, per crystal, `margins`: the relative gaps `decision_margins` reads."""
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    get = (lambda k: found[k]) if isinstance(found, dict) else (lambda k: getattr(found, k))
    B, M = len(counts), int(np.asarray(get("ops_rotation")).shape[1])
    out = SimpleNamespace(lattice=np.zeros((B, 3, 3)), lengths=np.zeros((B, 3)), angles=np.zeros((B, 3)),
                          transform=np.tile(np.eye(3, dtype=np.int32), (B, 1, 1)), centring=np.zeros(B, np.int32),
                          bravais=np.full(B, -1, np.int32), n_points=np.ones(B, np.int32), num_atoms=np.array(counts, np.int32),
                          flags=np.zeros(B, np.int32), margins=[[] for _ in range(B)], rotations=[[] for _ in range(B)])
    fx, ty_out, src = [], [], []
    for b, n in enumerate(counts):
        a0 = first[b]
        L32, f32, ty = lattice[b], frac[a0:a0 + n], types[a0:a0 + n]
        L, f = L32.astype(np.float64), f32.astype(np.float64)
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
        else:
            vol = abs(float(np.dot(L[0], np.cross(L[1], L[2]))))
            out.flags[b] = (CELL if (not vol > 0.0 or not np.isfinite(vol)) else 0) | (EMPTY if n == 0 else 0)
        K, pg = int(get("n_ops")[b]), int(get("point_group")[b])
        if not out.flags[b] and (int(get("flags")[b]) & (ss.AMBIGUOUS | ss.OVERFLOW | ss.NOT_A_GROUP) or not 1 <= K <= M or not 0 <= pg < 32):
            out.flags[b] = NO_GROUP
        P = None
        if not out.flags[b]:
            codes = [int(c) for c in np.asarray(get("ops_rotation"))[b, :K]]
            if any(not 0 <= c < ss.N_CODES for c in codes):
                out.flags[b] = NO_GROUP
        if not out.flags[b]:
            rotations = [ss.decode_rotation(c) for k, c in enumerate(codes) if k == 0 or codes[k - 1] != c]
            if any(abs(_idet(W)) != 1 for W in rotations) or len(rotations) > ss.MAX_LATTICE:
                out.flags[b] = NO_GROUP
        if not out.flags[b]:
            family = _FAMILY_OF_SYSTEM[ss.POINT_GROUP_SYSTEMS[pg]]
            P, out.margins[b] = conventional_basis(L, rotations, family, enum_range)
            out.rotations[b] = rotations
            ok = P is not None
            if ok:
                det, centring, pts = _centring(P)
                ok = centring >= 0 and (family, centring) in BRAVAIS_OF
            if ok:
                A = _adjugate(P)
                ok = all(((A.T @ W @ P.T) % det == 0).all() for W in rotations)
            if not ok:
                out.flags[b], P = NO_BASIS, None
        if P is None:  # copied through
            out.lattice[b] = L
            fx.append(f), ty_out.append(ty), src.append(np.arange(n))
        else:
            out.transform[b], out.centring[b], out.bravais[b], out.n_points[b] = P, centring, BRAVAIS_OF[(family, centring)], det
            out.num_atoms[b] = n * det
            out.lattice[b] = P.astype(np.float64) @ L
            w = ss._wrap01(f32.copy()).astype(np.float64)  # the float32 wrap: the kernel's values
            q = w @ A.astype(np.float64)
            fx.append(np.concatenate([ss._wrap01((q + t.astype(np.float64)) / det) for t in pts]))
            ty_out.append(np.tile(ty, det)), src.append(np.tile(np.arange(n), det))
        out.lengths[b], out.angles[b] = params_of_lattice(out.lattice[b])
    out.frac_x = np.concatenate(fx + [np.empty((0, 3))])
    out.types = np.concatenate(ty_out + [np.empty(0, np.int64)]).astype(np.int64)
    out.source = np.concatenate(src + [np.empty(0, np.int64)]).astype(np.int32)
    return out


def reduced_arrays_f64(red, counts):
    """(frac [sum n_out, 3] float32, lattice [B,3,3] float32, counts, types) of a cell_reduction.reduce_reference_f64 namespace:
    the reduced batch as the device hands it on, rounded to float32."""
    first = np.concatenate([[0], np.cumsum([int(n) for n in counts])])
    _, (frac, types) = cb.compact_ragged(first, red.n_out, red.frac_out, red.types_out)
    return frac.astype(np.float32), red.lattice_out.astype(np.float32), [int(n) for n in red.n_out], types.astype(np.int64)


def conventional_reference_f64(frac, lattice, counts, types, params=None, enum_range=ENUM_RANGE):
    """The chain in float64: cell_reduction.reduce_reference_f64, the reduced batch rounded to float32 (what the device hands on),
    symmetry_search.symmetry_reference_f64 on it, then `conventional_stage_f64`.  Returns the stage's namespace with `reduced`,
    `found` and `batch` (the reduced float32 batch) beside it."""
    p = params if params is not None else ConventionalCellParams()
    red = cr.reduce_reference_f64(frac, lattice, counts, types, p.reduction())
    batch = reduced_arrays_f64(red, counts)
    found = ss.symmetry_reference_f64(*batch, p.search(), details=True)
    out = conventional_stage_f64(*batch, found, enum_range)
    out.reduced, out.found, out.batch, out.reduce_flags = red, found, batch, red.flags
    return out


def decision_margins(ref, b):
    """The relative gap of every length comparison (and of the monoclinic a . c against 0) that decided a basis vector of crystal b
    of a restatement; empty for a crystal that took none (triclinic, cubic, flagged)."""
    return list(ref.margins[int(b)])


def guarded(ref, b) -> bool:
    """True when every deciding comparison of crystal b has a relative gap of at least GUARD_MARGIN."""
    return all(m >= GUARD_MARGIN for m in decision_margins(ref, b))


def search_guarded(found, b, symprec) -> bool:
    """True when every decision quantity of the search of crystal b (a namespace of symmetry_search.symmetry_reference_f64 with
    details=True) is at most symprec / 2 or at least 2 symprec: the float32 search then finds the same operations."""
    values = [v for v in (found.lattice_dev[int(b)], found.all_residuals[int(b)]) if v is not None]
    return all(bool(((v <= 0.5 * symprec) | (v >= 2.0 * symprec)).all()) for v in values)
