"""Symmetry search of generated crystals: the operations x' = W x + t a crystal has in the cell it is given, its point group and
its crystal system (arreau_crystal_symmetry, arreau_amd/csrc/symfind.hip; the rules are written out in include/arreau_hip.h,
"symmetry search").  Here: the parameters and their validation, the flag constants, the 32 point groups (names, crystal systems,
generators and the count table closed from them with symmetry.close_group), the rotation code, the entry point that needs no
engine (`find_symmetry`), `symmetry_sample_result` for a SampleResult or a loaded file, `contains`, the statistics lines and a
float64 numpy restatement of rules 1-6 for the tests (`symmetry_reference_f64`).  The restatement needs numpy alone.

What this is not: no space-group number (that needs the table of the 230 groups and an origin search), no standardisation of
the cell, no reduction to a primitive cell.  An operation whose matrix in the given basis has an entry outside {-1, 0, 1} is not
found: every conventional setting and the rhombohedral axes are covered, a badly skewed cell may not be.

Conventions.  The cell rows are a_0, a_1, a_2 (L); a fractional column x has the Cartesian position r_d = sum_k x_k L_kd.  An
operation acts on fractional columns, x' = W x + t.  Column j of W holds the image a'_j = sum_k W_kj a_k of basis vector a_j, so
with the metric G = L L^T (G_ij = a_i . a_j) the image basis has the metric G' = W^T G W and W is an isometry of the lattice
exactly when G' = G.  The rotation code of W is sum_{r,c} (W_rc + 1) 3^(3r + c): W_00 is the least significant base-3 digit;
the identity has code 16484.

float32 against float64 (rule 7).  Every arithmetic step of the kernel is one rounded float32 operation, never contracted to a
fused multiply-add, but no float32 restatement is kept: the integer outputs are compared with the float64 restatement on
GUARDED inputs -- every decision quantity (the deviation of a lattice candidate, the residual of an operation) at most
symprec / 2 or at least 2 symprec -- where the two agree on every discrete output.  The reals are held to a derived bound.
u = 2^-24 is the unit roundoff, A = max_d sum_k |L_kd|.
  * a wrapped coordinate w = f - floor(f) is exact up to u; W w (entries -1, 0, 1: the products are exact) is two sums of values
    below 3: at most 5 u; the translation t = wrap(w_q - W w_p0): the difference of values below 4 adds 4 u, the wrap u:
    |dt| <= 10 u -- TRANSLATION_BOUND = 16 u, on a component of t compared modulo 1;
  * y = W w_i + t: 5 u + 10 u and the sum's 4 u; delta = y - w_j: 5 u more, 24 u; delta - rint(delta) is exact;
  * c_d = (delta_0 L_0d + delta_1 L_1d) + delta_2 L_2d with |delta_k| <= 1/2: the inputs' 24 u A and five roundings of values
    below A / 2: 26.5 u A per component, 46 u A in norm; the three products, two sums and the square root of the length add a
    relative 2 u of a length below 0.87 A: 1.8 u A.
Together |residual_f32 - residual_exact| <= 48 u A (the residual is a max of minima of such lengths, and neither moves further
than its arguments); RESIDUAL_BOUND_FACTOR = 64 leaves the margin for the second-order terms: bound = 64 * 2^-24 * A, 3.8e-5 A
for a 10 A cubic cell."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from . import symmetry as sym_mod

NONFINITE, CELL, EMPTY, AMBIGUOUS, OVERFLOW, NOT_A_GROUP = 1, 2, 4, 8, 16, 32
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (AMBIGUOUS, "AMBIGUOUS"), (OVERFLOW, "OVERFLOW"),
              (NOT_A_GROUP, "NOT_A_GROUP"))
NO_RESULT_MASK = NONFINITE | CELL | EMPTY | AMBIGUOUS  # nothing else is reported for such a crystal
MAX_OPS_CAP = 4096        # symfind.hip / arreau_hip.h: ARREAU_SYM_MAX_OPS_CAP
MAX_LATTICE = 48          # a lattice has at most 48 isometries
STAGED_ATOMS = cb.STAGED_ATOMS  # also the number of candidate translations handled per round (symfind.hip: SYM_ROUND)
N_CODES = 3 ** 9
IDENTITY_CODE = 16484
DEFAULT_SYMPREC, DEFAULT_MAX_OPS = 0.1, 192
SYM_KEYS = ("n_lattice", "n_ops", "n_translations", "ops_rotation", "ops_translation", "ops_residual", "residual", "point_group",
            "flags", "symprec")
RESIDUAL_BOUND_FACTOR = 64.0
TRANSLATION_BOUND = 16.0 * 2.0 ** -24
F32 = np.float32

# rotation types in the order of the count vector: proper 1, 2, 3, 4, 6, then improper -1, m, -3, -4, -6
ROTATION_TYPES = ("1", "2", "3", "4", "6", "-1", "m", "-3", "-4", "-6")
_TYPE_OF = {(1, 3): 0, (1, -1): 1, (1, 0): 2, (1, 1): 3, (1, 2): 4, (-1, -3): 5, (-1, 1): 6, (-1, 0): 7, (-1, -1): 8, (-1, -2): 9}
CRYSTAL_SYSTEMS = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "trigonal", "hexagonal", "cubic")
# (name, crystal system, generators): id = position.  Trigonal and hexagonal groups in hexagonal axes, monoclinic b-unique.
POINT_GROUPS = (
    ("1", "triclinic", ("x,y,z",)),
    ("-1", "triclinic", ("-x,-y,-z",)),
    ("2", "monoclinic", ("-x,y,-z",)),
    ("m", "monoclinic", ("x,-y,z",)),
    ("2/m", "monoclinic", ("-x,y,-z", "-x,-y,-z")),
    ("222", "orthorhombic", ("-x,-y,z", "-x,y,-z")),
    ("mm2", "orthorhombic", ("-x,-y,z", "x,-y,z")),
    ("mmm", "orthorhombic", ("-x,-y,z", "-x,y,-z", "-x,-y,-z")),
    ("4", "tetragonal", ("-y,x,z",)),
    ("-4", "tetragonal", ("y,-x,-z",)),
    ("4/m", "tetragonal", ("-y,x,z", "-x,-y,-z")),
    ("422", "tetragonal", ("-y,x,z", "-x,y,-z")),
    ("4mm", "tetragonal", ("-y,x,z", "x,-y,z")),
    ("-42m", "tetragonal", ("y,-x,-z", "-x,y,-z")),
    ("4/mmm", "tetragonal", ("-y,x,z", "-x,y,-z", "-x,-y,-z")),
    ("3", "trigonal", ("-y,x-y,z",)),
    ("-3", "trigonal", ("-y,x-y,z", "-x,-y,-z")),
    ("32", "trigonal", ("-y,x-y,z", "y,x,-z")),
    ("3m", "trigonal", ("-y,x-y,z", "-y,-x,z")),
    ("-3m", "trigonal", ("-y,x-y,z", "y,x,-z", "-x,-y,-z")),
    ("6", "hexagonal", ("x-y,x,z",)),
    ("-6", "hexagonal", ("-x+y,-x,-z",)),
    ("6/m", "hexagonal", ("x-y,x,z", "-x,-y,-z")),
    ("622", "hexagonal", ("x-y,x,z", "y,x,-z")),
    ("6mm", "hexagonal", ("x-y,x,z", "-y,-x,z")),
    ("-6m2", "hexagonal", ("-x+y,-x,-z", "-y,-x,z")),
    ("6/mmm", "hexagonal", ("x-y,x,z", "y,x,-z", "-x,-y,-z")),
    ("23", "cubic", ("-x,-y,z", "-x,y,-z", "z,x,y")),
    ("m-3", "cubic", ("-x,-y,z", "-x,y,-z", "z,x,y", "-x,-y,-z")),
    ("432", "cubic", ("-y,x,z", "z,x,y")),
    ("-43m", "cubic", ("y,-x,-z", "z,x,y")),
    ("m-3m", "cubic", ("-y,x,z", "z,x,y", "-x,-y,-z")),
)
POINT_GROUP_NAMES = tuple(name for name, _, _ in POINT_GROUPS)
POINT_GROUP_SYSTEMS = tuple(system for _, system, _ in POINT_GROUPS)


def rotation_type(W) -> int:
    """The index into ROTATION_TYPES of an integer matrix of finite order (from det and trace), or -1 when it has none."""
    W = np.asarray(W)
    return _TYPE_OF.get((int(round(np.linalg.det(W))), int(np.trace(W))), -1)


def type_counts(rotations):
    """The count vector [10] of a set of rotation matrices (rule 6)."""
    counts = np.zeros(len(ROTATION_TYPES), dtype=np.int64)
    for W in rotations:
        k = rotation_type(W)
        if k < 0:
            return None
        counts[k] += 1
    return counts


def point_group_table():
    """The 32 count vectors [32,10], each closed from its group's generators (symmetry.close_group): never typed in."""
    return np.stack([type_counts([R for R, _ in sym_mod.close_group(gens)]) for _, _, gens in POINT_GROUPS])


_TABLE = None


def classify_counts(counts) -> int:
    """The id of the point group with this count vector, or -1."""
    global _TABLE
    if _TABLE is None:
        _TABLE = point_group_table()
    if counts is None:
        return -1
    hit = np.nonzero((_TABLE == np.asarray(counts)[None, :]).all(axis=1))[0]
    return int(hit[0]) if hit.size else -1


def classify(rotations, n_ops=None, n_translations=1):
    """(point group id, flags) of the distinct rotations of a found set (rule 6): -1 and NOT_A_GROUP when their counts match no
    row or n_ops != distinct rotations x n_translations."""
    rotations = list(rotations)
    pg = classify_counts(type_counts(rotations))
    if n_ops is not None and int(n_ops) != len(rotations) * int(n_translations):
        pg = -1
    return pg, (NOT_A_GROUP if pg < 0 else 0)


def crystal_system(point_group) -> str:
    """'cubic' for 31; 'none' for -1."""
    return POINT_GROUP_SYSTEMS[int(point_group)] if int(point_group) >= 0 else "none"


def point_group_name(point_group) -> str:
    return POINT_GROUP_NAMES[int(point_group)] if int(point_group) >= 0 else "none"


def encode_rotation(W) -> int:
    """The base-3 code of an integer matrix with entries in {-1, 0, 1}: sum (W_rc + 1) 3^(3r + c)."""
    W = np.asarray(W)
    if W.shape != (3, 3) or not np.isin(W, (-1, 0, 1)).all():
        raise ValueError("a rotation code holds a 3 x 3 matrix with entries in {-1, 0, 1}")
    return int(((W.reshape(-1).astype(np.int64) + 1) * 3 ** np.arange(9)).sum())


def decode_rotation(code) -> np.ndarray:
    """The int64 [3,3] matrix of a rotation code (the inverse of encode_rotation)."""
    if isinstance(code, bool) or not isinstance(code, Integral) or not 0 <= int(code) < N_CODES:
        raise ValueError(f"a rotation code lies in 0..{N_CODES - 1}, got {code!r}")
    return ((int(code) // 3 ** np.arange(9)) % 3 - 1).astype(np.int64).reshape(3, 3)


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class SymmetrySearchParams:
    """symprec: the tolerance in A on cell lengths and on the distance between an atom's image and its partner (0.1 is what CDVAE
    and MatterGen evaluate with: a starting value, not a claim).  max_ops: the operations stored per crystal (1..4096); n_ops
    counts them all."""
    symprec: float = DEFAULT_SYMPREC
    max_ops: int = DEFAULT_MAX_OPS

    def __post_init__(self):
        v = self.symprec
        if not isinstance(v, Real) or isinstance(v, bool) or not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"symprec must be a finite number > 0, got {v!r}")
        object.__setattr__(self, "symprec", float(v))
        v = self.max_ops
        if not isinstance(v, Integral) or isinstance(v, bool) or not 1 <= int(v) <= MAX_OPS_CAP:
            raise ValueError(f"max_ops must lie in 1..{MAX_OPS_CAP}, got {v!r}")
        object.__setattr__(self, "max_ops", int(v))


def resolve(find_symmetry):
    """sample(find_symmetry=...): None / False -> None, True -> the defaults, a SymmetrySearchParams -> itself."""
    return cb.resolve(find_symmetry, SymmetrySearchParams, "find_symmetry")


# ------------------------------------------------------------------------------------------------------- the device call
def find_symmetry(frac, lattice, offsets, types, params=None):
    """Search a batch on the GPU without an engine (arreau_crystal_symmetry, one launch).  frac [N,3] float32, lattice [B,3,3]
    float32 (rows a, b, c), offsets [B+1] int32 and types [N] int32 (species ids) are contiguous tensors on one cuda device.
    Returns a dict of device tensors: n_lattice, n_ops, n_translations, residual, point_group, flags, symprec [B];
    ops_rotation [B,max_ops] (codes, -1 beyond the stored ones), ops_translation [B,max_ops,3], ops_residual [B,max_ops]; and
    `lattice` (the input, for `contains`).  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else SymmetrySearchParams()
    dev, B, N = cb.check_batch("find_symmetry", frac, lattice, offsets, types)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    M = p.max_ops
    out = {"n_lattice": torch.empty(B, **i32), "n_ops": torch.empty(B, **i32), "n_translations": torch.empty(B, **i32),
           "ops_rotation": torch.empty((B, M), **i32), "ops_translation": torch.empty((B, M, 3), **f32),
           "ops_residual": torch.empty((B, M), **f32), "residual": torch.empty(B, **f32), "point_group": torch.empty(B, **i32),
           "flags": torch.empty(B, **i32)}
    c = _hip.SymmetryParamsC(p.symprec, p.max_ops)
    r = _hip.SymmetryResultC(*[_hip.ptr(out[k]).value if B else None for k in SYM_KEYS[:-1]])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_symmetry(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(offsets), B, N,
                                                      ctypes.byref(c), ctypes.byref(r), _hip.stream_ptr(dev)),
                   "arreau_crystal_symmetry")
    out["symprec"] = torch.full((B,), float(F32(p.symprec)), **f32)
    out["lattice"] = lattice
    return out


def result_to_numpy(result):
    """The dict of `find_symmetry` as host numpy arrays (synchronises)."""
    return cb.to_numpy(result)


def symmetry_sample_result(result, params=None, device="cuda"):
    """The symmetry of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32 and its atomic
    numbers taken as species ids: the dict of `find_symmetry` as numpy arrays."""
    return result_to_numpy(find_symmetry(*cb.upload(result, device), params))


# ------------------------------------------------------------------------------------------------------------- contains
def _wrap_nearest(d):
    return d - np.rint(d)


def group_operations(spec_or_ops):
    """The closed group [(R, t)] of a SymmetrySpec, of generators in xyz form or of (R, t) pairs."""
    if isinstance(spec_or_ops, sym_mod.SymmetrySpec):
        return list(spec_or_ops.ops)
    return sym_mod.close_group(list(spec_or_ops))


def contains(result, b, spec_or_ops) -> bool:
    """True when every operation of the closed group of `spec_or_ops` (a symmetry.SymmetrySpec, generators in xyz form or (R, t)
    pairs) is among the stored operations of crystal b: equal rotation, and a translation within symprec in A after wrapping
    the difference to the nearest lattice vector.  `result`: the numpy dict of a search (it holds `lattice` and `symprec`)."""
    b = int(b)
    stored = min(int(result["n_ops"][b]), int(np.asarray(result["ops_rotation"]).shape[1]))
    codes = np.asarray(result["ops_rotation"][b][:stored])
    trans = np.asarray(result["ops_translation"][b][:stored], dtype=np.float64)
    L = np.asarray(result["lattice"][b], dtype=np.float64).reshape(3, 3)
    symprec = float(np.asarray(result["symprec"]).reshape(-1)[b])
    for R, t in group_operations(spec_or_ops):
        if not np.isin(R, (-1, 0, 1)).all():
            return False
        rows = np.nonzero(codes == encode_rotation(R))[0]
        if not rows.size:
            return False
        d = np.linalg.norm(_wrap_nearest(trans[rows] - np.asarray(t, dtype=np.float64)[None, :]) @ L, axis=1)
        if not (d <= symprec).any():
            return False
    return True


def operation_residuals(frac, lattice, types, ops):
    """Rule 4 in float64 for given operations [(R, t)] on one crystal: the residual of each (max over atoms of the distance to
    the nearest atom of the same species), in A."""
    f = np.asarray(frac, dtype=np.float64).reshape(-1, 3)
    L = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    ty = np.asarray(types).reshape(-1)
    other = ty[:, None] != ty[None, :]
    out = []
    for R, t in ops:
        y = f @ np.asarray(R, dtype=np.float64).T + np.asarray(t, dtype=np.float64)
        d = np.linalg.norm(_wrap_nearest(y[:, None, :] - f[None, :, :]) @ L, axis=2)
        d[other] = np.inf
        out.append(d.min(axis=1).max())
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the count per crystal system, per point group
    and per flag."""
    pg = np.asarray(result["point_group"], dtype=np.int64).reshape(-1)
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    groups = {name: int((pg == k).sum()) for k, name in enumerate(POINT_GROUP_NAMES)}
    systems = {s: 0 for s in CRYSTAL_SYSTEMS}
    for k, name in enumerate(POINT_GROUP_NAMES):
        systems[POINT_GROUP_SYSTEMS[k]] += groups[name]
    return {"rank": cb.rank_of(rank), "attempted": int(pg.size), "classified": int((pg >= 0).sum()),
            "systems": systems, "point_groups": groups, "flags": cb.flag_counts(flags, FLAG_NAMES)}


def total_stats(parts):
    add = lambda key, names: {n: sum(p[key][n] for p in parts) for n in names}
    return {"rank": "total", "attempted": sum(p["attempted"] for p in parts), "classified": sum(p["classified"] for p in parts),
            "systems": add("systems", CRYSTAL_SYSTEMS), "point_groups": add("point_groups", POINT_GROUP_NAMES),
            "flags": add("flags", [n for _, n in FLAG_NAMES])}


def format_stats(st) -> str:
    """'symmetry rank 0: classified 16 / attempted 16; triclinic 14, cubic 2; point groups 1: 13, -1: 1, m-3m: 2; flags none'."""
    return f"symmetry {cb.who(st)}: classified {st['classified']} / attempted {st['attempted']}; {cb.some(st['systems'])}; " \
           f"point groups {cb.some(st['point_groups'], ': ')}; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


def contains_line(result, spec_or_ops) -> str:
    """'symmetry: 14 / 16 crystals contain the requested group (|G| = 16)'."""
    ops = group_operations(spec_or_ops)
    B = int(np.asarray(result["flags"]).shape[0])
    return f"symmetry: {sum(contains(result, b, ops) for b in range(B))} / {B} crystals contain the requested group (|G| = {len(ops)})"


# -------------------------------------------------------------------------------------------------- the numpy restatement
_ALL_W = None


def _all_candidates():
    """(codes [M], W [M,3,3] int64) of every matrix with entries in {-1, 0, 1} and det +-1, in code order."""
    global _ALL_W
    if _ALL_W is None:
        codes = np.arange(N_CODES)
        W = ((codes[:, None] // 3 ** np.arange(9)[None, :]) % 3 - 1).reshape(-1, 3, 3).astype(np.int64)
        det = (W[:, 0, 0] * (W[:, 1, 1] * W[:, 2, 2] - W[:, 1, 2] * W[:, 2, 1]) - W[:, 0, 1] * (W[:, 1, 0] * W[:, 2, 2] - W[:, 1, 2] * W[:, 2, 0])
               + W[:, 0, 2] * (W[:, 1, 0] * W[:, 2, 1] - W[:, 1, 1] * W[:, 2, 0]))
        keep = np.abs(det) == 1
        _ALL_W = (codes[keep], W[keep])
    return _ALL_W


def lattice_deviations(L):
    """Rule 2 in float64 for one cell [3,3]: (codes [M], W [M,3,3], dev [M]) over every candidate of det +-1, dev the largest of
    | |a'_i| - |a_i| | and |G'_ij - G_ij| / ((|a_i| + |a_j|) / 2), i < j: the candidate passes when dev <= symprec."""
    codes, W = _all_candidates()
    L = np.asarray(L, dtype=np.float64).reshape(3, 3)
    G = L @ L.T
    img = np.einsum("mkj,kd->mjd", W.astype(np.float64), L)  # a'_j = sum_k W_kj a_k
    Gi = np.einsum("mid,mjd->mij", img, img)
    ln = np.sqrt(np.diag(G))
    dev = np.abs(np.sqrt(Gi[:, [0, 1, 2], [0, 1, 2]]) - ln[None, :]).max(axis=1)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        dev = np.maximum(dev, np.abs(Gi[:, i, j] - G[i, j]) / ((ln[i] + ln[j]) / 2.0))
    return codes, W, dev


def residual_bound(lattice):
    """The derived bound on |residual_float32 - residual_exact| of one crystal (module docstring): 64 * 2^-24 * max_d sum_k |L_kd|."""
    return RESIDUAL_BOUND_FACTOR * 2.0 ** -24 * float(np.abs(np.asarray(lattice, dtype=np.float64).reshape(3, 3)).sum(axis=0).max())


def _wrap01(v):
    w = v - np.floor(v)
    w[w >= 1.0] = 0.0
    return w


def symmetry_reference_f64(frac, lattice, counts, types, params=None, details=False):
    """Rules 1-6 in float64 from the same float32 inputs: frac [N,3], lattice [B,3,3], counts [B] atoms per crystal, types [N].
    Returns a namespace of the nine outputs (the reals float64).  details=True adds, per crystal, `lattice_dev` (the deviation
    of every candidate of det +-1) and `all_residuals` (the residual of every (W, t) the search evaluates): what the guard of
    the test cases looks at."""
    p = params if params is not None else SymmetrySearchParams()
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    assert frac.shape[0] == types.shape[0]
    B, M, symprec = len(counts), p.max_ops, float(F32(p.symprec))
    out = SimpleNamespace(n_lattice=np.zeros(B, np.int32), n_ops=np.zeros(B, np.int32), n_translations=np.zeros(B, np.int32),
                          ops_rotation=np.full((B, M), -1, np.int32), ops_translation=np.zeros((B, M, 3)), ops_residual=np.zeros((B, M)),
                          residual=np.full(B, np.nan), point_group=np.full(B, -1, np.int32), flags=np.zeros(B, np.int32),
                          lattice_dev=[None] * B, all_residuals=[None] * B)
    for b, n in enumerate(counts):
        L, f, ty = lattice[b].astype(np.float64), frac[first[b]:first[b + 1]].astype(np.float64), types[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        vol = abs(float(np.dot(L[0], np.cross(L[1], L[2]))))
        if not vol > 0.0 or not np.isfinite(vol):
            out.flags[b] |= CELL
        if n == 0:
            out.flags[b] |= EMPTY
        if out.flags[b]:
            continue
        codes, W, dev = lattice_deviations(L)
        out.lattice_dev[b] = dev
        keep = dev <= symprec
        out.n_lattice[b] = int(keep.sum())
        if keep.sum() > MAX_LATTICE:
            out.flags[b] |= AMBIGUOUS
            continue
        w = _wrap01(f)
        species, cnt = np.unique(ty, return_counts=True)
        rare = species[int(np.argmin(cnt))]  # the fewest atoms, the smallest id on ties
        qs = np.nonzero(ty == rare)[0]
        other = ty[:, None] != ty[None, :]
        n_ops, worst, residuals, distinct = 0, 0.0, [], []
        for code, Wm in zip(codes[keep], W[keep].astype(np.float64)):
            Ww = w @ Wm.T
            t = _wrap01(w[qs] - Ww[qs[0]][None, :])  # [Q,3]
            res = np.empty(len(qs))
            step = max(1, (1 << 22) // max(1, n * n))
            for a in range(0, len(qs), step):
                delta = (Ww[None, :, None, :] + t[a:a + step, None, None, :]) - w[None, None, :, :]  # [q, i, j, 3]
                d = np.linalg.norm(_wrap_nearest(delta) @ L, axis=3)
                d[:, other] = np.inf
                res[a:a + step] = d.min(axis=2).max(axis=1)
            residuals.append(res)
            acc = np.nonzero(res <= symprec)[0]
            if acc.size:
                distinct.append(np.rint(Wm).astype(np.int64))
                if int(code) == IDENTITY_CODE:
                    out.n_translations[b] = acc.size
                worst = max(worst, float(res[acc].max()))
            for k in acc:
                if n_ops < M:
                    out.ops_rotation[b, n_ops], out.ops_translation[b, n_ops], out.ops_residual[b, n_ops] = int(code), t[k], res[k]
                n_ops += 1
        out.all_residuals[b] = np.concatenate(residuals) if residuals else np.empty(0)
        out.n_ops[b], out.residual[b] = n_ops, worst
        if n_ops > M:
            out.flags[b] |= OVERFLOW
        pg, flag = classify(distinct, n_ops, out.n_translations[b])
        out.point_group[b] = pg
        out.flags[b] |= flag
    if not details:
        del out.lattice_dev, out.all_residuals
    return out
