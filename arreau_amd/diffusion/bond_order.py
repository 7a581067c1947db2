"""Bond angles and Steinhardt order parameters of generated crystals: per atom the histogram of the angles between its bonds and
the bond-orientational order parameters q_2, q_4, q_6, q_8 of its neighbour shell, per crystal the summed histogram and the mean
q_l (arreau_crystal_bond_order, arreau_amd/csrc/bond_order.hip; the rules are written out in include/arreau_hip.h).  What a
coordination number cannot tell: an octahedron from a trigonal prism, fcc from hcp from an icosahedral shell (all 12), a
tetrahedral 4 from a square-planar 4.  Here: the parameters, the constants, the entry points that need no engine (`bond_order`:
the coordination launch, then the new one; `from_coordination`: the new one on a coordination result; `from_voronoi`: on a
Voronoi result's faces), the statistics and two numpy
restatements for the tests -- `bond_order_reference_f32`, one float32 operation at a time in the kernel's order, sums and butterfly
included (the bit-for-bit yardstick), and `bond_order_reference_f64`, the same lists in float64, which also returns the margin of
every pair's cosine to the nearest histogram edge.  Needs numpy alone at import.

The shell is the coordination rule's (coordination.py): every atom and image within (1 + tol) times the atom's nearest distance and
within the cutoff; of it the first max_neighbors entries in (j, image) order.  For a shell of m unit bond vectors u_e (Steinhardt,
Nelson & Ronchetti 1983, and the addition theorem of the spherical harmonics)
    q_l^2 = (4 pi / (2l+1)) sum_mm |mean_e Y_lmm(u_e)|^2 = (1 / m^2) sum_{e,f} P_l(u_e . u_f) = (m + 2 sum_{e<f} P_l(c_ef)) / m^2,
so the pairs e < f of an atom's bonds give the angle histogram (37 bins centred on 0, 5, ..., 180 degrees) and every q_l from
Legendre polynomials alone.  Not here: w_l (third-order invariants need the q_lm), neighbour-averaged (Lechner-Dellago)
parameters, a classification of environments or polyhedra, Voronoi weights.

Derived float32 bounds (u = 2^-24; screening.py's docstring derives, for the same arithmetic, |d disp_d| <= 11 u G per component
and |d_f32 - d_exact| <= 26.1 u G, G = max_d sum_k (1 + n_k) |L_kd| with n_k the largest image index of the list on axis k).
  * the unit vector u_d = disp_d / d: |du_d| <= (11 u G + |u_d| 26.1 u G) / d + u |u_d| <= 37.1 u G / d + u;
  * the cosine c = u . u': sum_d (|u_d| |du'_d| + |u'_d| |du_d|) <= 2 sqrt(3) (37.1 u G / d_min + u), and the dot product's three
    products and two sums add at most 3 u: |c_f32 - c_exact| <= 128.5 u G / d_min + 7 u, d_min the crystal's shortest bond.
    C_BOUND_FACTOR = 160 leaves the margin of screening.py's 32 over 26.1: c_bound = 160 u G / d_min + 8 u.  The clamp to [-1, 1]
    moves no value away from the exact one.  cos_min and cos_max are extremes of such values: the same bound.
  * P_l(c): |P_l'| <= l (l + 1) / 2 on [-1, 1], so the error of c enters with at most that factor; a step of the recurrence
    P_{k+1} = a_k (c P_k) - b_k P_{k-1} adds at most 10 u of its own (the roundings of a_k and b_k, two products of values up to
    2, one of a value up to 1, the difference; |P| <= 1) and carries the earlier errors with |a_k| and |b_k|: E_{k+1} = a_k E_k +
    b_k E_{k-1} + 10 u from E_0 = E_1 = 0 (`legendre_rounding_bound`: 10 u, 64 u, 333 u, 1714 u for l = 2, 4, 6, 8).
  * q2_l = (m + 2 S_l) / m^2 is a mean of such terms: the pairs' errors enter with (m - 1) / m < 1; every term passes through at
    most 63 + 6 additions of partial sums no larger than the sum of the absolute terms, 69 u after the division; the three final
    operations add 3 u: q2_bound = (l (l + 1) / 2) c_bound + legendre_rounding_bound(l) + 80 u.
An atom is GUARDED when the smallest margin of its pairs' cosines to a histogram edge exceeds FOUR c_bound (two sides, and a
factor two to spare): float32 puts every pair into the bin float64 does.  A degenerate atom (a bond of length 0) has no bound."""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import coordination as co
from . import crystal_batch as cb
from . import screening

NONFINITE, EMPTY, BAD_LIST, OVERLAP, ISOLATED, TRUNCATED = 1, 2, 4, 8, 16, 32
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (EMPTY, "EMPTY"), (BAD_LIST, "BAD_LIST"), (OVERLAP, "OVERLAP"), (ISOLATED, "ISOLATED"),
              (TRUNCATED, "TRUNCATED"))
FLAGS = FLAG_NAMES
BLANK = NONFINITE | BAD_LIST  # nothing was computed for the crystal's atoms
L_VALUES = (2, 4, 6, 8)
ANGLE_BINS = 37
F32 = np.float32
# E_k = float32(cos((k + 1/2) 5 degrees)), formed in double: bin(c) = #{k : c <= E_k}
COS_EDGES = np.cos((np.arange(ANGLE_BINS - 1, dtype=np.float64) + 0.5) * 5.0 * np.pi / 180.0).astype(F32)
CRYSTAL_KEYS = ("mean_q", "n_angles", "angle_hist", "flags")  # one row per crystal
RESULT_KEYS = CRYSTAL_KEYS + ("n_used", "q", "q2", "cos_min", "cos_max", "angles")  # arreau_bond_order_result, in its order
ATOM_KEYS = ("n_used", "q", "q2", "cos_min", "cos_max", "angles", "species")  # one row per atom; species: the atomic numbers
STORED_KEYS = CRYSTAL_KEYS + ("coord_flags",) + ATOM_KEYS  # what SampleResult.bond_order and a crystals file hold
C_BOUND_FACTOR = 160.0
U = 2.0 ** -24


def angle_centres():
    """The centres of the 37 angle bins in degrees: 0, 5, ..., 180."""
    return 5.0 * np.arange(ANGLE_BINS, dtype=np.float64)


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class BondOrderParams:
    """The coordination search's parameters (coordination.CoordinationParams, which validates them): the shell of an atom is
    what that search finds with them, and of it the first max_neighbors entries."""
    tol: float = 0.1
    cutoff: float = 6.0
    max_neighbors: int = 24
    max_shells: int = co.MAX_SHELLS

    def __post_init__(self):
        c = co.CoordinationParams(self.tol, self.cutoff, self.max_neighbors, self.max_shells)
        for name in ("tol", "cutoff", "max_neighbors", "max_shells"):
            object.__setattr__(self, name, getattr(c, name))

    def coordination(self):
        return co.CoordinationParams(self.tol, self.cutoff, self.max_neighbors, self.max_shells)


def resolve(bond_order):
    """sample(bond_order=...): None / False -> None, True -> the defaults, a BondOrderParams -> itself."""
    return cb.resolve(bond_order, BondOrderParams, "bond_order")


def check_shared(bond_order, coordination):
    """sample(bond_order=..., coordination=...) share the coordination launch: their parameters must agree."""
    if bond_order is not None and coordination is not None and bond_order.coordination() != coordination:
        raise ValueError(f"bond_order and coordination share one search: their parameters must agree, got {bond_order} and {coordination}")


# ------------------------------------------------------------------------------------------------------- the device calls
def from_coordination(frac, lattice, offsets, coordination_result, max_neighbors=None):
    """The bond angles and order parameters of a batch on the GPU from a device coordination result (the dict of
    coordination.coordination: its cn [N] and neighbors [N, max_neighbors, 4] are read; any int32 list in that layout serves):
    arreau_crystal_bond_order, one launch.  Returns a dict of device tensors (RESULT_KEYS): mean_q [B,4], n_angles [B], angle_hist
    [B,37], flags [B]; n_used [N], q and q2 [N,4] (l = 2, 4, 6, 8), cos_min and cos_max [N], angles [N,37]; and coord_flags, the
    search's own flags (None when the result carries none).  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    dev, B, N = cb.check_batch("bond_order", frac, lattice, offsets, None, types_optional=True)
    cn, nb = coordination_result["cn"], coordination_result["neighbors"]
    width = int(nb.shape[1]) if nb.dim() == 3 else -1
    if max_neighbors is None:
        max_neighbors = width
    for name, t, shape in (("cn", cn, (N,)), ("neighbors", nb, (N, int(max_neighbors), 4))):
        if tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"bond_order: {name} must be a contiguous int32 tensor of shape {shape} on the cuda device of frac")
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    nl = len(L_VALUES)
    out = {"mean_q": torch.empty((B, nl), **f32), "n_angles": torch.empty(B, **i32), "angle_hist": torch.empty((B, ANGLE_BINS), **i32),
           "flags": torch.empty(B, **i32), "n_used": torch.empty(N, **i32), "q": torch.empty((N, nl), **f32), "q2": torch.empty((N, nl), **f32),
           "cos_min": torch.empty(N, **f32), "cos_max": torch.empty(N, **f32), "angles": torch.empty((N, ANGLE_BINS), **i32)}
    c = _hip.BondOrderParamsC(int(max_neighbors), (ctypes.c_float * (ANGLE_BINS - 1))(*[float(e) for e in COS_EDGES]))
    r = _hip.BondOrderResultC(*[_hip.ptr(out[k]).value if out[k].numel() else None for k in RESULT_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_bond_order(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(offsets), B, N,
                                                        _hip.ptr(cn) if N else None, _hip.ptr(nb) if N else None, ctypes.byref(c),
                                                        ctypes.byref(r), _hip.stream_ptr(dev)), "arreau_crystal_bond_order")
    out["coord_flags"] = coordination_result.get("flags")
    return out


def from_voronoi(frac, lattice, offsets, voronoi_result, max_faces=None):
    """The same on Voronoi shells: the twin of `from_coordination` for a device Voronoi result (the dict of voronoi.voronoi), whose
    cn [N] and neighbors [N, max_faces, 4] have the coordination result's layout -- the shell of an atom is then the faces of
    weight >= tol of its Voronoi cell, of them the first max_faces.  The existing launch, no new kernel.  coord_flags is None:
    the Voronoi flags have their own bits (voronoi.FLAG_NAMES) and stay in the Voronoi result."""
    return from_coordination(frac, lattice, offsets, {"cn": voronoi_result["cn"], "neighbors": voronoi_result["neighbors"]}, max_faces)


def bond_order(frac, lattice, offsets, params=None):
    """The same without an engine from the crystals alone: the coordination launch with `params`, then the new one.  frac [N,3]
    float32, lattice [B,3,3] float32 (rows a, b, c) and offsets [B+1] int32 are contiguous tensors on one cuda device."""
    p = params if params is not None else BondOrderParams()
    return from_coordination(frac, lattice, offsets, co.coordination(frac, lattice, offsets, p.coordination()), p.max_neighbors)


def result_to_numpy(result):
    """The dict of `bond_order` / `from_coordination` as host numpy arrays (synchronises)."""
    return cb.to_numpy({k: v for k, v in result.items() if v is not None})


def sample_arrays(result, atomic_numbers):
    """What SampleResult.bond_order and a crystals file hold (STORED_KEYS) of a `result_to_numpy` dict: its arrays, the search's
    flags and `species`, the atomic numbers of the atoms (what the mean per element is taken over)."""
    out = {k: np.asarray(result[k]) for k in STORED_KEYS if k != "species"}
    out["species"] = np.rint(np.asarray(atomic_numbers, dtype=np.float64).reshape(-1)).astype(np.int64)
    if out["species"].shape != out["n_used"].shape:
        raise ValueError("bond_order: one atomic number per atom is needed")
    return out


def bond_order_sample_result(result, params=None, device="cuda"):
    """The bond angles and order parameters of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to
    float32: the dict of `sample_arrays`."""
    frac, lattice, off, _ = cb.upload(result, device)
    return sample_arrays(result_to_numpy(bond_order(frac, lattice, off, params)), result.atomic_numbers)


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the summed angle histogram as its non-empty bins
    {degrees: pairs}, the atoms with finite q and their summed q4 and q6, overall and per element (`species` given), the count
    per flag.  The atoms of the crystals nothing was computed for (NONFINITE, BAD_LIST; for the search NONFINITE, CELL) are left
    out."""
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    hist = np.asarray(result["angle_hist"], dtype=np.int64).reshape(-1, ANGLE_BINS)
    q = np.asarray(result["q"], dtype=np.float64).reshape(-1, len(L_VALUES))
    done_c = (flags & BLANK) == 0
    if result.get("coord_flags") is not None:
        done_c &= (np.asarray(result["coord_flags"], dtype=np.int64).reshape(-1) & (co.NONFINITE | co.CELL)) == 0
    total = hist[done_c].sum(axis=0)
    fin = np.isfinite(q).all(axis=1)
    i4, i6 = L_VALUES.index(4), L_VALUES.index(6)
    out = {"rank": cb.rank_of(rank), "crystals": int(flags.size), "computed": int(done_c.sum()), "atoms": int(fin.sum()),
           "n_angles": int(total.sum()), "angles": {int(5 * k): int(v) for k, v in enumerate(total) if v},
           "q4": float(q[fin, i4].sum()), "q6": float(q[fin, i6].sum()), "elements": {}, "flags": cb.flag_counts(flags, FLAG_NAMES)}
    if result.get("species") is not None:
        z = np.asarray(result["species"], dtype=np.int64).reshape(-1)
        out["elements"] = {int(v): [int(((z == v) & fin).sum()), float(q[(z == v) & fin, i4].sum()), float(q[(z == v) & fin, i6].sum())]
                           for v in np.unique(z[fin])}
    return out


def total_stats(parts):
    angles, elements = {}, {}
    for p in parts:
        for k, v in p["angles"].items():
            angles[int(k)] = angles.get(int(k), 0) + v
        for k, (a, s4, s6) in p["elements"].items():
            have = elements.get(int(k), [0, 0.0, 0.0])
            elements[int(k)] = [have[0] + a, have[1] + s4, have[2] + s6]
    return {"rank": "total", "crystals": sum(p["crystals"] for p in parts), "computed": sum(p["computed"] for p in parts),
            "atoms": sum(p["atoms"] for p in parts), "n_angles": sum(p["n_angles"] for p in parts), "angles": dict(sorted(angles.items())),
            "q4": sum(p["q4"] for p in parts), "q6": sum(p["q6"] for p in parts), "elements": dict(sorted(elements.items())),
            "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'bond order rank 0: 16 crystals, 320 atoms; angles 60: 24, 90: 12 (36 pairs); mean q4 0.191, q6 0.575 (Z 11: 0.191 /
    0.575); flags ISOLATED 1'."""
    hist = cb.some(dict(sorted((int(k), v) for k, v in st["angles"].items())), ": ")
    mean = f"q4 {st['q4'] / st['atoms']:.3f}, q6 {st['q6'] / st['atoms']:.3f}" if st["atoms"] else "q4 n/a, q6 n/a"
    per = ", ".join(f"Z {int(k)}: {s4 / a:.3f} / {s6 / a:.3f}" for k, (a, s4, s6) in sorted((int(k), v) for k, v in st["elements"].items()) if a)
    return f"bond order {cb.who(st)}: {st['crystals']} crystals, {st['atoms']} atoms; angles {hist} ({st['n_angles']} pairs); mean {mean}" + \
        (f" ({per})" if per else "") + f"; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------- the numpy restatements
def legendre_coefficients(dtype=F32):
    """(a_k, b_k), k = 1..7, of P_{k+1} = a_k (c P_k) - b_k P_{k-1}: (2k+1)/(k+1) and k/(k+1) formed in double, rounded to dtype."""
    k = np.arange(1, L_VALUES[-1], dtype=np.float64)
    return ((2.0 * k + 1.0) / (k + 1.0)).astype(dtype), (k / (k + 1.0)).astype(dtype)


def _legendre(c, dtype):
    """P_l(c), l in L_VALUES, of an array c by the recurrence, every operation rounded to dtype, in the kernel's order: [4, ...]."""
    a, b = legendre_coefficients(dtype)
    pm, pk, out = np.ones_like(c), c, []
    for k in range(1, L_VALUES[-1]):
        t = (c * pk).astype(dtype)
        t = (a[k - 1] * t).astype(dtype)
        s = (b[k - 1] * pm).astype(dtype)
        pm, pk = pk, (t - s).astype(dtype)
        if k + 1 in L_VALUES:
            out.append(pk)
    return np.stack(out)


_XOR = [np.arange(64) ^ w for w in (32, 16, 8, 4, 2, 1)]


def lane_sum(v):
    """The kernel's lane sum of 64 float32 lane values (leading axis): v <- v + shuffle_xor(v, w), w = 32 .. 1; lane 0's value."""
    v = np.asarray(v, dtype=F32)
    for idx in _XOR:
        v = (v + v[idx]).astype(F32)
    return v[0]


def _lane_extreme(v, less):
    for idx in _XOR:
        o = v[idx]
        v = np.where(less(o, v), o, v)
    return v[0]


def _empty_result(B, N, real):
    nl = len(L_VALUES)
    return SimpleNamespace(mean_q=np.full((B, nl), np.nan, real), n_angles=np.zeros(B, np.int32), angle_hist=np.zeros((B, ANGLE_BINS), np.int32),
                           flags=np.zeros(B, np.int32), n_used=np.zeros(N, np.int32), q=np.full((N, nl), np.nan, real),
                           q2=np.full((N, nl), np.nan, real), cos_min=np.full(N, np.nan, real), cos_max=np.full(N, np.nan, real),
                           angles=np.zeros((N, ANGLE_BINS), np.int32))


def _lists(cn, neighbors, N):
    cn = np.asarray(cn, dtype=np.int64).reshape(-1)
    neighbors = np.asarray(neighbors, dtype=np.int64)
    assert cn.shape == (N,) and neighbors.ndim == 3 and neighbors.shape[0] == N and neighbors.shape[2] == 4
    return cn, neighbors, neighbors.shape[1]


def _list_is_bad(cn, nb, n, max_nb):
    """Rule 2 of one crystal: some cn < 0, or a j outside 0..n-1 among an atom's first min(cn, max_neighbors) entries."""
    if (cn < 0).any():
        return True
    used = np.arange(max_nb)[None, :] < np.minimum(cn, max_nb)[:, None]
    j = nb[:, :, 0]
    return bool((used & ((j < 0) | (j >= n))).any())


def _bonds(p, L, i, entries, dtype):
    """Rule 3 for atom i: (disp [m,3], d2 [m]) of its entries [m,4], every operation rounded to dtype in the rule's order."""
    nv = entries[:, 1:].astype(dtype)
    s = ((nv[:, 0:1] * L[0][None] + nv[:, 1:2] * L[1][None]).astype(dtype) + nv[:, 2:3] * L[2][None]).astype(dtype)
    disp = ((p[entries[:, 0]] + s).astype(dtype) - p[i][None]).astype(dtype)
    sq = (disp * disp).astype(dtype)
    return disp, ((sq[:, 0] + sq[:, 1]).astype(dtype) + sq[:, 2]).astype(dtype)


def _bins(c, edges):
    return (c[:, None] <= edges[None, :]).sum(axis=1)


def bond_order_reference_f32(frac, lattice, counts, cn, neighbors):
    """The kernel's rules 1-9 in numpy float32, one operation at a time in the kernel's order (numpy never contracts to an FMA),
    the per-lane sums, the butterfly and the comparisons of the extremes included: frac [N,3], lattice [B,3,3], counts [B] atoms
    per crystal, cn [N] and neighbors [N, max_neighbors, 4] a coordination result's arrays.  Returns a namespace of the ten
    outputs (RESULT_KEYS), to be compared with the kernel's bit for bit."""
    frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    cn, neighbors, max_nb = _lists(cn, neighbors, frac.shape[0])
    out = _empty_result(len(counts), frac.shape[0], F32)
    inf = F32(np.inf)
    with np.errstate(all="ignore"):
        for b, n in enumerate(counts):
            a0 = first[b]
            L, f = lattice[b], frac[a0:a0 + n]
            if not (np.isfinite(L).all() and np.isfinite(f).all()):
                out.flags[b] = NONFINITE
                continue
            if _list_is_bad(cn[a0:a0 + n], neighbors[a0:a0 + n], n, max_nb):
                out.flags[b] = BAD_LIST
                continue
            p = cb.positions_and_shifts(f, L, (0, 0, 0), F32)[0]
            flags = EMPTY if n == 0 else 0
            for i in range(n):
                m = int(min(cn[a0 + i], max_nb))
                out.n_used[a0 + i] = m
                flags |= (ISOLATED if m == 0 else 0) | (TRUNCATED if cn[a0 + i] > max_nb else 0)
                if m == 0:
                    continue
                disp, d2 = _bonds(p, L, i, neighbors[a0 + i, :m], F32)
                if (d2 == 0).any():
                    flags |= OVERLAP
                    continue
                u = (disp / np.sqrt(d2)[:, None]).astype(F32)
                pr = (u[:, None, :] * u[None, :, :]).astype(F32)  # [e, f, d]
                c = ((pr[..., 0] + pr[..., 1]).astype(F32) + pr[..., 2]).astype(F32)
                c = np.where(c < F32(-1), F32(-1), c)
                c = np.where(c > F32(1), F32(1), c)
                P = _legendre(c, F32)  # [4, e, f]
                s, lo, hi = np.zeros((64, len(L_VALUES)), F32), np.full(64, inf), np.full(64, -inf)
                for e in range(m - 1):  # lane f > e meets e in ascending order
                    fs = slice(e + 1, m)
                    s[fs] = (s[fs] + P[:, e, fs].T).astype(F32)
                    lo[fs] = np.where(c[e, fs] < lo[fs], c[e, fs], lo[fs])
                    hi[fs] = np.where(c[e, fs] > hi[fs], c[e, fs], hi[fs])
                S, mf = lane_sum(s), F32(m)
                q2 = ((mf + (F32(2) * S).astype(F32)).astype(F32) / (mf * mf).astype(F32)).astype(F32)
                q2 = np.where(q2 < F32(0), F32(0), q2)
                out.q2[a0 + i], out.q[a0 + i] = q2, np.sqrt(q2)
                if m >= 2:
                    out.cos_min[a0 + i] = _lane_extreme(lo, lambda o, v: o < v)
                    out.cos_max[a0 + i] = _lane_extreme(hi, lambda o, v: o > v)
                    iu = np.triu_indices(m, 1)
                    out.angles[a0 + i] = np.bincount(_bins(c[iu], COS_EDGES), minlength=ANGLE_BINS)
            out.flags[b] = flags
            out.angle_hist[b] = out.angles[a0:a0 + n].sum(axis=0)
            out.n_angles[b] = out.angle_hist[b].sum()
            lanes, used = np.zeros((64, len(L_VALUES)), F32), 0
            for i in range(n):  # lane = i mod 64, ascending i
                if out.n_used[a0 + i] >= 1 and np.isfinite(out.q[a0 + i]).all():
                    lanes[i % 64] = (lanes[i % 64] + out.q[a0 + i]).astype(F32)
                    used += 1
            if used:
                out.mean_q[b] = (lane_sum(lanes) / F32(used)).astype(F32)
    return out


def legendre_rounding_bound(l):
    """The derived bound on the rounding error the float32 recurrence itself adds to P_l (module docstring): E_{k+1} = a_k E_k +
    b_k E_{k-1} + 10 u from E_0 = E_1 = 0."""
    a, b = legendre_coefficients(np.float64)
    em, ek = 0.0, 0.0
    for k in range(1, int(l)):
        em, ek = ek, a[k - 1] * ek + b[k - 1] * em + 10.0 * U
    return float(ek)


def c_bound(lattice, shells, d_min):
    """The derived bound on |c_float32 - c_exact| of one crystal (module docstring): 160 u G / d_min + 8 u, G = max_d sum_k
    (1 + n_k) |L_kd|; inf for d_min = 0."""
    G = screening.distance_bound(lattice, shells) / (screening.DISTANCE_BOUND_FACTOR * U)
    return C_BOUND_FACTOR * U * G / d_min + 8.0 * U if d_min > 0 else np.inf


def q2_bound(l, cb_):
    """The derived bound on |q2_l float32 - exact| given the crystal's c_bound (module docstring)."""
    return 0.5 * l * (l + 1) * cb_ + legendre_rounding_bound(l) + 80.0 * U


def bond_order_reference_f64(frac, lattice, counts, cn, neighbors):
    """The same rules on the same lists in float64 from the same float32 inputs and edges, without the operation-order detail (a
    plain sum over the pairs).  Returns the ten outputs (reals float64) and `pair_margin` (a list with one array per atom: for
    every pair e < f, in row-major order, the distance of c to the nearest histogram edge), `margin` [N] (its smallest; inf
    without pairs, NaN where nothing was computed), `n_below` [N] (the pairs with a margin of at most 4 c_bound), `c_bound` [B]
    and `q2_bound` [B,4] (the derived float32 bounds; inf for a crystal with a bond of length 0, NaN where nothing was computed)
    and `guarded` [N]: margin > 4 c_bound."""
    frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    N, B = frac.shape[0], len(counts)
    cn, neighbors, max_nb = _lists(cn, neighbors, N)
    out = _empty_result(B, N, np.float64)
    out.pair_margin, out.margin, out.n_below = [np.empty(0)] * N, np.full(N, np.nan), np.zeros(N, np.int64)
    out.c_bound, out.q2_bound, out.guarded = np.full(B, np.nan), np.full((B, len(L_VALUES)), np.nan), np.zeros(N, bool)
    edges = COS_EDGES.astype(np.float64)
    with np.errstate(all="ignore"):
        for b, n in enumerate(counts):
            a0 = first[b]
            L, f = lattice[b].astype(np.float64), frac[a0:a0 + n].astype(np.float64)
            if not (np.isfinite(L).all() and np.isfinite(f).all()):
                out.flags[b] = NONFINITE
                continue
            if _list_is_bad(cn[a0:a0 + n], neighbors[a0:a0 + n], n, max_nb):
                out.flags[b] = BAD_LIST
                continue
            p = cb.positions_and_shifts(f, L, (0, 0, 0), np.float64)[0]
            flags, d_min, shells = EMPTY if n == 0 else 0, np.inf, np.zeros(3, np.int64)
            for i in range(n):
                m = int(min(cn[a0 + i], max_nb))
                out.n_used[a0 + i] = m
                out.margin[a0 + i] = np.inf
                flags |= (ISOLATED if m == 0 else 0) | (TRUNCATED if cn[a0 + i] > max_nb else 0)
                if m == 0:
                    continue
                shells = np.maximum(shells, np.abs(neighbors[a0 + i, :m, 1:]).max(axis=0))
                disp, d2 = _bonds(p, L, i, neighbors[a0 + i, :m], np.float64)
                d_min = min(d_min, float(np.sqrt(d2.min())))
                if (d2 == 0).any():
                    flags |= OVERLAP
                    out.margin[a0 + i] = np.nan
                    continue
                u = disp / np.sqrt(d2)[:, None]
                iu = np.triu_indices(m, 1)
                c = np.clip(u @ u.T, -1.0, 1.0)[iu]
                S = _legendre(c, np.float64).sum(axis=1)
                q2 = np.maximum((m + 2.0 * S) / (m * m), 0.0)
                out.q2[a0 + i], out.q[a0 + i] = q2, np.sqrt(q2)
                if m >= 2:
                    out.cos_min[a0 + i], out.cos_max[a0 + i] = c.min(), c.max()
                    out.angles[a0 + i] = np.bincount(_bins(c, edges), minlength=ANGLE_BINS)
                    out.pair_margin[a0 + i] = np.abs(c[:, None] - edges[None, :]).min(axis=1)
                    out.margin[a0 + i] = out.pair_margin[a0 + i].min()
            out.flags[b] = flags
            out.angle_hist[b] = out.angles[a0:a0 + n].sum(axis=0)
            out.n_angles[b] = out.angle_hist[b].sum()
            use = (out.n_used[a0:a0 + n] >= 1) & np.isfinite(out.q[a0:a0 + n]).all(axis=1)
            if use.any():
                out.mean_q[b] = out.q[a0:a0 + n][use].mean(axis=0)
            if np.isfinite(d_min):
                out.c_bound[b] = c_bound(L, shells, d_min)
                out.q2_bound[b] = [q2_bound(l, out.c_bound[b]) for l in L_VALUES]
                for i in range(a0, a0 + n):
                    out.n_below[i] = int((out.pair_margin[i] <= 4.0 * out.c_bound[b]).sum())
                out.guarded[a0:a0 + n] = out.margin[a0:a0 + n] > 4.0 * out.c_bound[b]
    return out


def reference_lists(frac, lattice, counts, params=None):
    """(cn, neighbors) of the coordination search's float32 restatement with a BondOrderParams: the lists the restatements above
    and the kernel's chain read."""
    p = params if params is not None else BondOrderParams()
    r = co.coordination_reference_f32(frac, lattice, counts, p.coordination())
    return r.cn, r.neighbors
