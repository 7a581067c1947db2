"""Symmetrization of generated crystals: with the operations the symmetry search found within symprec, the atoms moved onto sites
those operations map onto each other exactly, the cell given the metric they leave invariant, and the orbits -- which atoms are
equivalent, with which multiplicity and site-symmetry order (arreau_crystal_symmetrize, arreau_amd/csrc/symmetrize.hip; the rules
are written out in include/arreau_hip.h, "symmetrization").  Here: the parameters (the symmetry search's) and their validation,
the flag constants, the entry point that needs no engine (`symmetrize`, which runs the search itself unless its result is handed
in), `symmetrize_sample_result` for a SampleResult or a loaded file, `sample_arrays` / `symmetrized_crystals`, the statistics lines
and a float64 numpy restatement of rules 1-7 built on symmetry_search.symmetry_reference_f64 (`symmetrize_reference_f64`).  The
restatement needs numpy alone.

What this is not: no space-group number, no origin search, no standard setting; the cell keeps the basis it came in (only its
orientation in space becomes the sampler's).  The symmetric structure sits where the least-squares translations put it: its
origin is the input's, moved by the mean of the noise.

How it works.  The search stored operations (W_m, t_m) with residuals below symprec.  For each, p_m(i) is the atom the image of
atom i falls next to and delta_{m,i} = (W_m w_i + t_m) - w_{p_m(i)} (nearest integer removed) the miss, image minus partner as the
search's rule 4 forms it.  The translation that minimises sum_i |miss|^2 for that permutation is t'_m = t_m - mean_i delta_{m,i}
(ops_shift_m = t'_m - t_m), and the mean over the group of the partners carried back, W_m^-1 (w_{p_m(i)} - t'_m), is x'_i = w_i +
(1 / n_ops) sum_m W_m^-1 (mean_i delta_{m,i} - delta_{m,i}): invariant under every (W_m, t'_m) when the p_m are permutations
that compose as the operations do.  tests/test_symmetrize_cpu.py checks that in float64 to 1e-10 A.

float32 against float64 (rule 8).  Every arithmetic step of the kernel is one rounded float32 operation, never contracted; no
float32 restatement is kept.  Discrete outputs (flags, partners, orbits) are compared with the float64 restatement on GUARDED
inputs: every decision quantity of the search at most symprec / 2 or at least 2 symprec, and for every (m, i) the nearest partner
at most symprec / 2 away and the second nearest at least 2 symprec (`partner_margins`).  The reals are held to derived bounds.
u = 2^-24, n atoms, K = n_ops operations, D = the largest |component of a delta| of the crystal (taken from the restatement: a
property of the input), l_max / l_min the longest / shortest cell edge, l_1 = l_max + symprec (an accepted image vector is no
longer), r = l_1 / l_min.
  * delta: 24 u, whatever its size (symmetry_search's docstring: y = W w + t carries 19 u, the difference with w_j 5 u more, the
    removal of the nearest integer is exact).
  * ops_shift = -(sum_i delta) / n: the inputs' 24 u; n - 1 roundings of partial sums below n D, divided by n: (n - 1) D u; the
    division D u: (24 + n D) u.  t' = t + ops_shift: t carries 10 u, the sum (below 2) u: (35 + n D) u.
  * g = -ops_shift - delta: 24 u + (24 + n D) u and its own rounding of a value below 2 D: (48 + (n + 2) D) u =: E_g.  V g with V
    = W^-1, itself one of the group's rotations, entries in {-1, 0, 1}: 3 E_g and two roundings of sums below 6 D: 3 E_g + 12 D u.
    The sum over K operations in order: K - 1 roundings of partial sums below 6 K D, divided by K: 6 (K - 1) D u; the division
    6 D u.  The shift of an atom carries (144 + (3 n + 6 K + 18) D) u; w_i (u), the sum (u) and the wrap (u) add 3 u.
    POSITION_BOUND = (160 + (3 n + 6 K + 18) D) u covers positions and refined translations, both compared modulo 1
    (`position_bound`): 1.0e-5 for n = K = 192 and D = 0.01.
  * metric: a'_j = (W_0j a_0 + W_1j a_1) + W_2j a_2, exact products and two roundings of sums below A = max_d sum_k |L_kd| <= 3
    l_max per component: 3.5 u A in norm.  A scalar product of two images (each no longer than l_1): 7 u A l_1 from them, 4 u
    l_1^2 from its five operations: at most 25 u l_1^2.  The mean over at most 48 rotations in order: 47 u l_1^2 and the
    division's u l_1^2: |G'_f32 - G'| <= 80 u l_1^2.  length = sqrt(G'_ii): 80 u l_1^2 / (2 l_min) + u l_1 = (40 r + 1) l_1 u
    (`length_bound`).  cos = G'_jk / (len_j len_k): 80 r^2 u from G', 2 (40 r^2 + r) u from the lengths, 2 u from the product and
    the quotient: (160 r^2 + 2 r + 2) u; the angle: that over sin(angle), and 16 u (4 ulp of a value below 4) for the device's acos
    (`angle_bound`).
  * a displacement |u_i| is a length of the kind the search's residual is, formed from a shift that carries the position bound:
    it is compared within symmetry_search.residual_bound (64 u A), as the residuals are."""
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from . import symmetry_search as ss

NONFINITE, CELL, EMPTY, NO_GROUP, NOT_A_PERMUTATION = 1, 2, 4, 8, 16
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (NO_GROUP, "NO_GROUP"), (NOT_A_PERMUTATION, "NOT_A_PERMUTATION"))
ATOM_KEYS = ("frac_x", "orbit", "orbit_size", "site_order")  # one row per atom; the other keys one row per crystal
SYMMETRIZED_KEYS = ("frac_x", "lattice", "lengths", "angles", "orbit", "orbit_size", "site_order", "n_orbits", "max_displacement",
                    "rms_displacement", "ops_translation", "flags")  # what SampleResult.symmetrized and a crystals file hold
RESULT_KEYS = ("frac_out", "lattice", "lengths", "angles", "orbit", "orbit_size", "site_order", "n_orbits", "max_displacement",
               "rms_displacement", "ops_translation", "ops_shift", "partner", "flags")  # arreau_symmetrize_result, in its order
U = 2.0 ** -24


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class SymmetrizeParams(ss.SymmetrySearchParams):
    """The symmetry search's parameters: symprec, the tolerance in A the operations are found with (0.1 by default), and max_ops,
    the operations stored per crystal -- a crystal with more is flagged NO_GROUP and copied through."""

    def search(self) -> ss.SymmetrySearchParams:
        return ss.SymmetrySearchParams(symprec=self.symprec, max_ops=self.max_ops)


def resolve(symmetrize):
    """sample(symmetrize=...): None / False -> None, True -> the defaults, a SymmetrizeParams -> itself."""
    return cb.resolve(symmetrize, SymmetrizeParams, "symmetrize")


def check_shared_search(symmetrize_params, find_symmetry_params):
    """sample(symmetrize=..., find_symmetry=...) shares one search launch: its parameters must agree."""
    if symmetrize_params is None or find_symmetry_params is None:
        return
    a, b = symmetrize_params, find_symmetry_params
    if (a.symprec, a.max_ops) != (b.symprec, b.max_ops):
        raise ValueError(f"symmetrize and find_symmetry share one search: symprec / max_ops {a.symprec} / {a.max_ops} and "
                         f"{b.symprec} / {b.max_ops} disagree")


# ------------------------------------------------------------------------------------------------------- the device call
def symmetrize(frac, lattice, offsets, types, params=None, found=None):
    """Symmetrize a batch on the GPU without an engine (arreau_crystal_symmetrize, one launch; one more for the search when
    `found`, the dict of symmetry_search.find_symmetry on the same tensors, is not handed in).  frac [N,3] float32, lattice
    [B,3,3] float32 (rows a, b, c), offsets [B+1] int32 and types [N] int32 (species ids) are contiguous tensors on one cuda
    device.  Returns a dict of device tensors: frac_out [N,3], orbit, orbit_size, site_order [N]; lattice [B,3,3], lengths, angles
    [B,3], n_orbits, max_displacement, rms_displacement, flags [B]; ops_translation, ops_shift [B,max_ops,3]; partner [max_ops,N];
    and `found`, `offsets`.  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else SymmetrizeParams()
    dev, B, N = cb.check_batch("symmetrize", frac, lattice, offsets, types)
    if found is None:
        found = ss.find_symmetry(frac, lattice, offsets, types, ss.SymmetrySearchParams(symprec=p.symprec, max_ops=p.max_ops))
    M = int(found["ops_rotation"].shape[1])
    if int(found["ops_rotation"].shape[0]) != B or found["ops_rotation"].device != dev:
        raise ValueError("symmetrize: `found` is not the search of this batch")
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {"frac_out": torch.empty((N, 3), **f32), "lattice": torch.empty((B, 3, 3), **f32), "lengths": torch.empty((B, 3), **f32),
           "angles": torch.empty((B, 3), **f32), "orbit": torch.empty(N, **i32), "orbit_size": torch.empty(N, **i32),
           "site_order": torch.empty(N, **i32), "n_orbits": torch.empty(B, **i32), "max_displacement": torch.empty(B, **f32),
           "rms_displacement": torch.empty(B, **f32), "ops_translation": torch.empty((B, M, 3), **f32),
           "ops_shift": torch.empty((B, M, 3), **f32), "partner": torch.empty((M, N), **i32), "flags": torch.empty(B, **i32)}
    s = _hip.SymmetryResultC(*[_hip.ptr(found[k]).value if B else None for k in ss.SYM_KEYS[:-1]])
    r = _hip.SymmetrizeResultC(*[_hip.ptr(out[k]).value if out[k].numel() else None for k in RESULT_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_symmetrize(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(offsets), B, N,
                                                        ctypes.byref(s), M, ctypes.byref(r), _hip.stream_ptr(dev)),
                   "arreau_crystal_symmetrize")
    out["found"], out["offsets"] = found, offsets
    return out


def result_to_numpy(result):
    """The dict of `symmetrize` as host numpy arrays (synchronises); `found` becomes the numpy dict of the search, and frac_x is
    frac_out under the name a crystals file uses."""
    out = cb.to_numpy({k: v for k, v in result.items() if k != "found"})
    if result.get("found") is not None:
        out["found"] = ss.result_to_numpy(result["found"])
    out["frac_x"] = out["frac_out"]
    return out


def symmetrize_sample_result(result, params=None, device="cuda"):
    """The symmetrization of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32 and its
    atomic numbers taken as species ids: the dict of `result_to_numpy`."""
    return result_to_numpy(symmetrize(*cb.upload(result, device), params))


def sample_arrays(symmetrized):
    """What SampleResult.symmetrized and a crystals file hold (SYMMETRIZED_KEYS) of a `result_to_numpy` dict."""
    return {k: np.asarray(symmetrized[k]) for k in SYMMETRIZED_KEYS}


def symmetrized_crystals(symmetrized, atomic_numbers, num_atoms):
    """The symmetrized crystals as the arrays of a crystals file: frac_x and lattice float64 (the rebuilt cells), the input's
    atomic_numbers and num_atoms, idx_start."""
    return cb.crystal_arrays(symmetrized["frac_x"], symmetrized["lattice"], atomic_numbers, num_atoms)


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the count per number of orbits and per flag, and
    the largest displacement."""
    k = np.asarray(result["n_orbits"], dtype=np.int64).reshape(-1)
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    moved = np.asarray(result["max_displacement"], dtype=np.float64).reshape(-1)
    ok = flags == 0
    return {"rank": cb.rank_of(rank), "attempted": int(k.size), "symmetrized": int(ok.sum()),
            "n_orbits": {int(v): int((k[ok] == v).sum()) for v in np.unique(k[ok])},
            "max_displacement": float(moved[ok].max()) if ok.any() else 0.0,
            "flags": cb.flag_counts(flags, FLAG_NAMES)}


def total_stats(parts):
    orbits = {}
    for p in parts:
        for k, v in p["n_orbits"].items():
            orbits[int(k)] = orbits.get(int(k), 0) + v
    return {"rank": "total", "attempted": sum(p["attempted"] for p in parts), "symmetrized": sum(p["symmetrized"] for p in parts),
            "n_orbits": dict(sorted(orbits.items())), "max_displacement": max([p["max_displacement"] for p in parts] + [0.0]),
            "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'symmetrize rank 0: symmetrized 15 / attempted 16; orbits 2: 3, 20: 12; max displacement 0.031 A; flags NO_GROUP 1'."""
    orbits = cb.some(dict(sorted((int(k), v) for k, v in st["n_orbits"].items())), ": ")
    return f"symmetrize {cb.who(st)}: symmetrized {st['symmetrized']} / attempted {st['attempted']}; orbits {orbits}; " \
           f"max displacement {st['max_displacement']:.3g} A; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------------ the derived bounds
def position_bound(n, n_ops, D):
    """|float32 - exact| of a component of frac_out or of a refined translation, modulo 1 (module docstring)."""
    return (160.0 + (3.0 * n + 6.0 * n_ops + 18.0) * D) * U


def _edges(lattice, symprec):
    ln = np.linalg.norm(np.asarray(lattice, dtype=np.float64).reshape(3, 3), axis=1)
    l1 = float(ln.max()) + float(symprec)
    return l1, l1 / float(ln.min())


def length_bound(lattice, symprec):
    """|float32 - exact| of a symmetrized cell length (module docstring): (40 r + 1) l_1 u, from the INPUT cell."""
    l1, r = _edges(lattice, symprec)
    return (40.0 * r + 1.0) * l1 * U


def angle_bound(lattice, symprec, angles):
    """|float32 - exact| of a symmetrized cell angle: ((160 r^2 + 2 r + 2) / sin(angle) + 16) u, with the smallest sine of the
    restatement's `angles` [3]."""
    _, r = _edges(lattice, symprec)
    return ((160.0 * r * r + 2.0 * r + 2.0) / float(np.sin(np.asarray(angles, dtype=np.float64)).min()) + 16.0) * U


# -------------------------------------------------------------------------------------------------- the numpy restatement
def lattice_from_params_f64(lengths, angles):
    """Rows a, b, c of the cell in the sampler's orientation (lattice_helpers.lattice_from_params; arreau_prep_cell) in float64."""
    a, b, c = (float(v) for v in lengths)
    ca, cb, cg = np.cos(np.asarray(angles, dtype=np.float64))
    sa, sb = np.sin(np.asarray(angles, dtype=np.float64)[:2])
    gs = math.acos(min(1.0, max(-1.0, (ca * cb - cg) / (sa * sb))))
    return np.array([[a * sb, 0.0, a * cb], [-b * sa * math.cos(gs), b * sa * math.sin(gs), b * ca], [0.0, 0.0, c]])


def params_of_metric(G):
    """(lengths [3], angles [3] in radians) of a metric tensor: angle i lies between the other two vectors (rule 5)."""
    with np.errstate(all="ignore"):
        ln = np.sqrt(np.diag(G))
        ang = np.array([np.arccos(np.clip(G[(i + 1) % 3, (i + 2) % 3] / (ln[(i + 1) % 3] * ln[(i + 2) % 3]), -1.0, 1.0)) for i in range(3)])
    return ln, ang


def inverse_rotation(W):
    """The exact integer inverse of an integer matrix of determinant +-1."""
    return np.rint(np.linalg.inv(np.asarray(W, dtype=np.float64))).astype(np.int64)


def refined_operations(ref, b):
    """[(W, t')] of crystal b of a restatement's (or `result_to_numpy`'s) arrays `ops_rotation` and `ops_translation`."""
    return [(ss.decode_rotation(int(c)), np.asarray(t, dtype=np.float64)) for c, t in zip(ref.ops_rotation[b], ref.ops_translation[b]) if c >= 0]


def symmetrize_reference_f64(frac, lattice, counts, types, params=None, found=None):
    """Rules 1-7 in float64 from the same float32 inputs: frac [N,3], lattice [B,3,3], counts [B] atoms per crystal, types [N];
    `found`: the namespace of symmetry_search.symmetry_reference_f64 on them (computed here when None).  Returns a namespace of
    the kernel's outputs (the reals float64; partner [max_ops, N]; ops_rotation [B, max_ops], the codes of the operations used,
    -1 elsewhere) and, for the guard of the test cases, per crystal `nearest` and `second` (the distance in A from every image
    (m, i) to its partner and to the next atom of the species, inf where there is none) and `D`, the largest |component| of a
    delta."""
    p = params if params is not None else SymmetrizeParams()
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    if found is None:
        found = ss.symmetry_reference_f64(frac, lattice, counts, types, ss.SymmetrySearchParams(symprec=p.symprec, max_ops=p.max_ops))
    B, N, M = len(counts), frac.shape[0], int(found.ops_rotation.shape[1])
    out = SimpleNamespace(frac_out=np.zeros((N, 3)), lattice=np.zeros((B, 3, 3)), lengths=np.zeros((B, 3)), angles=np.zeros((B, 3)),
                          orbit=np.zeros(N, np.int32), orbit_size=np.ones(N, np.int32), site_order=np.ones(N, np.int32),
                          n_orbits=np.array(counts, np.int32), max_displacement=np.zeros(B), rms_displacement=np.zeros(B),
                          ops_translation=np.zeros((B, M, 3)), ops_shift=np.zeros((B, M, 3)), partner=np.full((M, N), -1, np.int32),
                          flags=np.zeros(B, np.int32), ops_rotation=np.full((B, M), -1, np.int32), nearest=[None] * B, second=[None] * B,
                          D=np.zeros(B))
    for b, n in enumerate(counts):
        a0 = first[b]
        L, f, ty = lattice[b].astype(np.float64), frac[a0:a0 + n].astype(np.float64), types[a0:a0 + n]
        with np.errstate(all="ignore"):
            w = ss._wrap01(frac[a0:a0 + n].copy()).astype(np.float64)  # the float32 wrap, as the kernel copies it through
            G = L @ L.T
        out.frac_out[a0:a0 + n], out.orbit[a0:a0 + n] = w, np.arange(n)
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
        else:
            vol = abs(float(np.dot(L[0], np.cross(L[1], L[2]))))
            out.flags[b] = (CELL if (not vol > 0.0 or not np.isfinite(vol)) else 0) | (EMPTY if n == 0 else 0)
        K = int(found.n_ops[b])
        if not out.flags[b] and (int(found.flags[b]) & (ss.AMBIGUOUS | ss.OVERFLOW | ss.NOT_A_GROUP) or not 1 <= K <= M):
            out.flags[b] = NO_GROUP
        if not out.flags[b]:
            Ws = [ss.decode_rotation(int(c)) for c in found.ops_rotation[b, :K]]
            ts = np.asarray(found.ops_translation[b, :K], dtype=np.float64)
            w = ss._wrap01(f.copy())
            other = ty[:, None] != ty[None, :]
            partner = np.empty((K, n), dtype=np.int64)
            delta = np.empty((K, n, 3))
            nearest, second = np.empty((K, n)), np.full((K, n), np.inf)
            for m in range(K):
                e = ss._wrap_nearest((w @ Ws[m].T.astype(np.float64) + ts[m])[:, None, :] - w[None, :, :])  # [i, j, 3]
                d = np.linalg.norm(e @ L, axis=2)
                d[other] = np.inf
                partner[m] = d.argmin(axis=1)  # (the first minimum: ties to the smallest j)
                delta[m] = e[np.arange(n), partner[m]]
                srt = np.sort(d, axis=1)
                nearest[m] = srt[:, 0]
                if n > 1:
                    second[m] = srt[:, 1]
            out.nearest[b], out.second[b], out.D[b] = nearest, second, float(np.abs(delta).max())
            sizes = np.array([len(set(partner[:, i].tolist())) for i in range(n)])
            if any(len(set(partner[m].tolist())) != n for m in range(K)) or (K % sizes != 0).any():
                out.flags[b] = NOT_A_PERMUTATION
        if not out.flags[b]:
            mean = delta.mean(axis=1)  # [K,3]
            shift = -mean
            moved = np.zeros((n, 3))
            for m in range(K):
                moved += (mean[m] - delta[m]) @ inverse_rotation(Ws[m]).T.astype(np.float64)
            moved /= K
            out.frac_out[a0:a0 + n] = ss._wrap01(w + moved)
            out.partner[:K, a0:a0 + n] = partner
            out.ops_rotation[b, :K] = found.ops_rotation[b, :K]
            out.ops_shift[b, :K], out.ops_translation[b, :K] = shift, ts + shift
            out.orbit[a0:a0 + n], out.orbit_size[a0:a0 + n] = partner.min(axis=0), sizes
            out.site_order[a0:a0 + n] = K // sizes
            out.n_orbits[b] = int((partner.min(axis=0) == np.arange(n)).sum())
            dist = np.linalg.norm(moved @ L, axis=1)
            out.max_displacement[b], out.rms_displacement[b] = dist.max(), math.sqrt(float((dist ** 2).mean()))
            distinct = {int(c): W for c, W in zip(found.ops_rotation[b, :K], Ws)}
            G = sum(W.T.astype(np.float64) @ G @ W.astype(np.float64) for W in distinct.values()) / len(distinct)
        out.lengths[b], out.angles[b] = params_of_metric(G)
        with np.errstate(all="ignore"):
            out.lattice[b] = lattice_from_params_f64(out.lengths[b], out.angles[b]) if np.isfinite(G).all() and (np.diag(G) > 0).all() else np.nan
    return out


def partner_margins(ref, b):
    """(the largest nearest-partner distance, the smallest second-nearest distance) of crystal b of a restatement, in A; None for
    a crystal that took no partner decision."""
    if ref.nearest[b] is None:
        return None
    return float(ref.nearest[b].max()), float(ref.second[b].min())
