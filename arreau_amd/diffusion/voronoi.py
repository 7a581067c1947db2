"""Voronoi cells of generated crystals: per atom the faces of its Voronoi cell over every periodic image -- the neighbour behind
each face, the solid angle the face subtends, its area and distance --, the weight of each face (its solid angle over the atom's
largest: pymatgen VoronoiNN's weight, where CrystalNN starts), the number of faces of weight >= tol, the cell's volume and a
certificate that the cell is closed; per crystal the sums and extremes (arreau_crystal_voronoi, arreau_amd/csrc/voronoi.hip; the
rules are written out in include/arreau_hip.h).  Here: the parameters and their validation, the flag constants, the entry point that
needs no engine (`voronoi`), the statistics, `bond_segments` (the Cartesian end points of the stored faces' bonds: what the
reference's predict_bonds returns) and `voronoi_reference`, a numpy restatement of rules 0-6 -- in float64 the yardstick of the
tests, which also reports the margin of every deciding comparison; in float32 the same arithmetic, which
tools/exp/voronoi_f32_deviation.py measures against the float64 one.  A bit-for-bit float32 restatement does not exist: the solve
and atan2 make it pointless.  Needs numpy alone at import.

Not CrystalNN: no radii, no electronegativity terms, no distance weighting, no probabilities; plain Voronoi cells (not radical, not
weighted); no polyhedron names.

The float32 bounds of the reals are MEASURED, not derived (F32_DEVIATION below): the largest deviation of the float32 restatement
from the float64 one over every batch of tests/voronoi_cases.py, relative to the natural scale -- 4 pi for solid angles and
omega_sum, 1 for weights, V/n for volumes, (V/n)^(2/3) for areas, 1 for cn_eff (a sum of weights), the cutoff for lengths --, and
the tests allow BOUND_FACTOR = 16 times that for the device's atan2f and division and its different summation order over at most
128 fan triangles.  A lost vertex or a wrong face moves a solid angle by 1e-3 or more, so the factor hides nothing.  They are
never tuned from the kernel's output.  For an OPEN atom the bounds on volume, face_area and max_radius come out at 0.95 V/n, 2.3
(V/n)^(2/3) and 0.14 cutoff: those three are in effect unchecked on the device for OPEN atoms (two thirds of the ragged batch),
which are constrained by their integers, list, solid angles, weights and distances alone; atoms that are not OPEN are held to
F32_DEVIATION_CLOSED.

The kernel solves and tests the planes (rule 2) in float64 from its float32 displacements and builds the faces (rule 3) in float32;
`voronoi_reference(dtype=float32)` has that split, `dtype=float64` is float64 throughout.

Guards (an atom is GUARDED when the kernel must decide every comparison as the float64 restatement does): each face's |weight -
tol| > 1e-4; each solved triple's distance to the plane test's threshold more than ten times the float64 bound of its vertex, 8 u
(|d_a| + |d_b| + |d_c|) / (2 det_n) + 4 u |v| with u = 2^-53 and det_n = |det| / (|d_a||d_b||d_c|) (the header derives it); |det_n -
DET_TOL| > 1e-3 DET_TOL for each triple whose vertex passes the plane test or misses it by less than that (DET_TOL decides nothing
about the others); |2 max_radius - cutoff| > ten times the largest such vertex bound plus the vertex's float32 rounding; the closure residual's distance to CLOSURE_TOL > ten
times CLOSURE_F32 = 2e-5 (the float32 sum of a closed cell's solid angles); every candidate's |d2 - r2| / r2 > 1e-5."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import coordination as co
from . import crystal_batch as cb
from . import screening

NONFINITE, CELL, EMPTY, OVERLAP, OPEN, OVERFLOW, TRUNCATED = 1, 2, 4, 8, 16, 32, 64
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (OVERLAP, "OVERLAP"), (OPEN, "OPEN"), (OVERFLOW, "OVERFLOW"),
              (TRUNCATED, "TRUNCATED"))
FLAGS = FLAG_NAMES
MAX_FACES, MAX_CANDIDATES, FACE_VERTICES = 64, 128, 128
MAX_SHELLS = screening.MAX_SHELLS
DET_TOL, PLANE_TOL, CLOSURE_TOL = 1e-6, 1e-6, 1e-3  # include/arreau_hip.h: ARREAU_VORONOI_* (the first two float64, the last float32)
CRYSTAL_KEYS = ("n_faces", "min_cn", "max_cn", "mean_cn", "mean_cn_eff", "volume_sum", "flags")  # one row per crystal
FACE_KEYS = ("face_weight", "face_solid_angle", "face_area", "face_distance")
RESULT_KEYS = CRYSTAL_KEYS + ("cn", "neighbors") + FACE_KEYS + ("volume", "omega_sum", "max_radius", "cn_eff", "atom_flags")  # arreau_voronoi_result, in its order
ATOM_KEYS = RESULT_KEYS[len(CRYSTAL_KEYS):] + ("species",)  # one row per atom; species: the atoms' atomic numbers
STORED_KEYS = CRYSTAL_KEYS + ATOM_KEYS  # what SampleResult.voronoi and a crystals file hold
INTEGER_KEYS = ("n_faces", "min_cn", "max_cn", "flags", "cn", "neighbors", "atom_flags")
F32 = np.float32
U = 2.0 ** -24
U64 = 2.0 ** -53
# measured by tools/exp/voronoi_f32_deviation.py (numpy float32 against float64 over every batch of tests/voronoi_cases.py), each
# relative to its scale (module docstring); the tests allow BOUND_FACTOR times these
F32_DEVIATION = {"face_solid_angle": 3.54e-7, "omega_sum": 2.26e-7, "face_weight": 1.65e-6, "cn_eff": 7.91e-6, "volume": 5.93e-2,
                 "face_area": 1.43e-1, "max_radius": 8.85e-3, "face_distance": 4.27e-7}
# the same over the atoms that are not OPEN.  An unclosed cell has far vertices from nearly parallel planes (det_n down to DET_TOL)
# whose coordinates are large; rounding them to float32 moves its areas, its volume and its radius by the percents above, while its
# solid angles stay as good as a closed cell's.  A closed atom is held to these:
F32_DEVIATION_CLOSED = {"face_solid_angle": 2.67e-7, "omega_sum": 2.00e-7, "face_weight": 1.54e-6, "cn_eff": 7.91e-6, "volume": 4.18e-7,
                        "face_area": 1.28e-6, "max_radius": 1.55e-7, "face_distance": 4.00e-7}
# the batches at the caps (tests/voronoi_cases.py: NEW_NAMES; faces of up to 128 vertex copies, atoms of 40 and 70 faces), measured
# the same way after the tables above were made.  A batch that exceeds a table has a row here, (closed, any): per quantity the
# larger of the table's number and its own, and only that batch is held to it; "hard cap" exceeds nothing and has none.  The older
# batches' bounds are the tables above, unchanged.
_AT_CAPS = {"cages": {"face_solid_angle": 2.72e-7, "omega_sum": 5.34e-7, "volume": 7.03e-7, "face_area": 1.78e-6},
            "hub40": {"cn_eff": 7.95e-6, "volume": 4.28e-7}, "hub70": {"cn_eff": 1.36e-5},
            "large wide": {"volume": 7.25e-7, "face_area": 1.71e-6}}  # (what each exceeds F32_DEVIATION_CLOSED by; its OPEN atoms: within F32_DEVIATION)
F32_DEVIATION_AT_CAPS = {name: ({**F32_DEVIATION_CLOSED, **row}, {k: max(v, row.get(k, 0.0)) for k, v in F32_DEVIATION.items()})
                         for name, row in _AT_CAPS.items()}
BOUND_FACTOR = 16.0
WEIGHT_GUARD, DET_GUARD, CUTOFF_GUARD, GUARD_FACTOR, CLOSURE_F32 = 1e-4, 1e-3, 1e-5, 10.0, 2e-5


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class VoronoiParams:
    """tol: a face counts as a neighbour when its weight (solid angle over the atom's largest) is at least tol, in [0, 1] (0.05: a
    starting value, not a claim); cutoff in A: the atoms whose planes may bound a cell, and the image search covers it (6.0: a
    starting value; an atom whose cell it does not close is flagged OPEN); max_faces: the faces stored per atom (1..64; cn counts
    them all); max_candidates: the atoms within the cutoff an atom may have (1..128; more: OVERFLOW); max_shells caps the periodic
    images per axis (1..8): a cell that needs more is flagged CELL."""
    tol: float = 0.05
    cutoff: float = 6.0
    max_faces: int = 32
    max_candidates: int = MAX_CANDIDATES
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
        if not self.tol <= 1.0:
            raise ValueError(f"tol must lie in [0, 1], got {self.tol}")
        if not float(F32(self.cutoff)) > 0.0:
            raise ValueError(f"cutoff must be > 0, got {self.cutoff}")
        for name, top in (("max_faces", MAX_FACES), ("max_candidates", MAX_CANDIDATES), ("max_shells", MAX_SHELLS)):
            v = getattr(self, name)
            if not isinstance(v, Integral) or isinstance(v, bool) or not 1 <= int(v) <= top:
                raise ValueError(f"{name} must lie in 1..{top}, got {v!r}")
            object.__setattr__(self, name, int(v))


def resolve(voronoi):
    """sample(voronoi=...): None / False -> None, True -> the defaults, a VoronoiParams -> itself."""
    return cb.resolve(voronoi, VoronoiParams, "voronoi")


# ------------------------------------------------------------------------------------------------------- the device call
def voronoi(frac, lattice, offsets, params=None):
    """The Voronoi cells of a batch on the GPU without an engine (arreau_crystal_voronoi, one launch).  frac [N,3] float32, lattice
    [B,3,3] float32 (rows a, b, c) and offsets [B+1] int32 are contiguous tensors on one cuda device.  Returns a dict of device
    tensors (RESULT_KEYS): n_faces, min_cn, max_cn, mean_cn, mean_cn_eff, volume_sum, flags [B]; cn, volume, omega_sum,
    max_radius, cn_eff, atom_flags [N]; neighbors [N, max_faces, 4] (j local to the crystal, n_1, n_2, n_3; -1 beyond cn);
    face_weight, face_solid_angle, face_area, face_distance [N, max_faces] (NaN beyond cn).  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else VoronoiParams()
    dev, B, N = cb.check_batch("voronoi", frac, lattice, offsets, None, types_optional=True)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    reals = ("mean_cn", "mean_cn_eff", "volume_sum", "volume", "omega_sum", "max_radius", "cn_eff")
    out = {k: torch.empty(B, **(f32 if k in reals else i32)) for k in CRYSTAL_KEYS}
    out.update({"cn": torch.empty(N, **i32), "neighbors": torch.empty((N, p.max_faces, 4), **i32)})
    out.update({k: torch.empty((N, p.max_faces), **f32) for k in FACE_KEYS})
    out.update({k: torch.empty(N, **(f32 if k in reals else i32)) for k in ("volume", "omega_sum", "max_radius", "cn_eff", "atom_flags")})
    c = _hip.VoronoiParamsC(p.tol, p.cutoff, p.max_faces, p.max_candidates, p.max_shells)
    r = _hip.VoronoiResultC(*[_hip.ptr(out[k]).value if out[k].numel() else None for k in RESULT_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_voronoi(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(offsets), B, N, ctypes.byref(c),
                                                     ctypes.byref(r), _hip.stream_ptr(dev)), "arreau_crystal_voronoi")
    return out


def result_to_numpy(result):
    """The dict of `voronoi` as host numpy arrays (synchronises)."""
    return cb.to_numpy(result)


def sample_arrays(result, atomic_numbers):
    """What SampleResult.voronoi and a crystals file hold (STORED_KEYS) of a `result_to_numpy` dict: its arrays and `species`,
    the atomic numbers of the atoms (what the means per element are taken over)."""
    out = {k: np.asarray(result[k]) for k in STORED_KEYS if k != "species"}
    out["species"] = np.rint(np.asarray(atomic_numbers, dtype=np.float64).reshape(-1)).astype(np.int64)
    if out["species"].shape != out["cn"].shape:
        raise ValueError("voronoi: one atomic number per atom is needed")
    return out


def voronoi_sample_result(result, params=None, device="cuda"):
    """The Voronoi cells of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32: the dict of
    `sample_arrays`."""
    frac, lattice, off, _ = cb.upload(result, device)
    return sample_arrays(result_to_numpy(voronoi(frac, lattice, off, params)), result.atomic_numbers)


def bond_segments(result, crystals, b):
    """The Cartesian end points [K, 2, 3] (float64) of crystal b's stored faces' bonds: from atom i's wrapped position to the
    wrapped position of the neighbour j behind the face, shifted by its image (n_1, n_2, n_3); atoms in order, each atom's faces
    in stored order.  `result` holds cn and neighbors (numpy), `crystals` frac_x, lattice and num_atoms."""
    return co.bond_segments(result, crystals, b)


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the histogram of cn over the atoms whose cells were
    built, their summed cn and cn_eff overall and per element (`species` given), the OPEN atoms, the count per flag."""
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    cn = np.asarray(result["cn"], dtype=np.int64).reshape(-1)
    eff = np.asarray(result["cn_eff"], dtype=np.float64).reshape(-1)
    done = ~np.isnan(np.asarray(result["omega_sum"], dtype=np.float64).reshape(-1)) & ~np.isnan(eff)  # (not blanked, not OVERFLOW)
    is_open = (np.asarray(result["atom_flags"], dtype=np.int64).reshape(-1) & OPEN) != 0
    out = {"rank": cb.rank_of(rank), "crystals": int(flags.size), "atoms": int(done.sum()),
           "cn": {int(v): int((cn[done] == v).sum()) for v in np.unique(cn[done])}, "n_faces": int(cn[done].sum()),
           "cn_eff": float(eff[done].sum()), "open": int((is_open & done).sum()), "elements": {}, "flags": cb.flag_counts(flags, FLAG_NAMES)}
    if result.get("species") is not None:
        z = np.asarray(result["species"], dtype=np.int64).reshape(-1)
        out["elements"] = {int(v): [int(((z == v) & done).sum()), int(cn[(z == v) & done].sum()), float(eff[(z == v) & done].sum())]
                           for v in np.unique(z[done])}
    return out


def total_stats(parts):
    hist, elements = {}, {}
    for p in parts:
        for k, v in p["cn"].items():
            hist[int(k)] = hist.get(int(k), 0) + v
        for k, (a, s, e) in p["elements"].items():
            have = elements.get(int(k), [0, 0, 0.0])
            elements[int(k)] = [have[0] + a, have[1] + s, have[2] + e]
    return {"rank": "total", "crystals": sum(p["crystals"] for p in parts), "atoms": sum(p["atoms"] for p in parts),
            "cn": dict(sorted(hist.items())), "n_faces": sum(p["n_faces"] for p in parts), "cn_eff": sum(p["cn_eff"] for p in parts),
            "open": sum(p["open"] for p in parts), "elements": dict(sorted(elements.items())),
            "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'voronoi rank 0: 16 crystals, 320 atoms; cn 12: 12, 14: 308; mean cn 13.92, cn_eff 10.41 (Z 11: 14.00 / 10.50); open 3 / 320
    atoms (0.9 %); flags OPEN 1'."""
    hist = cb.some(dict(sorted((int(k), v) for k, v in st["cn"].items())), ": ")
    mean = f"cn {st['n_faces'] / st['atoms']:.2f}, cn_eff {st['cn_eff'] / st['atoms']:.2f}" if st["atoms"] else "cn n/a, cn_eff n/a"
    per = ", ".join(f"Z {int(k)}: {s / a:.2f} / {e / a:.2f}" for k, (a, s, e) in sorted((int(k), v) for k, v in st["elements"].items()) if a)
    share = f" ({100.0 * st['open'] / st['atoms']:.1f} %)" if st["atoms"] else ""
    return f"voronoi {cb.who(st)}: {st['crystals']} crystals, {st['atoms']} atoms; cn {hist}; mean {mean}" + \
        (f" ({per})" if per else "") + f"; open {st['open']} / {st['atoms']} atoms{share}; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------- the numpy restatement
def _empty_result(B, N, max_faces, real):
    nan = lambda *shape: np.full(shape, np.nan, real)
    return SimpleNamespace(n_faces=np.zeros(B, np.int32), min_cn=np.full(B, -1, np.int32), max_cn=np.full(B, -1, np.int32), mean_cn=nan(B),
                           mean_cn_eff=nan(B), volume_sum=nan(B), flags=np.zeros(B, np.int32), cn=np.zeros(N, np.int32),
                           neighbors=np.full((N, max_faces, 4), -1, np.int32), face_weight=nan(N, max_faces), face_solid_angle=nan(N, max_faces),
                           face_area=nan(N, max_faces), face_distance=nan(N, max_faces), volume=nan(N), omega_sum=nan(N), max_radius=nan(N),
                           cn_eff=nan(N), atom_flags=np.zeros(N, np.int32))


_TRIPLES = {}


def _triples(K):
    """Every a < b < c below K in lexicographic order: three index arrays."""
    if K not in _TRIPLES:
        a, b, c = np.meshgrid(np.arange(K), np.arange(K), np.arange(K), indexing="ij")
        keep = (a < b) & (b < c)
        _TRIPLES[K] = (a[keep], b[keep], c[keep])
    return _TRIPLES[K]


def _cross(u, v, dt):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1).astype(dt)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def atom_cell(d, d2, cutoff, tol, dt=np.float64, chunk=1 << 15):
    """Rules 2-5 for one atom from its candidates' displacements d [K,3] and squared distances d2 [K] (both of dtype dt, in
    ascending (j, m)): rule 2 (the planes) in float64 from d taken as exact, as the kernel does; the vertices rounded to dt and
    rules 3-5 in dt.  Returns a namespace: is_face [K], omega, area, weight [K] (0 where no face), length [K], volume, omega_sum,
    max_radius, cn_eff, cn, open, nv [K] (the vertex copies found on each candidate's plane), too_many (a face with more than
    FACE_VERTICES of them), faces (per face the ordered vertices [k,3]), and the margins plane_ratio, det, radius, closure, weight, bound (module docstring)."""
    K = d.shape[0]
    f8 = np.float64
    D = d.astype(f8)
    h = 0.5 * ((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
    L8 = np.sqrt(2.0 * h)
    l = np.sqrt(d2).astype(dt)  # the stored distance
    verts = [[] for _ in range(K)]
    m = SimpleNamespace(plane_ratio=np.inf, det=np.inf, bound=0.0)
    max_r2 = dt(0)
    if K >= 3:
        ta, tb, tc = _triples(K)
        thr = PLANE_TOL * float(cutoff) * L8
        for s0 in range(0, ta.size, chunk):
            a, b, c = ta[s0:s0 + chunk], tb[s0:s0 + chunk], tc[s0:s0 + chunk]
            ab, bc, ca = _cross(D[a], D[b], f8), _cross(D[b], D[c], f8), _cross(D[c], D[a], f8)
            det = _dot(ab, D[c])
            prod = L8[a] * L8[b] * L8[c]
            with np.errstate(all="ignore"):
                detn = np.abs(det) / prod
                solved = (det != 0) & ~(np.abs(det) < DET_TOL * prod)
                v = (h[a][:, None] * bc + h[b][:, None] * ca + h[c][:, None] * ab) / det[:, None]
            idx = np.flatnonzero((det != 0) & np.isfinite(v).all(axis=1))  # (a skipped triple is solved too: would its vertex count?)
            if idx.size == 0:
                continue
            a, b, c, v, detn, solved = a[idx], b[idx], c[idx], v[idx], detn[idx], solved[idx]
            over = (v @ D.T - h[None, :]) - thr[None, :]  # > 0: beyond the plane's slack
            with np.errstate(all="ignore"):
                over = over / L8[None, :]  # as a distance
            over[np.isnan(over)] = -np.inf  # (a candidate of length 0 never rejects)
            rows = np.arange(idx.size)
            for own in (a, b, c):
                over[rows, own] = -np.inf
            worst = over.max(axis=1)
            ok = solved & (worst <= 0)
            vl = np.sqrt(_dot(v, v))
            bound = 8.0 * U64 * (L8[a] + L8[b] + L8[c]) / (2.0 * detn) + 4.0 * U64 * vl
            with np.errstate(all="ignore"):
                ratio = np.abs(worst) / bound
            m.plane_ratio = min(m.plane_ratio, float(ratio[solved].min(initial=np.inf)))
            counts = worst <= GUARD_FACTOR * bound  # accepted, or nearly: only for these does DET_TOL decide anything
            m.det = min(m.det, float((np.abs(detn[counts] - DET_TOL) / DET_TOL).min(initial=np.inf)))
            for t in np.flatnonzero(ok):
                w = v[t].astype(dt)
                for e in (a[t], b[t], c[t]):
                    verts[e].append(w)
                max_r2 = max(max_r2, _dot(w, w))
                m.bound = max(m.bound, float(bound[t]) + float(np.spacing(F32(vl[t]))))
    out = SimpleNamespace(is_face=np.zeros(K, bool), omega=np.zeros(K, dt), area=np.zeros(K, dt), weight=np.zeros(K, dt), length=l,
                          faces=[None] * K, too_many=False, nv=np.array([len(x) for x in verts], dtype=np.int64))
    for e in range(K):
        nv = int(out.nv[e])
        if nv > FACE_VERTICES:
            out.too_many = True
        if nv < 3 or nv > FACE_VERTICES:
            continue
        w = np.asarray(verts[e], dtype=dt)
        g = (w.sum(axis=0) * (dt(1) / dt(nv))).astype(dt)
        n = (d[e] / l[e]).astype(dt)
        t = np.zeros(3, dt)
        t[int(np.argmin(np.abs(n)))] = 1  # (argmin: the first on ties, x before y before z)
        u1 = _cross(n[None], t[None], dt)[0]
        u1 = (u1 / np.sqrt(_dot(u1, u1))).astype(dt)
        u2 = _cross(n[None], u1[None], dt)[0]
        r = (w - g[None]).astype(dt)
        w = w[np.argsort(np.arctan2(_dot(r, u2[None]), _dot(r, u1[None])).astype(dt), kind="stable")]
        w1 = np.roll(w, -1, axis=0)
        out.area[e] = (dt(0.5) * _dot(n[None], _cross((w - g[None]).astype(dt), (w1 - g[None]).astype(dt), dt))).astype(dt).sum(dtype=dt)
        gl, pl, ql = np.sqrt(_dot(g, g)).astype(dt), np.sqrt(_dot(w, w)).astype(dt), np.sqrt(_dot(w1, w1)).astype(dt)
        num = _dot(g[None], _cross(w, w1, dt))
        den = gl * pl * ql + _dot(g[None], w) * ql + _dot(g[None], w1) * pl + _dot(w, w1) * gl
        out.omega[e] = (dt(2) * np.arctan2(num, den).astype(dt)).astype(dt).sum(dtype=dt)
        out.is_face[e], out.faces[e] = True, w
    f = out.is_face
    with np.errstate(all="ignore"):
        top = out.omega[f].max() if f.any() else dt(0)
        if top > 0:  # (rule 4: a zero-area face's solid angle is rounding noise of either sign and weighs 0)
            out.weight[f] = (np.maximum(out.omega[f], dt(0)) / top).astype(dt)
    out.cn = int((f & (out.weight >= dt(tol))).sum())
    out.cn_eff, out.omega_sum = out.weight[f].sum(dtype=dt), out.omega[f].sum(dtype=dt)
    out.volume = (out.area[f] * l[f] * (dt(1) / dt(6))).astype(dt).sum(dtype=dt)
    out.max_radius = dt(np.sqrt(max_r2))
    residual = abs(float(out.omega_sum) - 4.0 * np.pi)
    out.open = bool(2.0 * float(out.max_radius) > float(dt(cutoff)) or not residual <= float(F32(CLOSURE_TOL)))
    m.weight = float(np.abs(out.weight[f].astype(np.float64) - float(F32(tol))).min(initial=np.inf))
    m.radius, m.closure = abs(2.0 * float(out.max_radius) - float(dt(cutoff))), abs(residual - float(F32(CLOSURE_TOL)))
    out.margins = m
    return out


def _is_guarded(m, cutoff_margin):
    return bool(m.weight > WEIGHT_GUARD and m.plane_ratio > GUARD_FACTOR and m.det > DET_GUARD and m.radius > GUARD_FACTOR * m.bound
                and m.closure > GUARD_FACTOR * CLOSURE_F32 and cutoff_margin > CUTOFF_GUARD)


def voronoi_reference(frac, lattice, counts, params=None, dtype=np.float64, keep_faces=False, exact_inputs=False):
    """Rules 0-6 in numpy, every operation in `dtype`, from the float32 inputs: frac [N,3], lattice [B,3,3], counts [B] atoms per
    crystal.  float64 is the yardstick; float32 the same arithmetic (the candidates' d2 then one float32 operation at a time, as
    the kernel forms them).  Returns a namespace of the eighteen outputs (RESULT_KEYS, reals of `dtype`) and, per atom, `margins`
    (a list of namespaces plane_ratio, det, radius, closure, weight, bound, cutoff; None where no cell was built), `guarded` [N]
    (module docstring: float32 decides every comparison of the atom as float64 does), `n_candidates` [N], `max_vertices` [N] (the
    most vertex copies on one plane of the atom, also where that is too many; -1 where rule 2 was not reached), `selected` (per
    atom the candidate indices, in (j, m) order, of the faces of weight >= tol: all cn of them; None where no cell was built);
    with keep_faces, `faces`: per atom a list of (j, (n_1, n_2, n_3), ordered vertices [k,3] relative to the atom, area, solid angle) of every face.
    exact_inputs (float64 only) takes frac and lattice as the float64 numbers they are, not as the float32 the kernel would see:
    an ideal structure whose ratios float32 cannot hold (hcp) stays ideal."""
    if exact_inputs:
        assert np.dtype(dtype) == np.float64
        frac, lattice = np.asarray(frac, dtype=np.float64).reshape(-1, 3), np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3)
        counts = [int(n) for n in counts]
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    else:
        frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    p_ = params if params is not None else VoronoiParams()
    dt = np.dtype(dtype).type
    B, N = len(counts), frac.shape[0]
    out = _empty_result(B, N, p_.max_faces, dt)
    out.margins, out.guarded, out.n_candidates, out.faces = [None] * N, np.zeros(N, bool), np.zeros(N, np.int64), [None] * N
    out.max_vertices, out.selected = np.full(N, -1, np.int64), [None] * N
    R = float(F32(p_.cutoff))
    r2 = dt(F32(np.float64(R) ** 2)) if dt == F32 else np.float64(F32(np.float64(R) ** 2))
    for b, n in enumerate(counts):
        L, f = lattice[b], frac[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        if dt == F32:
            _, q, bad = cb.cell_f32(L, p_.cutoff, 0.0, p_.max_shells)
        else:
            vol, q = cb.cell_f64(L.astype(np.float64), R)
            bad = not np.isfinite(vol) or not (q <= p_.max_shells).all()
        if bad:
            out.flags[b] = CELL
            continue
        if n == 0:
            out.flags[b] = EMPTY
            continue
        nk = [max(1, int(np.ceil(qk))) for qk in q]
        pos, g, centre, s = cb.positions_and_shifts(f.astype(dt), L.astype(dt), nk, dt)
        M = g.shape[0]
        flags = 0
        for i in range(n):
            A = first[b] + i
            disp = ((pos[:, None, :] + s[None, :, :]).astype(dt) - pos[i][None, None, :]).astype(dt).reshape(n * M, 3)
            sq = (disp * disp).astype(dt)
            d2 = ((sq[:, 0] + sq[:, 1]).astype(dt) + sq[:, 2]).astype(dt)
            near = d2 <= r2
            near[i * M + centre] = False
            e = np.flatnonzero(near)
            others = np.ones(n * M, bool)
            others[i * M + centre] = False
            cutoff_margin = float(np.abs(d2[others].astype(np.float64) / float(r2) - 1.0).min(initial=np.inf))
            out.n_candidates[A] = e.size
            aflags = OVERLAP if (d2[e] == 0).any() else 0
            if e.size > p_.max_candidates or aflags:
                aflags |= OVERFLOW if e.size > p_.max_candidates else 0
                out.atom_flags[A] = aflags
                flags |= aflags
                continue
            c = atom_cell(disp[e], d2[e], R, float(F32(p_.tol)), dt)
            out.max_vertices[A] = c.nv.max(initial=0)
            if c.too_many:
                out.atom_flags[A] = aflags | OVERFLOW
                flags |= aflags | OVERFLOW
                continue
            sel = np.flatnonzero(c.is_face & (c.weight >= dt(F32(p_.tol))))
            k = min(sel.size, p_.max_faces)
            out.cn[A], out.selected[A] = sel.size, sel
            out.neighbors[A, :k, 0], out.neighbors[A, :k, 1:] = e[sel[:k]] // M, g[e[sel[:k]] % M]
            out.face_weight[A, :k], out.face_solid_angle[A, :k] = c.weight[sel[:k]], c.omega[sel[:k]]
            out.face_area[A, :k], out.face_distance[A, :k] = c.area[sel[:k]], c.length[sel[:k]]
            out.volume[A], out.omega_sum[A], out.max_radius[A], out.cn_eff[A] = c.volume, c.omega_sum, c.max_radius, c.cn_eff
            aflags |= (OPEN if c.open else 0) | (TRUNCATED if sel.size > p_.max_faces else 0)
            out.atom_flags[A] = aflags
            flags |= aflags
            c.margins.cutoff = cutoff_margin
            out.margins[A], out.guarded[A] = c.margins, _is_guarded(c.margins, cutoff_margin)
            if keep_faces:
                out.faces[A] = [(int(e[k_] // M), tuple(int(x) for x in g[e[k_] % M]), c.faces[k_], float(c.area[k_]), float(c.omega[k_]))
                                for k_ in np.flatnonzero(c.is_face)]
        a0, a1 = first[b], first[b + 1]
        cn = out.cn[a0:a1]
        out.n_faces[b], out.min_cn[b], out.max_cn[b], out.flags[b] = cn.sum(), cn.min(), cn.max(), flags
        out.mean_cn[b] = dt(cn.sum()) / dt(n)
        out.mean_cn_eff[b] = out.cn_eff[a0:a1].sum(dtype=dt) / dt(n)
        out.volume_sum[b] = out.volume[a0:a1].sum(dtype=dt)
    return out


def scales(lattice, counts, params=None):
    """Per crystal the natural scales the measured bounds are relative to (module docstring): a dict of [B] arrays keyed like
    F32_DEVIATION (cn_eff's is 1: the deviation of the whole sum of weights was measured)."""
    lattice = np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3)
    p_ = params if params is not None else VoronoiParams()
    with np.errstate(all="ignore"):
        per_atom = np.abs(np.linalg.det(lattice)) / np.maximum(np.asarray(counts, dtype=np.float64), 1.0)
    one, R = np.ones(len(lattice)), float(F32(p_.cutoff))
    return {"face_solid_angle": 4.0 * np.pi * one, "omega_sum": 4.0 * np.pi * one, "face_weight": one, "cn_eff": one, "volume": per_atom,
            "face_area": per_atom ** (2.0 / 3.0), "max_radius": R * one, "face_distance": R * one}
