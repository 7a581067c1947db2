"""Duplicate detection of generated crystals: a reduced formula and a pair-distribution fingerprint per crystal
(arreau_crystal_fingerprint) and the all-pairs match of a set with itself or with another set (arreau_fingerprint_match), both in
arreau_amd/csrc/fingerprint.hip; the rules are written out in include/arreau_hip.h.  Here: the parameters and their validation,
the flag constants, the entry points that need no engine (`fingerprint`, `match`), `unique_sample_result` for a SampleResult or a
loaded file, the statistics lines, and numpy restatements for the tests -- `fingerprint_reference_f64` (float64 arithmetic from
the same float32 inputs, image range one shell wider than the kernel's), `fingerprint_reference_f32` (numpy float32, every sum in
the naive order of the rule) and `match_reference`.  The restatements need numpy alone.

The rule in short (Oganov & Valle, J. Chem. Phys. 130, 104504 (2009); the normalisation is taken at the bin centre): contacts
enumerated as the screen enumerates them out to r_cut = r_max + 5 sigma; a contact at R between species ranks A <= B adds
c g(R_k - R) to every bin k of component (A, B), c = 2 for A == B; F_AB[k] = V S_AB[k] / (4 pi R_k^2 N_A N_B) - 1; the stored row is
sqrt(w_AB) F_AB[k] / |F|_w with w_AB = N_A N_B / N^2; d(x, y) = (1 - f_x . f_y) / 2 between crystals of one reduced formula.

float32 against float64.  The kernel's arithmetic is the float32 restatement's; its order of the norm's sum and its exponential
(one v_exp_f32 on a base-2 argument) differ from numpy's.  Over the cases of tests/uniqueness_cases.py the float32 restatement
deviates from the float64 one by at most F32_DEVIATION_FHAT = 2.4e-6 in a component of the row (measured 2.365e-6) and
F32_DEVIATION_D = 5.4e-7 in a distance (measured 5.32e-7; both on the CPU, asserted in tests/test_uniqueness_cpu.py); the kernel
is allowed four times that: FHAT_BOUND = 9.6e-6, D_BOUND = 2.16e-6."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from .screening import MAX_SHELLS, distance_bound

NONFINITE, CELL, MANY_SPECIES, EMPTY = 1, 2, 4, 8
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (MANY_SPECIES, "MANY_SPECIES"), (EMPTY, "EMPTY"))
MAX_SPECIES, BINS, COMPONENTS = 8, 64, 36
ROW = COMPONENTS * BINS
STAGED_ATOMS = cb.STAGED_ATOMS
LIST, DRAIN = 1024, 768   # fingerprint.hip: FP_LIST, FP_DRAIN -- the contact list is drained once it holds more than DRAIN
MATCH_TILE = 16           # fingerprint.hip: MATCH_TILE
UNIQUE_KEYS = ("duplicate_of", "distance", "nearest", "nearest_distance", "flags", "unique")
DEFAULT_TOLERANCE = 0.01
# measured: the largest deviation of fingerprint_reference_f32 from fingerprint_reference_f64 over tests/uniqueness_cases.py
F32_DEVIATION_FHAT, F32_DEVIATION_D = 2.4e-6, 5.4e-7  # measured 2.365e-6 and 5.32e-7
FHAT_BOUND, D_BOUND = 4 * F32_DEVIATION_FHAT, 4 * F32_DEVIATION_D
F32 = np.float32


@dataclass(frozen=True)
class FingerprintParams:
    """The fingerprint's radial grid (r_max in A, n_bins <= 64), its smearing sigma in A, the cap on periodic images per axis
    and the match tolerance on d = (1 - cos) / 2.  The defaults are starting values, not claims about any model."""
    r_max: float = 6.0
    n_bins: int = BINS
    sigma: float = 0.1
    tolerance: float = DEFAULT_TOLERANCE
    max_shells: int = MAX_SHELLS

    def __post_init__(self):
        for name in ("r_max", "sigma", "tolerance"):
            v = getattr(self, name)
            if not isinstance(v, Real) or isinstance(v, bool):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not math.isfinite(v):
                raise ValueError(f"{name} must be finite, got {v}")
            object.__setattr__(self, name, float(v))
        if not self.r_max > 0.0 or not self.sigma > 0.0:
            raise ValueError(f"r_max and sigma must be > 0, got {self.r_max} and {self.sigma}")
        check_tolerance(self.tolerance)
        for name, top in (("n_bins", BINS), ("max_shells", MAX_SHELLS)):
            v = getattr(self, name)
            if not isinstance(v, Integral) or isinstance(v, bool) or not 1 <= int(v) <= top:
                raise ValueError(f"{name} must lie in 1..{top}, got {v!r}")
            object.__setattr__(self, name, int(v))

    @property
    def r_cut(self):
        """float32(double(float32 r_max) + 5 double(float32 sigma)), as the C entry point forms it."""
        return F32(np.float64(F32(self.r_max)) + 5.0 * np.float64(F32(self.sigma)))


def check_tolerance(tolerance):
    if not isinstance(tolerance, Real) or isinstance(tolerance, bool) or not 0.0 <= float(tolerance) <= 1.0:
        raise ValueError(f"tolerance must lie in [0, 1], got {tolerance!r}")
    return float(tolerance)


def resolve(unique):
    """sample(unique=...): None / False -> None, True -> the defaults, a FingerprintParams -> itself."""
    return cb.resolve(unique, FingerprintParams, "unique")


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


# ------------------------------------------------------------------------------------------------------- the device calls
def fingerprint(frac, lattice, offsets, types, params=None):
    """Fingerprint a batch on the GPU without an engine (arreau_crystal_fingerprint, one launch).  frac [N,3] float32, lattice
    [B,3,3] float32 (rows a, b, c), offsets [B+1] int32 and types [N] int32 (species ids) are contiguous tensors on one cuda
    device.  Returns a dict of device tensors: fingerprint [B, 2304], species [B,8], counts [B,8], flags [B].  Does not
    synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else FingerprintParams()
    dev, B, N = cb.check_batch("fingerprint", frac, lattice, offsets, types)
    i32 = dict(device=dev, dtype=torch.int32)
    out = {"fingerprint": torch.empty((B, ROW), device=dev, dtype=torch.float32), "species": torch.empty((B, MAX_SPECIES), **i32),
           "counts": torch.empty((B, MAX_SPECIES), **i32), "flags": torch.empty(B, **i32)}
    c = _hip.FingerprintParamsC(p.r_max, p.sigma, p.n_bins, p.max_shells)
    r = _set_struct(out)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_fingerprint(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(offsets), B, N,
                                                         ctypes.byref(c), ctypes.byref(r), _hip.stream_ptr(dev)),
                   "arreau_crystal_fingerprint")
    return out


def _set_struct(s):
    from .. import _hip
    B = int(s["flags"].shape[0])
    return _hip.FingerprintResultC(*[_hip.ptr(s[k]).value if B else None for k in ("fingerprint", "species", "counts", "flags")])


def match(x, y=None, tolerance=DEFAULT_TOLERANCE):
    """Match a fingerprinted set (the dict of `fingerprint`) with itself (y None: only earlier crystals are candidates) or with
    another set (arreau_fingerprint_match, one launch).  Returns a dict of device tensors [Bx]: duplicate_of, distance, nearest,
    nearest_distance, flags (x's) and `unique` = duplicate_of < 0 and flags == 0 -- in two-set mode the same expression says
    the crystal has no match in y.  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    tolerance = check_tolerance(tolerance)
    dev = x["fingerprint"].device
    for s in (x,) if y is None else (x, y):
        B = int(s["flags"].shape[0])
        for k, shape, dtype in (("fingerprint", (B, ROW), torch.float32), ("species", (B, MAX_SPECIES), torch.int32),
                                ("counts", (B, MAX_SPECIES), torch.int32), ("flags", (B,), torch.int32)):
            t = s[k]
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous() or dev.type != "cuda":
                raise ValueError(f"match: {k} must be a contiguous {dtype} tensor of shape {shape} on one cuda device")
    Bx = int(x["flags"].shape[0])
    out = {"duplicate_of": torch.empty(Bx, device=dev, dtype=torch.int32), "distance": torch.empty(Bx, device=dev, dtype=torch.float32),
           "nearest": torch.empty(Bx, device=dev, dtype=torch.int32), "nearest_distance": torch.empty(Bx, device=dev, dtype=torch.float32)}
    r = _hip.MatchResultC(*[_hip.ptr(out[k]).value if Bx else None for k in ("duplicate_of", "distance", "nearest", "nearest_distance")])
    xs = _set_struct(x)
    ys = _set_struct(y) if y is not None else None
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_fingerprint_match(ctypes.byref(xs), Bx, ctypes.byref(ys) if ys is not None else None,
                                                       int(y["flags"].shape[0]) if y is not None else 0, tolerance, ctypes.byref(r),
                                                       _hip.stream_ptr(dev)), "arreau_fingerprint_match")
    out["flags"] = x["flags"]
    out["unique"] = (out["duplicate_of"] < 0) & (x["flags"] == 0)
    return out


def unique_batch(frac, lattice, offsets, types, params=None):
    """Both launches on one device state: the uniqueness dict (`match` of the batch with itself) as device tensors."""
    p = params if params is not None else FingerprintParams()
    return match(fingerprint(frac, lattice, offsets, types, p), None, p.tolerance)


def uniqueness_to_numpy(u):
    """The UNIQUE_KEYS of the dict of `match` as host numpy arrays (synchronises)."""
    return {k: u[k].cpu().numpy() for k in UNIQUE_KEYS}


def unique_sample_result(result, params=None, against=None, device="cuda"):
    """Uniqueness of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32 and its atomic
    numbers taken as species ids: the UNIQUE_KEYS as numpy arrays.  With `against` (another SampleResult, e.g. a training set)
    the set is matched with that one instead: `unique` then says the crystal has no match there (it is novel)."""
    p = params if params is not None else FingerprintParams()
    x = fingerprint(*cb.upload(result, device), p)
    y = fingerprint(*cb.upload(against, device), p) if against is not None else None
    return uniqueness_to_numpy(match(x, y, p.tolerance))


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(u, rank=0):
    """What a summary line needs, of one rank's (or the whole set's) uniqueness arrays."""
    flags, unique = np.asarray(u["flags"]).reshape(-1), np.asarray(u["unique"]).reshape(-1).astype(bool)
    nd = np.asarray(u["nearest_distance"], dtype=np.float64).reshape(-1)
    nd = nd[np.isfinite(nd)]
    return {"rank": cb.rank_of(rank), "attempted": int(flags.size), "unique": int(unique.sum()),
            "duplicates": int((np.asarray(u["duplicate_of"]).reshape(-1) >= 0).sum()), "flagged": int((flags != 0).sum()),
            "nearest_min": float(nd.min()) if nd.size else None, "nearest_median": float(np.median(nd)) if nd.size else None}


def format_stats(st, word="unique") -> str:
    """'unique rank 0: unique 14 / attempted 16; duplicates 1, flagged 1; nearest_distance min 0.0012 median 0.21'."""
    line = f"{word} {cb.who(st)}: {word} {st['unique']} / attempted {st['attempted']}; " \
           f"{'duplicates' if word == 'unique' else 'matched'} {st['duplicates']}, flagged {st['flagged']}"
    if st["nearest_min"] is not None:
        line += f"; nearest_distance min {st['nearest_min']:.4g} median {st['nearest_median']:.4g}"
    return line


# ------------------------------------------------------------------------------------------------- the numpy restatements
def _formula(t):
    """(species [K], counts [K], ranks [n]) of one crystal's species ids."""
    species, ranks, counts = np.unique(np.asarray(t, dtype=np.int64), return_inverse=True, return_counts=True)
    return species, counts, ranks.reshape(-1)


def _empty(B, dtype):
    return SimpleNamespace(fingerprint=np.zeros((B, ROW), dtype), species=np.full((B, MAX_SPECIES), -1, np.int32),
                           counts=np.zeros((B, MAX_SPECIES), np.int32), flags=np.zeros(B, np.int32))


def _components(ranks, i, j):
    A, Bq = np.minimum(ranks[i], ranks[j]), np.maximum(ranks[i], ranks[j])
    return Bq * (Bq + 1) // 2 + A, A == Bq


def fingerprint_reference_f32(frac, lattice, counts, types, params=None):
    """The kernel's rule in numpy float32: the screen restatement's float32 contacts, then every sum in the rule's naive order
    (a cell adds its contacts in enumeration order; the norm adds component by component, bin by bin).  numpy's exp stands where
    the kernel has one v_exp_f32.  Returns a namespace fingerprint [B, 2304] float32, species, counts [B,8], flags [B]."""
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    p = params if params is not None else FingerprintParams()
    out = _empty(len(counts), F32)
    r_cut = p.r_cut
    rc2 = F32(np.float64(r_cut) ** 2)
    sigma = np.float64(F32(p.sigma))
    inv2s2, gnorm = F32(1.0 / (2.0 * sigma * sigma)), F32(1.0 / (sigma * math.sqrt(2.0 * math.pi)))
    Rk = ((np.arange(BINS, dtype=F32) + F32(0.5)) * (F32(p.r_max) / F32(p.n_bins))).astype(F32)
    for b, n in enumerate(counts):
        L, f, t = lattice[b], frac[first[b]:first[b + 1]], types[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        species, cnt, ranks = _formula(t)
        vol, q, bad = cb.cell_f32(L, r_cut, 0.0, p.max_shells)
        flags = (EMPTY if n == 0 else 0) | (MANY_SPECIES if len(species) > MAX_SPECIES else 0) | (CELL if bad or not vol > 0 else 0)
        if flags:
            out.flags[b] = flags
            continue
        nk = [max(1, int(np.ceil(qk))) for qk in q]
        pos, g, centre, s = cb.positions_and_shifts(f, L, nk, F32)
        S = np.zeros((COMPONENTS, BINS), F32)
        for i, j, m, d2 in cb.contacts(pos, s, centre, F32):
            keep = d2 < rc2
            R = np.sqrt(d2[keep]).astype(F32)
            comp, same = _components(ranks, i[keep], j[keep])
            x = (Rk[None, :] - R[:, None]).astype(F32)
            val = np.exp(-((x * x).astype(F32) * inv2s2).astype(F32)).astype(F32)
            np.add.at(S, comp, np.where(same[:, None], val + val, val).astype(F32))  # unbuffered: one addition at a time, in order
        K = len(species)
        pref = F32(F32(vol * gnorm) / F32(4.0 * math.pi))
        fn = F32(n)
        row, wsq = np.zeros((COMPONENTS, BINS), F32), np.zeros((COMPONENTS, BINS), F32)
        for Bq in range(K):
            for A in range(Bq + 1):
                c = Bq * (Bq + 1) // 2 + A
                na, nb = F32(cnt[A]), F32(cnt[Bq])
                wt = F32(F32(na * nb) / F32(fn * fn))
                row[c, :p.n_bins] = ((S[c] * pref).astype(F32) / (((Rk * Rk).astype(F32) * na).astype(F32) * nb).astype(F32) - F32(1))[:p.n_bins]
                wsq[c, :p.n_bins] = wt
        terms = ((wsq * row).astype(F32) * row).astype(F32).reshape(-1)
        norm2 = np.add.accumulate(terms, dtype=F32)[-1]
        if norm2 > 0:
            out.fingerprint[b] = ((np.sqrt(wsq).astype(F32) * row).astype(F32) * F32(F32(1) / np.sqrt(norm2))).reshape(-1)
        out.species[b, :K], out.counts[b, :K] = species, cnt // np.gcd.reduce(cnt)
    return out


def fingerprint_reference_f64(frac, lattice, counts, types, params=None, widen=1, details=False):
    """The same rule in float64 from the same float32 inputs; the image range is n_k + `widen` per axis (one shell wider than
    the kernel's by default).  details=True adds `bound` [B] (screening.distance_bound of the crystal), `near_cut` [B] (contacts
    whose distance lies within that bound of r_cut: float32 may disagree on whether they count) and `n_contacts` [B]."""
    frac, lattice, counts, types, first = cb.inputs(frac, lattice, counts, types)
    p = params if params is not None else FingerprintParams()
    B = len(counts)
    out = _empty(B, np.float64)
    out.bound, out.near_cut, out.n_contacts = np.full(B, np.nan), np.zeros(B, np.int64), np.zeros(B, np.int64)
    r_cut, sigma = float(p.r_cut), float(F32(p.sigma))
    Rk = (np.arange(BINS) + 0.5) * (float(F32(p.r_max)) / p.n_bins)
    for b, n in enumerate(counts):
        L, f, t = lattice[b].astype(np.float64), frac[first[b]:first[b + 1]].astype(np.float64), types[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        species, cnt, ranks = _formula(t)
        vol, q = cb.cell_f64(L, r_cut)
        bad = not vol > 0 or not np.isfinite(vol) or not (q <= p.max_shells).all()
        flags = (EMPTY if n == 0 else 0) | (MANY_SPECIES if len(species) > MAX_SPECIES else 0) | (CELL if bad else 0)
        if flags:
            out.flags[b] = flags
            continue
        nk = np.maximum(1, np.ceil(q).astype(np.int64))
        out.bound[b] = distance_bound(L, nk)
        pos, g, centre, s = cb.positions_and_shifts(f, L, nk + int(widen), np.float64)
        S = np.zeros((COMPONENTS, BINS))
        for i, j, m, d2 in cb.contacts(pos, s, centre, np.float64):
            R = np.sqrt(d2)
            out.near_cut[b] += int((np.abs(R - r_cut) <= out.bound[b]).sum())
            keep = R < r_cut
            R = R[keep]
            out.n_contacts[b] += R.size
            comp, same = _components(ranks, i[keep], j[keep])
            x = Rk[None, :] - R[:, None]
            val = np.exp(-x * x / (2.0 * sigma * sigma)) / (sigma * math.sqrt(2.0 * math.pi)) * np.where(same, 2.0, 1.0)[:, None]
            np.add.at(S, comp, val)
        K = len(species)
        row, wt = np.zeros((COMPONENTS, BINS)), np.zeros((COMPONENTS, BINS))
        for Bq in range(K):
            for A in range(Bq + 1):
                cc = Bq * (Bq + 1) // 2 + A
                row[cc, :p.n_bins] = (vol * S[cc] / (4.0 * math.pi * Rk * Rk * cnt[A] * cnt[Bq]) - 1.0)[:p.n_bins]
                wt[cc, :p.n_bins] = cnt[A] * cnt[Bq] / float(n) ** 2
        norm2 = float((wt * row * row).sum())
        if norm2 > 0:
            out.fingerprint[b] = (np.sqrt(wt) * row / math.sqrt(norm2)).reshape(-1)
        out.species[b, :K], out.counts[b, :K] = species, cnt // np.gcd.reduce(cnt)
    if not details:
        del out.bound, out.near_cut, out.n_contacts
    return out


def _get(s, k):
    return np.asarray(s[k] if isinstance(s, dict) else getattr(s, k))


def match_reference(x, y=None, tolerance=DEFAULT_TOLERANCE):
    """The match rule in float64 on fingerprinted sets (namespaces or dicts of fingerprint, species, counts, flags).  Returns a
    namespace duplicate_of, nearest (int32), distance, nearest_distance (float64), flags, unique, and the full tables `d`
    [Bx, By] and `candidate` [Bx, By] (comparable, and earlier in self mode)."""
    tolerance = check_tolerance(tolerance)
    self_mode = y is None
    y = x if self_mode else y
    fx, fy = _get(x, "fingerprint").astype(np.float64), _get(y, "fingerprint").astype(np.float64)
    Bx, By = fx.shape[0], fy.shape[0]
    # (row by row with numpy's own sum: equal rows give equal bits, which a BLAS product does not promise)
    d = np.array([0.5 * (1.0 - (fx[r][None, :] * fy).sum(axis=1)) for r in range(Bx)]).reshape(Bx, By)
    ok = (_get(x, "flags") == 0)[:, None] & (_get(y, "flags") == 0)[None, :]
    ok &= (_get(x, "species")[:, None, :] == _get(y, "species")[None, :, :]).all(-1)
    ok &= (_get(x, "counts")[:, None, :] == _get(y, "counts")[None, :, :]).all(-1)
    if self_mode:
        ok &= np.arange(By)[None, :] < np.arange(Bx)[:, None]
    out = SimpleNamespace(duplicate_of=np.full(Bx, -1, np.int32), nearest=np.full(Bx, -1, np.int32), distance=np.full(Bx, np.inf),
                          nearest_distance=np.full(Bx, np.inf), flags=_get(x, "flags").astype(np.int32), d=d, candidate=ok)
    for r in range(Bx):
        cand = np.nonzero(ok[r])[0]
        if cand.size:
            near = cand[np.argmin(d[r, cand])]  # the first of equal minima: the smaller index
            out.nearest[r], out.nearest_distance[r] = near, d[r, near]
            hit = cand[d[r, cand] <= tolerance]
            if hit.size:
                out.duplicate_of[r], out.distance[r] = hit[0], d[r, hit[0]]
    out.unique = (out.duplicate_of < 0) & (out.flags == 0)
    return out
