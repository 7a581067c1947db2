"""Powder X-ray diffraction patterns of generated crystals: per crystal the pattern on a fixed 2 theta grid -- every reciprocal
lattice point of the range as a Gaussian of its Lorentz-polarisation-weighted |F|^2 / V^2 --, the number of lattice points kept,
the volume and the summed amplitudes (arreau_crystal_xrd, arreau_amd/csrc/xrd.hip; the rules are written out in
include/arreau_hip.h).  The one observable a generated crystal is compared with in a laboratory, and a signature that does not
depend on the description: the same pattern in any basis, in the primitive cell, in the conventional cell and in any supercell,
which makes it the cross-check on reduce_cell, conventional_cell, symmetrize and unique.  Here: the parameters and their
validation, the flag constants, `derived` (what the host works out of the parameters, in float64) and `grid`, the entry point that
needs no engine (`xrd`), the host additions (`sample_arrays`: max_intensity, two_theta_peak and the grid's five parameters per
crystal), the statistics, `distance` ((1 - cos) / 2, the fingerprint's measure) and `xrd_reference`, a numpy restatement of rules
1-8 -- in float64 the yardstick of the tests, which also reports each crystal's margin to the d* cuts and its reflections; in
float32 the kernel's split of precisions and its operation order with numpy's sine, cosine and exp.  Needs numpy alone at import.

What this is not: no form-factor tables (the atoms are point scatterers of amplitude Z, or 1, or the caller's weights, so
relative intensities are those of Z-weighted points), no anomalous dispersion, no peak list, no merging of equivalent
reflections, no preferred orientation, no K alpha 2, no neutron or electron scattering lengths beyond the caller's own weights.

The float32 bound is MEASURED, not derived (F32_DEVIATION below): the largest |P_32 - P_64| / max(P_64) of the float32 mode
against float64 over every batch of tests/xrd_cases.py, and the tests allow the device BOUND_FACTOR = 16 times the largest of
them (voronoi.BOUND_FACTOR: the margin this tree gives a measured float32 bound) for its sincospif and expf and its fused
float64 operations.  It is never tuned from the kernel's output.  The derived part: the reduced phase t - rint(t) carries at most
2 pi (|h| + |k| + |l| + 2) 2^-24 radians (three products, two sums and the wrap, each within 2^-24 of a term of size at most
|h|, |k|, |l| or 1), which grows with max_index: 2.4e-5 radians at |h| = |k| = |l| = 21, 1.4e-4 at 127."""
import math
from dataclasses import dataclass, replace
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from .voronoi import BOUND_FACTOR

NONFINITE, CELL, EMPTY, RANGE = 1, 2, 4, 8
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (RANGE, "RANGE"))
MAX_POINTS, MAX_INDEX, MAX_TWO_THETA, MAX_WINDOW = 4096, 127, 160.0, 10.0  # include/arreau_hip.h: ARREAU_XRD_*
ROUND = 256  # box entries per round: one per thread of the workgroup
SCATTERING = ("Z", "unit", "weights")  # atomic numbers, 1, or the caller's own [N] float32 array (the engine-free entry point)
RESULT_KEYS = ("pattern", "n_reflections", "volume", "weight_sum", "flags")  # arreau_xrd_result, in its order
GRID_KEYS = ("wavelength", "two_theta_min", "two_theta_max", "n_points", "fwhm")  # the columns of `grid`
STORED_KEYS = RESULT_KEYS + ("max_intensity", "two_theta_peak", "grid")  # what SampleResult.xrd and a crystals file hold
F32 = np.float32
# measured by tools/exp/xrd_f32_deviation.py: the largest |P_32 - P_64| / max(P_64) of xrd_reference's float32 mode against its
# float64 mode over each batch of tests/xrd_cases.py (BATCHES, in its order); the tests allow BOUND_FACTOR times the largest
F32_DEVIATION = {"textbook": 1.29e-07, "cscl unit": 2.1e-07, "invariance": 2.79e-07, "ragged": 5.53e-07, "large": 5.93e-07, "flags": 1.12e-07,
                 "points 2": 4.57e-07, "points 257": 2.92e-07, "points 4096": 2.67e-07, "narrow": 3.7e-07, "wide": 4.14e-07, "b_iso": 2.77e-07}
F32_BOUND = BOUND_FACTOR * max(F32_DEVIATION.values())  # 9.5e-6 of the pattern's maximum
MARGIN_GUARD = 1e-9  # a crystal whose nearest lattice point lies closer than this (relative) to a d* cut has no exact n_reflections


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class XrdParams:
    """wavelength in A (1.54184: Cu K alpha); the grid: n_points (2..4096) equally spaced 2 theta values from two_theta_min to
    two_theta_max in degrees, ends included, 0 <= min < max <= 160 (5, 90, 1701: 0.05 degree steps); fwhm in degrees of every
    reflection's Gaussian (0.2), 6 sigma = 2.548 fwhm at most 10 degrees; b_iso in A^2, one Debye-Waller B for every atom (0);
    scattering: "Z" (the atomic numbers: the forward-scattering limit of the X-ray form factor), "unit" (1) or "weights" (the
    caller's own [N] float32 array, at `xrd` alone); max_index: the largest |h_k| the box may need (1..127; 64): a crystal that
    needs more is flagged RANGE.  Starting values, not claims."""
    wavelength: float = 1.54184
    two_theta_min: float = 5.0
    two_theta_max: float = 90.0
    n_points: int = 1701
    fwhm: float = 0.2
    b_iso: float = 0.0
    scattering: str = "Z"
    max_index: int = 64

    def __post_init__(self):
        for name in ("wavelength", "two_theta_min", "two_theta_max", "fwhm", "b_iso"):
            v = getattr(self, name)
            if not isinstance(v, Real) or isinstance(v, bool) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if not self.wavelength > 0.0:
            raise ValueError(f"wavelength must be > 0, got {self.wavelength}")
        if not 0.0 <= self.two_theta_min < self.two_theta_max <= MAX_TWO_THETA:
            raise ValueError(f"0 <= two_theta_min < two_theta_max <= {MAX_TWO_THETA:g} is required, got {self.two_theta_min}, {self.two_theta_max}")
        for name, lo, hi in (("n_points", 2, MAX_POINTS), ("max_index", 1, MAX_INDEX)):
            v = getattr(self, name)
            if not isinstance(v, Integral) or isinstance(v, bool) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must lie in {lo}..{hi}, got {v!r}")
            object.__setattr__(self, name, int(v))
        if not self.fwhm > 0.0:
            raise ValueError(f"fwhm must be > 0, got {self.fwhm}")
        sigma = self.fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        if not 0.0 < 6.0 * sigma <= MAX_WINDOW:
            raise ValueError(f"fwhm: 6 sigma = {6.0 * sigma:g} degrees must lie in (0, {MAX_WINDOW:g}] (fwhm <= {MAX_WINDOW / 6.0 * 2.0 * math.sqrt(2.0 * math.log(2.0)):.4f})")
        if not self.b_iso >= 0.0:
            raise ValueError(f"b_iso must be >= 0, got {self.b_iso}")
        if self.scattering not in SCATTERING:
            raise ValueError(f"scattering must be one of {SCATTERING}, got {self.scattering!r}")
        d = derived(self)
        if not (math.isfinite(d.dhi * d.dhi) and d.dhi * d.dhi > 0.0 and d.step > 0.0 and math.isfinite(1.0 / d.step)):
            raise ValueError("wavelength or grid outside what float64 holds")


def resolve(xrd):
    """sample(xrd=...): None / False -> None, True -> the defaults, an XrdParams -> itself (scattering "Z" or "unit": the sampler
    has no array of weights to give)."""
    p = cb.resolve(xrd, XrdParams, "xrd")
    if p is not None and p.scattering == "weights":
        raise ValueError('xrd: scattering "weights" is for the entry point that takes the array (xrd.xrd); use "Z" or "unit"')
    return p


def derived(p):
    """Rule 1, float64, as the library's entry point works it out: sigma, six_sigma, norm = 1 / (sigma sqrt(2 pi)), the range lo,
    hi in degrees, its d* cuts dlo, dhi, and the grid's step."""
    sigma = p.fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    lo, hi = max(p.two_theta_min - 6.0 * sigma, 0.0), p.two_theta_max + 6.0 * sigma
    rad = math.pi / 180.0
    return SimpleNamespace(sigma=sigma, six_sigma=6.0 * sigma, norm=1.0 / (sigma * math.sqrt(2.0 * math.pi)), lo=lo, hi=hi,
                           dlo=2.0 * math.sin(0.5 * lo * rad) / p.wavelength, dhi=2.0 * math.sin(0.5 * hi * rad) / p.wavelength,
                           step=(p.two_theta_max - p.two_theta_min) / (p.n_points - 1))


def grid(params=None):
    """The 2 theta values of a pattern's columns in degrees, float64 [n_points]: two_theta_min + p step, the last two_theta_max.
    `params`: an XrdParams, None for the defaults, or one row of a stored `grid` array (GRID_KEYS)."""
    if params is None:
        params = XrdParams()
    if not isinstance(params, XrdParams):
        row = np.asarray(params, dtype=np.float64).reshape(-1)
        params = SimpleNamespace(two_theta_min=float(row[1]), two_theta_max=float(row[2]), n_points=int(round(row[3])))
    n = params.n_points
    g = params.two_theta_min + np.arange(n, dtype=np.float64) * ((params.two_theta_max - params.two_theta_min) / (n - 1))
    g[-1] = params.two_theta_max
    return g


def grid_row(p):
    """The five grid-defining parameters (GRID_KEYS) as float64 [5]."""
    return np.array([p.wavelength, p.two_theta_min, p.two_theta_max, float(p.n_points), p.fwhm], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------- the device call
def xrd(frac, lattice, offsets, weights_or_atomic_numbers, params=None):
    """The powder patterns of a batch on the GPU without an engine (arreau_crystal_xrd, one launch).  frac [N,3] float32, lattice
    [B,3,3] float32 (rows a, b, c) and offsets [B+1] int32 are contiguous tensors on one cuda device; the fourth argument is a
    tensor [N] on it: with scattering "Z" the atomic numbers (any integer or float dtype), with "weights" the amplitudes
    themselves (float32), with "unit" it is not read and may be None.  Returns a dict of device tensors (RESULT_KEYS): pattern
    [B, n_points] float32; n_reflections, flags int32 and volume, weight_sum float32 [B].  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else XrdParams()
    dev, B, N = cb.check_batch("xrd", frac, lattice, offsets, None, types_optional=True)
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    if p.scattering == "unit":
        weights = torch.ones(N, **f32)
    else:
        w = weights_or_atomic_numbers
        if w is None or tuple(w.shape) != (N,) or w.device != dev or (p.scattering == "weights" and w.dtype != torch.float32):
            raise ValueError(f"xrd: scattering {p.scattering!r} needs a [{N}] tensor on the cuda device of frac"
                             + (" of dtype float32" if p.scattering == "weights" else ""))
        weights = w.to(torch.float32).contiguous()
    out = {"pattern": torch.empty((B, p.n_points), **f32), "n_reflections": torch.empty(B, **i32), "volume": torch.empty(B, **f32),
           "weight_sum": torch.empty(B, **f32), "flags": torch.empty(B, **i32)}
    c = _hip.XrdParamsC(p.wavelength, p.two_theta_min, p.two_theta_max, p.fwhm, p.b_iso, p.n_points, p.max_index)
    r = _hip.XrdResultC(*[_hip.ptr(out[k]).value if out[k].numel() else None for k in RESULT_KEYS])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_xrd(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(offsets), _hip.ptr(weights), B, N,
                                                 ctypes.byref(c), ctypes.byref(r), _hip.stream_ptr(dev)), "arreau_crystal_xrd")
    return out


def result_to_numpy(result):
    """The dict of `xrd` as host numpy arrays (synchronises)."""
    return cb.to_numpy(result)


def sample_arrays(result, params=None):
    """What SampleResult.xrd and a crystals file hold (STORED_KEYS) of a `result_to_numpy` dict: its arrays, max_intensity [B]
    (the pattern's largest value; NaN for a flagged crystal), two_theta_peak [B] (the grid value there, the first on ties) and
    grid [B, 5], the five grid-defining parameters (GRID_KEYS) once per crystal: the 2 theta values are `grid(row)`."""
    p = params if params is not None else XrdParams()
    out = {k: np.asarray(result[k]) for k in RESULT_KEYS}
    pattern = out["pattern"].reshape(-1, p.n_points)
    B = pattern.shape[0]
    blank = np.isnan(pattern).any(axis=1)
    at = np.where(blank, 0, np.argmax(np.where(np.isnan(pattern), -np.inf, pattern), axis=1)) if B else np.zeros(0, np.int64)
    out["pattern"] = pattern
    out["max_intensity"] = np.where(blank, np.nan, pattern[np.arange(B), at]).astype(np.float32)
    out["two_theta_peak"] = np.where(blank, np.nan, grid(p)[at])
    out["grid"] = np.tile(grid_row(p)[None, :], (B, 1))
    return out


def host_weights(atomic_numbers, params=None):
    """The amplitudes [N] float32 of a result's atoms under `params`: the atomic numbers, or ones."""
    p = params if params is not None else XrdParams()
    z = np.rint(np.asarray(atomic_numbers, dtype=np.float64).reshape(-1))
    if p.scattering == "weights":
        raise ValueError('xrd: scattering "weights" is for the entry point that takes the array (xrd.xrd)')
    return (np.ones_like(z) if p.scattering == "unit" else z).astype(np.float32)


def for_weights(p):
    """The parameters of the launch that is given `host_weights(.., p)` as its amplitudes."""
    return p if p.scattering == "unit" else replace(p, scattering="weights")


def xrd_sample_result(result, params=None, device="cuda"):
    """The powder patterns of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32: the dict
    of `sample_arrays`."""
    import torch
    p = params if params is not None else XrdParams()
    frac, lattice, off, _ = cb.upload(result, device)
    w = torch.as_tensor(host_weights(result.atomic_numbers, p), device=frac.device)
    return sample_arrays(result_to_numpy(xrd(frac, lattice, off, w, for_weights(p))), p)


# ------------------------------------------------------------------------------------------------------------ the measure
def distance(p, q) -> float:
    """(1 - cos(p, q)) / 2 of two patterns on one grid, the fingerprint's measure: 0 for equal shapes whatever their scale, 1/2
    for patterns without a common peak.  NaN when either is blank or all zero."""
    p, q = np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(q, dtype=np.float64).reshape(-1)
    if p.shape != q.shape:
        raise ValueError("xrd.distance: the patterns lie on different grids")
    with np.errstate(all="ignore"):
        return float(0.5 * (1.0 - np.dot(p, q) / (np.sqrt(np.dot(p, p)) * np.sqrt(np.dot(q, q)))))


def distance_matrix(patterns, others=None):
    """distance of every row of `patterns` [B, n] to every row of `others` [T, n] (itself when None): float64 [B, T]."""
    a = np.asarray(patterns, dtype=np.float64)
    b = a if others is None else np.asarray(others, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("xrd.distance_matrix: the patterns lie on different grids")
    with np.errstate(all="ignore"):
        na, nb = np.sqrt((a * a).sum(axis=1)), np.sqrt((b * b).sum(axis=1))
        return 0.5 * (1.0 - (a @ b.T) / (na[:, None] * nb[None, :]))


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the crystals with a pattern, their summed
    n_reflections, the sum, minimum and maximum of their two_theta_peak, the count per flag."""
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    peak = np.asarray(result["two_theta_peak"], dtype=np.float64).reshape(-1)
    ok = (flags == 0) & ~np.isnan(peak)
    return {"rank": cb.rank_of(rank), "crystals": int(flags.size), "patterns": int(ok.sum()),
            "n_reflections": int(np.asarray(result["n_reflections"], dtype=np.int64).reshape(-1)[ok].sum()),
            "peak_sum": float(peak[ok].sum()), "peak_min": float(peak[ok].min()) if ok.any() else None,
            "peak_max": float(peak[ok].max()) if ok.any() else None, "flags": cb.flag_counts(flags, FLAG_NAMES)}


def total_stats(parts):
    lows, highs = [p["peak_min"] for p in parts if p["peak_min"] is not None], [p["peak_max"] for p in parts if p["peak_max"] is not None]
    return {"rank": "total", "crystals": sum(p["crystals"] for p in parts), "patterns": sum(p["patterns"] for p in parts),
            "n_reflections": sum(p["n_reflections"] for p in parts), "peak_sum": sum(p["peak_sum"] for p in parts),
            "peak_min": min(lows) if lows else None, "peak_max": max(highs) if highs else None,
            "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'xrd rank 0: 16 crystals, 15 patterns; mean n_reflections 412.3; two_theta_peak mean 31.42, min 12.05, max 44.60; flags RANGE 1'."""
    k = st["patterns"]
    body = (f"mean n_reflections {st['n_reflections'] / k:.1f}; two_theta_peak mean {st['peak_sum'] / k:.2f}, min {st['peak_min']:.2f}, "
            f"max {st['peak_max']:.2f}") if k else "mean n_reflections n/a; two_theta_peak n/a"
    return f"xrd {cb.who(st)}: {st['crystals']} crystals, {k} patterns; {body}; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


def against_lines(patterns, targets):
    """What `python -m arreau_amd.screen --xrd_against` prints of the crystals' patterns [B, n] and the targets' [T, n] under the
    same parameters: with T == B the paired mean and median distance, otherwise each crystal's smallest distance to any target."""
    patterns, targets = np.asarray(patterns, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    if len(patterns) == len(targets):
        d = np.array([distance(p, q) for p, q in zip(patterns, targets)])
        ok = ~np.isnan(d)
        if not ok.any():
            return [f"xrd against: {len(d)} pairs, none with two patterns"]
        return [f"xrd against: {int(ok.sum())} / {len(d)} pairs; paired distance mean {d[ok].mean():.6f}, median {np.median(d[ok]):.6f}"]
    m = distance_matrix(patterns, targets)
    lines = []
    for b, row in enumerate(m):
        ok = ~np.isnan(row)
        lines.append(f"xrd against: crystal {b}: " + (f"smallest distance {row[ok].min():.6f} (target {int(np.flatnonzero(ok)[np.argmin(row[ok])])})"
                                                     if ok.any() else "no pattern"))
    return lines


# ------------------------------------------------------------------------------------------------- the numpy restatement
def box_of(lattice_row, params=None):
    """(H_1, H_2, H_3) as floats of one cell [3,3] under `params` (rule 3): floor(d*_hi |a_k|)."""
    A = np.asarray(lattice_row, dtype=np.float64).reshape(3, 3)
    return np.floor(derived(params if params is not None else XrdParams()).dhi * np.sqrt((A * A).sum(axis=1)))


def xrd_reference(frac, lattice, counts, weights, params=None, dtype=np.float64, exact_inputs=False):
    """Rules 1-8 in numpy from the float32 inputs: frac [N,3], lattice [B,3,3], counts [B] atoms per crystal, weights [N].
    dtype float64 is the yardstick (the structure factor, the Gaussians and every sum in float64, the coordinates unwrapped:
    exp(2 pi i h x) does not see the wrap); float32 is the kernel's split -- rules 2-4 and 6 float64, rule 5 one float32 operation
    at a time in atom order with the sine and cosine of 2 pi r rounded to float32, rule 7 float32 in ascending box index --, the
    arithmetic whose deviation from float64 is measured for the bound.  Returns a namespace: pattern [B, n_points] (of `dtype`),
    n_reflections, volume, weight_sum, flags [B]; `margin` [B], the relative distance |d* / cut - 1| of the crystal's nearest box
    point to either d* cut (inf where none; NaN for a flagged crystal); `box` [B,3]; `rounds` [B], the rounds of 256 box
    entries; `reflections`, per crystal (two_theta [K], intensity [K]) of the kept half-space reflections in box order, each
    intensity the Friedel pair's I of rule 6 (None for a flagged crystal).
    exact_inputs (float64 only) takes frac and lattice as the float64 numbers they are, not as the float32 the kernel would see:
    two descriptions of one crystal then describe it to 2^-53, not to 2^-24."""
    if exact_inputs:
        assert np.dtype(dtype) == np.float64
        frac, lattice = np.asarray(frac, dtype=np.float64).reshape(-1, 3), np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3)
        counts = [int(n) for n in counts]
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    else:
        frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    weights = np.ascontiguousarray(weights, dtype=F32).reshape(-1)
    assert weights.shape[0] == frac.shape[0]
    p = params if params is not None else XrdParams()
    d = derived(p)
    f32 = np.dtype(dtype) == np.float32
    dt = F32 if f32 else np.float64
    B, g = len(counts), grid(p)
    out = SimpleNamespace(pattern=np.full((B, p.n_points), np.nan, dt), n_reflections=np.zeros(B, np.int32), volume=np.full(B, np.nan, F32),
                          weight_sum=np.full(B, np.nan, F32), flags=np.zeros(B, np.int32), margin=np.full(B, np.nan), box=np.zeros((B, 3), np.int64),
                          rounds=np.zeros(B, np.int64), reflections=[None] * B)
    deg = 180.0 / math.pi
    for b, n in enumerate(counts):
        L, f, w = lattice[b], frac[first[b]:first[b + 1]], weights[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all() and np.isfinite(w).all()):
            out.flags[b] = NONFINITE
            continue
        A = L.astype(np.float64)
        R = np.array([np.cross(A[1], A[2]), np.cross(A[2], A[0]), np.cross(A[0], A[1])])
        det = float(np.dot(A[0], R[0]))
        V = abs(det)
        with np.errstate(all="ignore"):
            vol32 = cb.cell_f32(L.astype(F32), 1.0, 0.0, 8)[0]
        if not (vol32 > 0 and np.isfinite(vol32) and V > 0 and np.isfinite(V)):
            out.flags[b] = CELL
            continue
        if n == 0:
            out.flags[b] = EMPTY
            continue
        H = np.floor(d.dhi * np.sqrt((A * A).sum(axis=1)))
        if not (H <= p.max_index).all():
            out.flags[b] = RANGE
            continue
        H = H.astype(np.int64)
        R = R / det
        h, k, l = [a.reshape(-1) for a in np.meshgrid(np.arange(0, H[0] + 1), np.arange(-H[1], H[1] + 1), np.arange(-H[2], H[2] + 1), indexing="ij")]
        half = (h > 0) | (k > 0) | ((k == 0) & (l > 0))
        G = (h[:, None] * R[0][None] + k[:, None] * R[1][None]) + l[:, None] * R[2][None]
        d2 = (G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2]
        keep = half & (d2 >= d.dlo * d.dlo) & (d2 <= d.dhi * d.dhi)
        ds = np.sqrt(d2[half])
        with np.errstate(all="ignore"):
            margin = np.abs(ds / d.dhi - 1.0).min(initial=np.inf)
            if d.dlo > 0:
                margin = min(margin, np.abs(ds / d.dlo - 1.0).min(initial=np.inf))
        out.margin[b], out.box[b], out.rounds[b] = margin, H, -(-h.size // ROUND)
        hk, d2k = np.stack([h[keep], k[keep], l[keep]], axis=1), d2[keep]
        if f32:
            x = (f - np.floor(f)).astype(F32)
            x[x >= F32(1)] = F32(0)
            hf = hk.astype(F32)
            t = ((hf[:, 0:1] * x[None, :, 0] + hf[:, 1:2] * x[None, :, 1]).astype(F32) + hf[:, 2:3] * x[None, :, 2]).astype(F32)
            r = (t - np.rint(t)).astype(F32)
            ang = 2.0 * math.pi * r.astype(np.float64)  # (sincospi(2 r): no rounding of the argument)
            c, s = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
            zero = np.zeros((hk.shape[0], 1), F32)  # (an empty list of reflections keeps its shape)
            re = np.concatenate([zero, np.cumsum((w[None, :] * c).astype(F32), axis=1, dtype=F32)], axis=1)[:, -1].astype(np.float64)
            im = np.concatenate([zero, np.cumsum((w[None, :] * s).astype(F32), axis=1, dtype=F32)], axis=1)[:, -1].astype(np.float64)
        else:
            x = f.astype(np.float64)
            x = x - np.floor(x)
            ang = 2.0 * math.pi * (hk.astype(np.float64) @ x.T)
            wd = w.astype(np.float64)
            re, im = np.cos(ang) @ wd, np.sin(ang) @ wd
        sth = 0.5 * p.wavelength * np.sqrt(d2k)
        s2 = sth * sth
        c2t = 1.0 - 2.0 * s2
        lp = (1.0 + c2t * c2t) / (s2 * np.sqrt(1.0 - s2))
        dw = np.exp(-0.5 * p.b_iso * d2k) if p.b_iso != 0.0 else np.ones_like(d2k)
        tt = 2.0 * deg * np.arcsin(sth)
        inten = 2.0 * (re * re + im * im) * dw * lp * (1.0 / (V * V))
        amp = (inten * d.norm).astype(dt)
        P = np.zeros(p.n_points, dt)
        for e in range(tt.size):
            lo = int(min(max(math.floor((tt[e] - d.six_sigma - p.two_theta_min) / d.step), 0), p.n_points - 1))
            hi = int(min(max(math.ceil((tt[e] + d.six_sigma - p.two_theta_min) / d.step), 0), p.n_points - 1))
            dd = g[lo:hi + 1] - tt[e]
            m = np.abs(dd) <= d.six_sigma
            z = (dd[m] / d.sigma).astype(dt)
            with np.errstate(under="ignore"):
                P[lo:hi + 1][m] = (P[lo:hi + 1][m] + (amp[e] * np.exp((dt(-0.5) * (z * z).astype(dt)).astype(dt)).astype(dt)).astype(dt)).astype(dt)
        out.pattern[b], out.n_reflections[b], out.volume[b], out.reflections[b] = P, 2 * tt.size, vol32, (tt, inten)
        # rule 8: thread t adds atoms t, t + 256, ...; the butterfly within a wave; the four waves in order
        part = np.zeros(ROUND, F32)
        for a0 in range(0, n, ROUND):
            chunk = w[a0:a0 + ROUND]
            part[:chunk.size] = (part[:chunk.size] + chunk).astype(F32)
        waves = part.reshape(4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            waves = (waves + waves[:, np.arange(64) ^ off]).astype(F32)
        total = F32(0)
        for v in waves[:, 0]:
            total = F32(total + v)
        out.weight_sum[b] = total
    return out
