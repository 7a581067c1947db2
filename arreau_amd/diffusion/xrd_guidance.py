"""XRD guidance: steering the sampler towards a target powder pattern (arreau_sample_loop_xrd_guided, arreau_xrd_guidance_step,
arreau_amd/csrc/xrd_guide.hip; the rules are written out in include/arreau_hip.h, section "XRD guidance").  Here: the option and
its validation, the flag constants, the class amplitudes, a numpy restatement of rules 1-6 (`reference`: float64 the yardstick of
the tests; float32 the kernel's split of precisions and operation kinds), the guided prediction (`guided_eps`), the measured
float32 bound and the statistics.  Needs numpy alone at import.

The rule in one paragraph.  P is the crystal's powder pattern (xrd.py, the atoms' amplitudes those of their current species
class: Z, or 1, and 0 for the mask class, so a masked atom neither scatters nor is pushed), Q the target on the same grid,
dist = (1 - cos(P, Q)) / 2.  Its derivative with respect to atom a's Cartesian position is D_a = -4 pi w_a sum_hkl kappa c (Re F
sin phi_a - Im F cos phi_a) G_hkl over the kept half-space reflections, with c = sum_p u(p) G(p) over the reflection's window, u =
d dist / d P and kappa = 2 DW LP / V^2 / (sigma sqrt(2 pi)).  g_a = D_a L^-1 and eps'_a = eps_a + (w / sigma_t^2) g_a: the
predictor's clean-position estimate x - sigma_t^2 eps moves -w g, one descent step of size w (A^2) on the distance.

What this is not: positions only -- the peak positions depend on the cell alone, so a wrong cell cannot be repaired (fix the
cell: fixed_cell, a condition or a lattice system); no guidance of species; no intensity scale or background fit (the cosine
distance is scale free); no weight schedule other than 1 / sigma_t^2; with the synthetic checkpoints of this tree no claim on
sample quality.  A crystal of more than 256 atoms is flagged LARGE and not guided.

The float32 bound on g is MEASURED, not derived (F32_DEVIATION): the largest |g_32 - g_64| over the crystal's largest |g_64|
component, of `reference`'s float32 mode against its float64 mode over every batch of tests/xrd_guidance_cases.py
(tools/exp/xrd_guidance_f32_deviation.py); the tests allow the device G_F32_BOUND = 16 times the largest of them, the factor
xrd.BOUND_FACTOR gives the pattern, for its sincospif and expf and its fused float64 operations.  It is never taken from the
device.  It holds for crystals at a float64 distance of at least MIN_TEST_DISTANCE from their target: nearer to it u is a
difference of nearly equal numbers and no float32 bound relative to |g| is meaningful."""
import math
from numbers import Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from . import xrd
from .xrd import CELL, EMPTY, NONFINITE, RANGE, BOUND_FACTOR, XrdParams

NO_TARGET, DARK, LARGE = 16, 32, 64
FLAG_NAMES = xrd.FLAG_NAMES + ((NO_TARGET, "NO_TARGET"), (DARK, "DARK"), (LARGE, "LARGE"))
SKIPPED = NONFINITE | CELL | EMPTY | RANGE | NO_TARGET | DARK | LARGE  # a crystal with any flag keeps its eps bit for bit
MAX_ATOMS = cb.STAGED_ATOMS
INFO_KEYS = ("distance", "reflections", "flags")  # SampleResult.info["xrd_guidance"]: the last evaluation's, one entry per crystal
DEFAULT_WEIGHT = 2.0  # A^2; a starting value, not a claim
MIN_TEST_DISTANCE = 1e-3
F32 = np.float32
U32 = 2.0 ** -24
# measured by tools/exp/xrd_guidance_f32_deviation.py over each batch of tests/xrd_guidance_cases.py (BATCHES, in its order)
F32_DEVIATION = {"textbook": 5.94e-07, "triclinic": 3.68e-07, "ragged": 2.19e-06, "random 20": 1e-06, "atoms 256": 3.65e-06,
                 "narrow": 8.45e-07, "wide": 6.94e-07, "b_iso": 7.06e-07, "unit": 4.18e-07}
G_F32_BOUND = BOUND_FACTOR * max(F32_DEVIATION.values())  # 5.8e-5 of the crystal's largest |g| component


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


def check_patterns(target, n_points, B=None):
    """The target patterns as float32 [T, n_points], T == 1 for a single row; ValueError unless finite, non-negative, no row all
    zero, on a grid of n_points, and (B given) T in (1, B)."""
    a = np.asarray(target)
    if a.dtype == object or a.dtype.kind not in "fiu" or a.ndim not in (1, 2) or a.shape[-1] != n_points or a.size == 0:
        raise ValueError(f"xrd_guidance: target patterns must be [n_points] or [B, n_points] numbers with n_points = {n_points}, got shape {a.shape}")
    with np.errstate(over="ignore"):
        a = np.ascontiguousarray(a.reshape(-1, n_points), dtype=F32)
    if not np.isfinite(a).all():
        raise ValueError("xrd_guidance: the target patterns must be finite (in float32)")
    if (a < 0).any():
        raise ValueError("xrd_guidance: the target patterns must be non-negative")
    if not (a > 0).any(axis=1).all():
        raise ValueError("xrd_guidance: a target pattern is all zero")
    if B is not None and a.shape[0] not in (1, B):
        raise ValueError(f"xrd_guidance: {a.shape[0]} target patterns for {B} crystals (one for all, or one each)")
    return a


def _is_crystals(target):
    return all(hasattr(target, k) for k in ("frac_x", "lattice", "num_atoms", "atomic_numbers"))


class XrdGuidance:
    """target: the patterns to approach -- [n_points] (one for every crystal) or [B, n_points] on the grid of `params`, or
    crystals (a SampleResult or a loaded crystals file, one for every crystal or one each), whose patterns are computed by
    xrd.xrd under the same params before the loop; weight w in A^2: the descent step on the predicted clean structure (finite,
    >= 0; 2.0 is a starting value; 0 is the sampler without guidance, bit for bit); params: the xrd.XrdParams of the grid, the
    peak width and the scattering ("Z" or "unit" inside sample())."""

    def __init__(self, target, weight=DEFAULT_WEIGHT, params=None):
        params = XrdParams() if params is None else params
        if not isinstance(params, XrdParams):
            raise ValueError(f"xrd_guidance: params must be an xrd.XrdParams, got {params!r}")
        if not isinstance(weight, Real) or isinstance(weight, bool):
            raise ValueError(f"xrd_guidance: weight must be a number, got {weight!r}")
        with np.errstate(over="ignore"):
            if not (math.isfinite(weight) and np.isfinite(F32(weight)) and weight >= 0.0):
                raise ValueError(f"xrd_guidance: weight must be finite (in float32) and >= 0, got {weight}")
        self.weight, self.params = float(weight), params
        if target is None:
            raise ValueError("xrd_guidance: a target (patterns or crystals) is required")
        self.crystals = target if _is_crystals(target) else None
        self.target = None if self.crystals is not None else check_patterns(target, params.n_points)
        if self.crystals is not None and len(np.asarray(self.crystals.num_atoms).reshape(-1)) < 1:
            raise ValueError("xrd_guidance: the target crystals hold no crystal")

    def __repr__(self):
        what = f"{len(np.asarray(self.crystals.num_atoms).reshape(-1))} crystals" if self.crystals is not None else f"patterns {self.target.shape}"
        return f"XrdGuidance(target={what}, weight={self.weight}, params={self.params})"

    def count(self):
        """The number of targets: 1 (one for every crystal) or one per crystal."""
        return len(np.asarray(self.crystals.num_atoms).reshape(-1)) if self.crystals is not None else self.target.shape[0]

    def patterns(self, B, device="cuda"):
        """The target rows float32 [B, n_points]: the given patterns, or the crystals' patterns under `params` (one xrd launch)."""
        rows = self.target
        if self.crystals is not None:
            rows = check_patterns(xrd.xrd_sample_result(self.crystals, self.params, device)["pattern"], self.params.n_points)
        rows = check_patterns(rows, self.params.n_points, B)
        return np.ascontiguousarray(np.broadcast_to(rows, (B, self.params.n_points)) if rows.shape[0] == 1 else rows)


def resolve(xrd_guidance):
    """sample(xrd_guidance=...): None / False -> None, an XrdGuidance -> itself."""
    if xrd_guidance is None or xrd_guidance is False:
        return None
    if isinstance(xrd_guidance, XrdGuidance):
        return xrd_guidance
    raise ValueError(f"xrd_guidance must be None or an XrdGuidance, got {xrd_guidance!r}")


def check_sampling(guidance, *, inversion=False, B=None):
    """What XRD guidance is not combined with, before any work: an inversion (encode, arreau_invert_loop) has no prediction to
    guide; scattering "weights" has no array inside sample() (the amplitudes are those of the species classes); the number of
    targets is 1 or the batch's.  Every noise mode is served: noise='philox' by the guided loop, 'device' and 'reference' by the
    guidance step between the network evaluation and the step."""
    if guidance is None:
        return
    if inversion:
        raise ValueError("xrd_guidance is not supported with an inversion (encode): there is no clean-structure prediction to guide")
    if guidance.params.scattering == "weights":
        raise ValueError('xrd_guidance: scattering "weights" is for the step export (atom weights); inside sample() use "Z" or "unit"')
    if B is not None and guidance.count() not in (1, int(B)):
        raise ValueError(f"xrd_guidance: {guidance.count()} targets for {B} crystals (one for all, or one each)")


def class_weights(z_table, params=None):
    """The amplitude of every species class, float32 [S]: under scattering "Z" its atomic number, under "unit" 1; the last class,
    the mask, weighs 0 -- an atom that is still masked does not scatter and gets no push."""
    p = params if params is not None else XrdParams()
    if p.scattering == "weights":
        raise ValueError('xrd_guidance: scattering "weights" has no class amplitudes; use "Z" or "unit"')
    zs = np.asarray(list(z_table.zs), dtype=np.float64).reshape(-1)
    w = (np.ones_like(zs) if p.scattering == "unit" else zs).astype(F32)
    w[-1] = 0.0
    return w


def atom_weights(types, weights_of_class):
    """w_a = weights_of_class[types[a]], 0 for a class outside the table: the kernel's rule."""
    t, w = np.asarray(types, dtype=np.int64).reshape(-1), np.asarray(weights_of_class, dtype=F32).reshape(-1)
    ok = (t >= 0) & (t < w.size)
    return np.where(ok, w[np.clip(t, 0, w.size - 1)], F32(0)).astype(F32)


# ------------------------------------------------------------------------------------------------------- the restatement
def _reflections(L, f, w, p, d, f32):
    """The kept half-space reflections of one unflagged crystal in box order (rules 4-6 of the xrd section, as xrd_reference forms
    them): hkl [K,3], G [K,3], two_theta, kappa [K], Re F, Im F [K] and the sine and cosine of every atom's phase [K,n] -- in the
    float32 mode the reduced float32 phase, its sine and cosine rounded to float32 and the atom sums float32 in atom order."""
    A = L.astype(np.float64)
    R = np.array([np.cross(A[1], A[2]), np.cross(A[2], A[0]), np.cross(A[0], A[1])])
    det = float(np.dot(A[0], R[0]))
    V = abs(det)
    H = np.floor(d.dhi * np.sqrt((A * A).sum(axis=1))).astype(np.int64)
    R = R / det
    h, k, l = [a.reshape(-1) for a in np.meshgrid(np.arange(0, H[0] + 1), np.arange(-H[1], H[1] + 1), np.arange(-H[2], H[2] + 1), indexing="ij")]
    half = (h > 0) | (k > 0) | ((k == 0) & (l > 0))
    G = (h[:, None] * R[0][None] + k[:, None] * R[1][None]) + l[:, None] * R[2][None]
    d2 = (G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2]
    keep = half & (d2 >= d.dlo * d.dlo) & (d2 <= d.dhi * d.dhi)
    hk, G, d2 = np.stack([h[keep], k[keep], l[keep]], axis=1), G[keep], d2[keep]
    if f32:
        x = (f - np.floor(f)).astype(F32)
        x[x >= F32(1)] = F32(0)
        hf = hk.astype(F32)
        t = ((hf[:, 0:1] * x[None, :, 0] + hf[:, 1:2] * x[None, :, 1]).astype(F32) + hf[:, 2:3] * x[None, :, 2]).astype(F32)
        ang = 2.0 * math.pi * (t - np.rint(t)).astype(F32).astype(np.float64)
        c, s = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
        zero = np.zeros((hk.shape[0], 1), F32)
        re = np.concatenate([zero, np.cumsum((w[None, :] * c).astype(F32), axis=1, dtype=F32)], axis=1)[:, -1].astype(np.float64)
        im = np.concatenate([zero, np.cumsum((w[None, :] * s).astype(F32), axis=1, dtype=F32)], axis=1)[:, -1].astype(np.float64)
        c, s = c.astype(np.float64), s.astype(np.float64)
    else:
        x = f.astype(np.float64)
        ang = 2.0 * math.pi * (hk.astype(np.float64) @ (x - np.floor(x)).T)
        c, s = np.cos(ang), np.sin(ang)
        re, im = c @ w.astype(np.float64), s @ w.astype(np.float64)
    sth = 0.5 * p.wavelength * np.sqrt(d2)
    s2 = sth * sth
    c2t = 1.0 - 2.0 * s2
    lp = (1.0 + c2t * c2t) / (s2 * np.sqrt(1.0 - s2))
    dw = np.exp(-0.5 * p.b_iso * d2) if p.b_iso != 0.0 else np.ones_like(d2)
    return SimpleNamespace(hkl=hk, G=G, R=R, two_theta=2.0 * (180.0 / math.pi) * np.arcsin(sth), kappa=(2.0 * dw * lp * (1.0 / (V * V))) * d.norm,
                           re=re, im=im, sin=s, cos=c)


def reference(frac, lattice, counts, weights, target, params=None, dtype=np.float64, exact_inputs=False):
    """Rules 1-6 in numpy from the float32 inputs: frac [N,3], lattice [B,3,3], counts [B], weights [N] (the atoms' amplitudes:
    atom_weights(types, class_weights(...))), target [B, n_points] (or one row for all).  dtype float64 is the yardstick; float32
    follows the kernel's operation kinds -- the pattern of xrd_reference's float32 mode, the three sums float64, u rounded to
    float32, the Gaussians float32, the reduced float32 phases with their sines and cosines rounded to float32, everything after
    them float64, g rounded to float32.  Returns a namespace: distance [B] (NaN for a flagged crystal), reflections [B], flags
    [B], D [N,3] (d distance / d r_a), g [N,3] = D L^-1 (zero for a flagged crystal), pattern [B, n_points], u [B, n_points];
    g_terms [N,3], the same sums with every term's magnitude in place of the term: what g cancels from (a single atom's g
    vanishes identically -- the pattern does not see a translation --, so its float32 error has only this scale).
    exact_inputs (float64 only) takes frac and lattice as the float64 numbers they are, as xrd_reference does."""
    p = params if params is not None else XrdParams()
    f32 = np.dtype(dtype) == np.float32
    xr = xrd.xrd_reference(frac, lattice, counts, weights, p, dtype=dtype, exact_inputs=exact_inputs)
    if exact_inputs:
        frac, lattice = np.asarray(frac, dtype=np.float64).reshape(-1, 3), np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3)
        counts = [int(n) for n in counts]
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    else:
        frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    weights = np.ascontiguousarray(weights, dtype=F32).reshape(-1)
    B, N = len(counts), frac.shape[0]
    target = np.asarray(target, dtype=F32).reshape(-1, p.n_points)
    target = np.broadcast_to(target, (B, p.n_points)) if target.shape[0] == 1 else target
    assert target.shape[0] == B
    d, grid = xrd.derived(p), xrd.grid(p)
    out = SimpleNamespace(distance=np.full(B, np.nan), reflections=np.zeros(B, np.int64), flags=np.zeros(B, np.int64), D=np.zeros((N, 3)),
                          g=np.zeros((N, 3), F32 if f32 else np.float64), pattern=xr.pattern, u=np.zeros((B, p.n_points)), g_terms=np.zeros((N, 3)))
    for b, n in enumerate(counts):
        Q = target[b].astype(np.float64)
        if xr.flags[b]:
            out.flags[b] = xr.flags[b]
        elif n > MAX_ATOMS:
            out.flags[b] = LARGE
        elif not np.isfinite(Q).all() or (Q < 0).any() or not (Q > 0).any():
            out.flags[b] = NO_TARGET
        if out.flags[b]:
            continue
        P = xr.pattern[b].astype(np.float64)
        pq, pp, qq = float(P @ Q), float(P @ P), float(Q @ Q)
        if not (pp > 0.0 and math.isfinite(pp)):
            out.flags[b] = DARK
            continue
        inv = 1.0 / (math.sqrt(pp) * math.sqrt(qq))
        u = -0.5 * inv * (Q - (pq / pp) * P)
        if f32:
            u = u.astype(F32).astype(np.float64)
        L, f, w = lattice[b], frac[first[b]:first[b + 1]], weights[first[b]:first[b + 1]]
        r = _reflections(L, f, w, p, d, f32)
        assert 2 * r.two_theta.size == xr.n_reflections[b]
        c = np.zeros(r.two_theta.size)
        for e, tt in enumerate(r.two_theta):
            lo = int(min(max(math.floor((tt - d.six_sigma - p.two_theta_min) / d.step), 0), p.n_points - 1))
            hi = int(min(max(math.ceil((tt + d.six_sigma - p.two_theta_min) / d.step), 0), p.n_points - 1))
            dd = grid[lo:hi + 1] - tt
            m = np.abs(dd) <= d.six_sigma
            z = dd[m] / d.sigma
            with np.errstate(under="ignore"):
                if f32:
                    z = z.astype(F32)
                    G = np.exp((F32(-0.5) * (z * z).astype(F32)).astype(F32)).astype(F32).astype(np.float64)
                else:
                    G = np.exp(-0.5 * z * z)
            c[e] = float(np.dot(u[lo:hi + 1][m], G))
        turn = r.re[:, None] * r.sin - r.im[:, None] * r.cos  # [K, n]
        D = -4.0 * math.pi * w.astype(np.float64)[:, None] * (turn.T @ ((r.kappa * c)[:, None] * r.G))
        g = D @ r.R.T
        size = np.abs(r.re)[:, None] * np.abs(r.sin) + np.abs(r.im)[:, None] * np.abs(r.cos)
        out.g_terms[first[b]:first[b + 1]] = (4.0 * math.pi * np.abs(w.astype(np.float64))[:, None]
                                              * (size.T @ (np.abs(r.kappa * c)[:, None] * np.abs(r.G)))) @ np.abs(r.R.T)
        out.D[first[b]:first[b + 1]] = D
        out.g[first[b]:first[b + 1]] = g.astype(F32) if f32 else g
        out.u[b], out.distance[b], out.reflections[b] = u, 0.5 * (1.0 - pq * inv), 2 * r.two_theta.size
    return out


def gamma(g, L):
    """g times the metric L L^T: d distance / d (fractional coordinates), what central differences of the distance measure."""
    L = np.asarray(L, dtype=np.float64).reshape(3, 3)
    return np.asarray(g, dtype=np.float64) @ (L @ L.T)


def sigma_coefficient(ve_sigmas, t, weight):
    """w / sigma_t^2 per crystal in float64, t clamped into 1..T as the kernel clamps it; ve_sigmas [T+1]."""
    sig = np.asarray(ve_sigmas, dtype=np.float64).reshape(-1)
    t = np.clip(np.asarray(t, dtype=np.int64).reshape(-1), 1, sig.size - 1)
    return float(F32(weight)) / sig[t] ** 2


def guided_eps(eps, ref, counts, ve_sigmas, t, weight):
    """eps' = eps + (w / sigma_t^2) g in float64: eps [N,3], ref the namespace of `reference`, t [B] the crystals' timesteps.  A
    flagged crystal keeps its eps (its g is zero)."""
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, 3)
    k = np.repeat(sigma_coefficient(ve_sigmas, t, weight), [int(n) for n in counts])
    return eps + k[:, None] * np.asarray(ref.g, dtype=np.float64)


def g_scale(g, g_terms):
    """What the float32 deviation of a crystal's g is measured against: its largest |g_f64| component; for a single atom, whose g
    is zero identically, the largest component of g_terms."""
    g = np.asarray(g, dtype=np.float64).reshape(-1, 3)
    return float(np.abs(g_terms if g.shape[0] == 1 else g).max(initial=0.0))


def g_bound(g, g_terms):
    """The largest |g_f32 - g_f64| of a component allowed in a crystal whose float64 gradient is g [n,3]: G_F32_BOUND of g_scale
    (module docstring)."""
    return G_F32_BOUND * g_scale(g, g_terms)


def eps_bound(k, gb, g, eps_guided):
    """The largest |eps'_f32 - eps'_exact| per component: k = w / sigma_t^2 (float64), gb the crystal's g_bound; k in float32 and
    the product cost 4 u of |g|, the sum 2 u of |eps'| (contact guidance's expression)."""
    return k * (gb + 4 * U32 * np.abs(g)) + 2 * U32 * np.abs(eps_guided)


# ------------------------------------------------------------------------------------------------------- the device side
class DeviceGuidance:
    """What the engine's entry points take (sample_loop(xrd_guidance=...), xrd_guidance_step): params an xrd.XrdParams, the weight,
    target a float32 [B, n_points] device tensor, the amplitudes as class_weights float32 [S] or -- the step export alone --
    atom_weights float32 [N] (exactly one), and info, the dict of allocate_info or None."""

    def __init__(self, params, weight, target, class_weights=None, atom_weights=None, info=None):
        self.params, self.weight, self.target = params, float(weight), target
        self.class_weights, self.atom_weights, self.info = class_weights, atom_weights, info


def device_guidance(guidance, z_table, B, device):
    """The DeviceGuidance of a sample() call: the target rows uploaded (crystals: their patterns by one xrd launch first), the
    class amplitudes of the model's table, fresh diagnostic arrays."""
    import torch
    target = torch.as_tensor(guidance.patterns(B, device), device=device).contiguous()
    weights = torch.as_tensor(class_weights(z_table, guidance.params), device=device).contiguous()
    return DeviceGuidance(guidance.params, guidance.weight, target, class_weights=weights, info=allocate_info(B, device))


def allocate_info(B, device):
    """The three diagnostic arrays of a guided run on the device: distance float32 [B], reflections and flags int32 [B], zeroed."""
    import torch
    return {"distance": torch.zeros(B, device=device, dtype=torch.float32), "reflections": torch.zeros(B, device=device, dtype=torch.int32),
            "flags": torch.zeros(B, device=device, dtype=torch.int32)}


def info_to_numpy(info):
    """SampleResult.info["xrd_guidance"] of the device arrays: the last evaluation's distance, reflections and flags per crystal."""
    return {k: info[k].cpu().numpy() for k in INFO_KEYS}


def stats_of(info, rank=0):
    """The last-evaluation statistics of one rank's info dict: crystals, the guided ones, the sum, minimum and maximum of their
    distance, the count per flag."""
    dist = np.asarray(info["distance"], dtype=np.float64).reshape(-1)
    flags = np.asarray(info["flags"], dtype=np.int64).reshape(-1)
    ok = (flags == 0) & ~np.isnan(dist)
    return {"rank": cb.rank_of(rank), "crystals": int(flags.size), "guided": int(ok.sum()), "distance_sum": float(dist[ok].sum()),
            "distance_min": float(dist[ok].min()) if ok.any() else None, "distance_max": float(dist[ok].max()) if ok.any() else None,
            "flags": cb.flag_counts(flags, FLAG_NAMES)}


def total_stats(parts, rank="total"):
    """The sum of stats_of dicts: over the ranks (rank "total"), or over one rank's batches (its number)."""
    lows = [p["distance_min"] for p in parts if p["distance_min"] is not None]
    highs = [p["distance_max"] for p in parts if p["distance_max"] is not None]
    return {"rank": cb.rank_of(rank), "crystals": sum(p["crystals"] for p in parts), "guided": sum(p["guided"] for p in parts),
            "distance_sum": sum(p["distance_sum"] for p in parts), "distance_min": min(lows) if lows else None,
            "distance_max": max(highs) if highs else None, "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    k = st["guided"]
    body = (f"distance to the target mean {st['distance_sum'] / k:.6f}, min {st['distance_min']:.6f}, max {st['distance_max']:.6f}" if k
            else "distance to the target n/a")
    return f"xrd guidance, {cb.who(st)}: {st['crystals']} crystals, last evaluation: {k} guided, {body}, flags: {cb.some(st['flags'])}"


def summary_lines(parts):
    return cb.summary_lines(parts, format_stats, total_stats)
