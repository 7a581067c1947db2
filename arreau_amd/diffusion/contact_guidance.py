"""Contact guidance: steering the sampler away from short contacts (arreau_sample_loop_guided, arreau_contact_guidance_step,
arreau_amd/csrc/contact_guide.hip; the rules are written out in include/arreau_hip.h, section "contact guidance").  Here: the
parameters and their validation, the flag constants, a float64 restatement of the rule for the tests (`reference`), the guided
prediction (`guided_eps`) and the derived float32 bounds (`g_bound`, `energy_bound`).  Needs numpy alone at import.

The rule.  For a crystal with cell rows a, b, c (the cell the step's network evaluation saw), wrapped positions r and d0 =
min_distance:
  * contacts: every (i, j, n), j != i, n an integer image in the screen's range for the radius d0, with 0 < d < d0,
    d = |r_j + n L - r_i|; self images are left out, a pair at d == 0 is skipped and sets OVERLAP;
  * penalty U = 1/2 sum_i sum_(j,n) 1/2 (d0 - d)^2 (A^2);
  * Cartesian gradient on atom i: D_i = sum_(j,n) ((d0 - d) / d) (r_j + n L - r_i), pointing towards the neighbours;
  * fractional gradient g_i = D_i L^-1, g_ik = (D_i . c_k) / V, c_0 = b x c, c_1 = c x a, c_2 = a x b, V = a . (b x c): the
    fractional move -w g_i is the Cartesian move -w D_i in any cell;
  * guided prediction eps'_i = eps_i + (w / sigma_t^2) g_i: the predictor's clean-position estimate x - sigma_t^2 eps moves one
    descent step of size w down U.  An isolated contact moves each atom w (d0 - d) away from the other: w = 0.5 resolves it.
    Read as a score (eps = -sigma^2 score) this is guidance by p_t(y | x) ~ exp(-w U / sigma_t^2).  The corrector reads
    -eps' / sigma_t^2 as its score and normalises its step by |eps'|.
What this is not: no cell-strain term (lengths and angles are not guided), no radii or species dependence, no weight schedule
other than 1 / sigma_t^2, no claim on sample quality.

The float32 bound on g (`g_bound`), u = 2^-24.  Let G = max_d sum_k (1 + N_k) |L_kd| (screening.py's G: the largest magnitude a
coordinate of r_j + n L reaches), C the largest number of contacts one atom of the crystal has, d_min the crystal's smallest
contact distance.
  1. disp = (r_j + s) - r_i.  r_j, s and r_i are three products and two sums each (at most 2.5 u of their term sums), the two
     combining operations add u (1 + N) sum |L| and u G: every component is off by at most 10 u G, the vector by
     e = sqrt(3) 10 u G.  This is the cancellation term: it does not shrink with d.
  2. d = sqrt(d2): |dd| <= e + 3 u d0 (the dot product's three roundings and the root's half ulp, d < d0).
  3. one contact's term f disp, f = (d0 - d) / d, |f disp| = d0 - d <= d0:
     |d term| <= |df| d + f e + u d0, with |df| <= (|dd| + u d0) / d + (d0 - d) |dd| / d^2 + u f.  Since 1 <= d0 / d this is at most
     tau = 3 (d0 / d_min) (e + 3 u d0).
  4. D_i adds at most C such terms in at most C + 6 additions (the lane's partial sum, six butterfly steps):
     |dD| <= C tau + (C + 6) C u d0, and |D| <= C d0.
  5. g_k = (D . c_k) / V.  With P the largest product of two row norms, |dc_k| <= 6 sqrt(3) u P <= 11 u P and
     |dV| / |V| <= rho = 14 u |a| |b| |c| / |V|.  With h = max_k |c_k| / |V| (one over the smallest plane spacing):
     |dg| <= h |dD| + C d0 (11 u P / |V| + h (4 u + 2 rho)).
`energy_bound`, C now the crystal's ordered contacts: one term (d0 - d)^2 is off by at most 2 d0 (e + 4 u d0) + u d0^2; C of them in
at most C + 10 additions of terms
<= d0^2; times 1/4; plus u U for the last product.
`eps_bound`: eps' = eps + k g with k = w / sigma^2 in float32 (3 u relative): k (g_bound + 4 u |g|) + 2 u |eps'|."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from . import screening

NONFINITE, CELL, EMPTY, OVERLAP = 1, 2, 4, 8
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (OVERLAP, "OVERLAP"))
SKIPPED = NONFINITE | CELL | EMPTY  # a crystal with one of these keeps its eps bit for bit
MAX_SHELLS = screening.MAX_SHELLS
INFO_KEYS = ("energy", "contacts", "flags")  # SampleResult.info["contact_guidance"]: the last evaluation's, one entry per crystal
F32 = np.float32
U32 = 2.0 ** -24


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


@dataclass(frozen=True)
class ContactGuidance:
    """min_distance d0 in A: contacts shorter than it are pushed apart (finite, > 0; the screen's default threshold); weight w:
    the descent step on the predicted clean structure (finite, >= 0; 0.5 resolves an isolated contact exactly; 0 is the sampler
    without guidance, bit for bit); max_shells caps the periodic images per axis (1..8): a cell that needs more is flagged CELL
    and not guided."""
    min_distance: float = 0.5
    weight: float = 0.5
    max_shells: int = MAX_SHELLS

    def __post_init__(self):
        for name in ("min_distance", "weight"):
            v = getattr(self, name)
            if not isinstance(v, Real) or isinstance(v, bool):
                raise ValueError(f"{name} must be a number, got {v!r}")
            with np.errstate(over="ignore"):
                if not (math.isfinite(v) and np.isfinite(F32(v)) and v >= 0.0):
                    raise ValueError(f"{name} must be finite (in float32) and >= 0, got {v}")
            object.__setattr__(self, name, float(v))
        if not float(F32(self.min_distance)) > 0.0:
            raise ValueError(f"min_distance must be > 0, got {self.min_distance}")
        v = self.max_shells
        if not isinstance(v, Integral) or isinstance(v, bool) or not 1 <= int(v) <= MAX_SHELLS:
            raise ValueError(f"max_shells must lie in 1..{MAX_SHELLS}, got {v!r}")
        object.__setattr__(self, "max_shells", int(v))


def resolve(contact_guidance):
    """sample(contact_guidance=...): None / False -> None, True -> the defaults, a ContactGuidance -> itself."""
    return cb.resolve(contact_guidance, ContactGuidance, "contact_guidance")


def check_sampling(guidance, *, inversion=False):
    """What contact guidance is not combined with, before any work: an inversion (encode, arreau_invert_loop) has no prediction
    to guide.  Every noise mode is served: noise='philox' by the guided loop, 'device' and 'reference' by the guidance step
    between the network evaluation and the step."""
    if guidance is not None and inversion:
        raise ValueError("contact_guidance is not supported with an inversion (encode): there is no clean-structure prediction to guide")


# ------------------------------------------------------------------------------------------------------- the restatement
def _wrap(f):
    """crystal_wrap in the dtype given: w = f - floor(f), a result of 1 becomes 0."""
    w = f - np.floor(f)
    return np.where(w >= 1, 0, w).astype(f.dtype)


def reference(frac, lattice, offsets, params):
    """The rule in float64.  frac [N,3] (float32: wrapped in float32 as the kernel wraps it, then exact in float64; float64:
    wrapped in float64), lattice [B,3,3] rows a, b, c, offsets [B+1] (clamped into [0, N] as the kernel clamps them), params a
    ContactGuidance.  Returns a namespace: U [B], D [N,3], g [N,3] (zero for a skipped crystal), contacts [B] (unordered: the
    ordered contacts / 2), ordered [B], atom_contacts [N] (the contacts of every atom), flags [B]; per crystal the lists d (every ordered contact's distance) and margin
    (|d - d0| of every pair and image but the overlaps: how far each is from changing sides); d_min [B] (inf without contacts)."""
    frac = np.asarray(frac)
    frac = frac.reshape(-1, 3) if frac.dtype == F32 else np.asarray(frac, dtype=np.float64).reshape(-1, 3)
    lattice = np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    N, B = frac.shape[0], lattice.shape[0]
    d0 = float(F32(params.min_distance))
    md2 = float(F32(d0 * d0))  # the kernel compares squares against the float32 square, as the screen does
    out = SimpleNamespace(U=np.zeros(B), D=np.zeros((N, 3)), g=np.zeros((N, 3)), contacts=np.zeros(B, np.int64), ordered=np.zeros(B, np.int64),
                          flags=np.zeros(B, np.int64), atom_contacts=np.zeros(N, np.int64), d=[], margin=[], d_min=np.full(B, np.inf), shells=np.zeros((B, 3), np.int64))
    for b in range(B):
        first = int(min(max(offsets[b], 0), N))
        last = int(min(max(offsets[b + 1], first), N))
        n = last - first
        L, f = lattice[b], frac[first:last]
        out.d.append(np.zeros(0)); out.margin.append(np.zeros(0))
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
            out.flags[b] = NONFINITE
            continue
        with np.errstate(all="ignore"):
            vol, q = cb.cell_f64(L, d0)
        cell_bad = not np.isfinite(vol) or not bool((q <= params.max_shells).all())
        out.flags[b] = (CELL if cell_bad else 0) | (EMPTY if n == 0 else 0)
        if out.flags[b]:
            continue
        nk = np.maximum(1, np.ceil(q)).astype(np.int64)
        out.shells[b] = nk
        p = _wrap(f).astype(np.float64) @ L
        shifts, _ = cb.shift_table(nk)
        s = shifts.astype(np.float64) @ L
        disp = p[None, :, None, :] + s[None, None, :, :] - p[:, None, None, :]  # [i, j, m, 3]
        d2 = (disp ** 2).sum(-1)
        other = ~np.eye(n, dtype=bool)[:, :, None] & np.ones(s.shape[0], bool)[None, None, :]
        zero = other & (d2 == 0)
        if zero.any():
            out.flags[b] |= OVERLAP
        d = np.sqrt(d2)
        hit = other & (d2 > 0) & (d2 < md2)
        out.margin[b] = np.abs(d - d0)[other & ~zero]
        out.d[b] = d[hit]
        gap = np.where(hit, d0 - d, 0.0)
        with np.errstate(all="ignore"):
            fct = np.where(hit, gap / np.where(hit, d, 1.0), 0.0)
        D = (fct[..., None] * disp).sum((1, 2))
        out.D[first:last] = D
        c = np.array([np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])])
        out.g[first:last] = D @ c.T / float(np.dot(L[0], c[0]))
        out.U[b] = 0.25 * float((gap ** 2).sum())
        out.ordered[b] = int(hit.sum())
        out.atom_contacts[first:last] = hit.sum((1, 2))
        out.contacts[b] = out.ordered[b] // 2
        if out.ordered[b]:
            out.d_min[b] = float(out.d[b].min())
    return out


def sigma_coefficient(ve_sigmas, t, weight):
    """w / sigma_t^2 per crystal in float64, t clamped into 1..T as the kernel clamps it; ve_sigmas [T+1]."""
    sig = np.asarray(ve_sigmas, dtype=np.float64).reshape(-1)
    t = np.clip(np.asarray(t, dtype=np.int64).reshape(-1), 1, sig.size - 1)
    return float(F32(weight)) / sig[t] ** 2


def guided_eps(eps, ref, offsets, ve_sigmas, t, params):
    """eps' = eps + (w / sigma_t^2) g in float64: eps [N,3], ref the namespace of `reference`, t [B] the crystals' timesteps.  A
    skipped crystal keeps its eps."""
    eps = np.asarray(eps, dtype=np.float64).reshape(-1, 3)
    counts = np.diff(np.clip(np.asarray(offsets, dtype=np.int64), 0, eps.shape[0]))
    k = np.repeat(sigma_coefficient(ve_sigmas, t, params.weight), counts)
    return eps + k[:, None] * ref.g


# ------------------------------------------------------------------------------------------------------- the float32 bounds
def _cell_terms(L, shells):
    L = np.asarray(L, dtype=np.float64)
    G = float(((1 + np.asarray(shells, dtype=np.float64))[:, None] * np.abs(L)).sum(0).max())
    norms = np.linalg.norm(L, axis=1)
    c = np.array([np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])])
    vol = abs(float(np.dot(L[0], c[0])))
    P = float(max(norms[0] * norms[1], norms[1] * norms[2], norms[0] * norms[2]))
    return G, P, float(np.linalg.norm(c, axis=1).max()) / vol, 14 * U32 * float(norms.prod()) / vol, vol


def g_bound(d0, d_min, L, shells, atom_contacts):
    """The largest |g_f32 - g_exact| of a component of g in a crystal (module docstring, steps 1-5): d0, the crystal's smallest
    contact distance d_min, its cell L [3,3], the images per axis `shells` [3] and the largest contact count of one of its atoms.
    0 without contacts."""
    C = float(atom_contacts)
    if C == 0:
        return 0.0
    G, P, h, rho, vol = _cell_terms(L, shells)
    e = math.sqrt(3.0) * 10 * U32 * G
    tau = 3 * (d0 / d_min) * (e + 3 * U32 * d0)
    dD = C * tau + (C + 6) * C * U32 * d0
    return h * dD + C * d0 * (11 * U32 * P / vol + h * (4 * U32 + 2 * rho))


def energy_bound(d0, L, shells, ordered, U):
    """The largest |U_f32 - U_exact| of a crystal (module docstring)."""
    C = float(ordered)
    G = _cell_terms(L, shells)[0]
    e = math.sqrt(3.0) * 10 * U32 * G
    return 0.25 * (C * (2 * d0 * (e + 4 * U32 * d0) + U32 * d0 * d0) + (C + 10) * C * U32 * d0 * d0) + U32 * abs(U)


def eps_bound(k, gb, g, eps_guided):
    """The largest |eps'_f32 - eps'_exact| per component: k = w / sigma_t^2 (float64), gb the crystal's g_bound."""
    return k * (gb + 4 * U32 * np.abs(g)) + 2 * U32 * np.abs(eps_guided)


# ------------------------------------------------------------------------------------------------------- the device side
def allocate_info(B, device):
    """The three diagnostic arrays of a guided run on the device: energy float32 [B], contacts and flags int32 [B], zeroed."""
    import torch
    return {"energy": torch.zeros(B, device=device, dtype=torch.float32), "contacts": torch.zeros(B, device=device, dtype=torch.int32),
            "flags": torch.zeros(B, device=device, dtype=torch.int32)}


def info_to_numpy(info):
    """SampleResult.info["contact_guidance"] of the device arrays: the last evaluation's energy, contacts and flags per crystal."""
    return {k: info[k].cpu().numpy() for k in INFO_KEYS}


def stats_of(info, rank=0):
    """The last-step statistics of one rank's info dict(s): crystals, contacts, crystals with a contact, summed energy, flag counts."""
    contacts = np.asarray(info["contacts"], dtype=np.int64).reshape(-1)
    flags = np.asarray(info["flags"], dtype=np.int64).reshape(-1)
    return {"rank": cb.rank_of(rank), "crystals": int(contacts.size), "contacts": int(contacts.sum()), "with_contacts": int((contacts > 0).sum()),
            "energy": float(np.asarray(info["energy"], dtype=np.float64).sum()), "flags": cb.flag_counts(flags, FLAG_NAMES)}


def total_stats(parts, rank="total"):
    """The sum of stats_of dicts: over the ranks (rank "total"), or over one rank's batches (its number)."""
    out = {"rank": cb.rank_of(rank), "crystals": 0, "contacts": 0, "with_contacts": 0, "energy": 0.0, "flags": {name: 0 for _, name in FLAG_NAMES}}
    for p in parts:
        for k in ("crystals", "contacts", "with_contacts", "energy"):
            out[k] += p[k]
        for name, v in p["flags"].items():
            out["flags"][name] += v
    return out


def format_stats(st) -> str:
    return (f"contact guidance, {cb.who(st)}: {st['crystals']} crystals, last evaluation: {st['contacts']} contacts below min_distance in "
            f"{st['with_contacts']} crystals, penalty {st['energy']:.4g} A^2, flags: {cb.some(st['flags'])}")


def summary_lines(parts):
    return cb.summary_lines(parts, format_stats, total_stats)
