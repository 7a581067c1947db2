"""Ewald electrostatics of generated crystals: per crystal the electrostatic energy of the caller's point charges on its sites
under periodic boundary conditions -- its real-space, reciprocal-space, self and background parts, the net charge, the splitting
parameter used and the numbers of terms kept --, per atom the site potential (arreau_crystal_ewald, arreau_amd/csrc/ewald.hip; the
rules are written out in include/arreau_hip.h).  The first physical question asked of a generated ionic crystal: with these ions
on these sites, is the electrostatics reasonable, and which site is badly coordinated?  Table free: the user supplies the
charges per element.  Here: the parameters and their validation, the flag constants, `host_charges`, the entry point that needs
no engine (`ewald`), the host additions (`sample_arrays`: energy_per_atom, charge and species), the statistics, `madelung` and
`ewald_reference`, a numpy restatement of the rules -- in float64 the yardstick of the tests, which also reports each crystal's
margins to the two cuts; in float32 the kernel's split of precisions: the displacement and d2 of a pair bit for bit (hence n_pairs
exactly), the reduced phase and its sine and cosine in float32, everything else float64.  Needs numpy alone at import; the
restatement needs scipy.special.erfc.

Units: charges in e, lengths in A, K = 14.399645 eV A = V A / e; the potential is K times the sums (volts: 8.92 V on a site of
rock salt) and the energy (1 / 2) sum q potential in eV -- the textbook (K / 2) sum q phi with K inside the potential.

What this is not: no forces or stress, no guidance, no oxidation-state guessing or charge-balance check (a crystal that is not
neutral is computed with a neutralising background and flagged CHARGED), no dipole correction or other boundary terms beyond
tin-foil, no short-range repulsion -- so the energy alone favours collapse and is no stability ranking.

The float32 bound is MEASURED, not derived (F32_DEVIATION below): the largest deviation of the float32 mode from float64 over
every batch of tests/ewald_cases.py, energies relative to |E_self|, potentials relative to K 2 alpha max|q| / sqrt(pi); the tests
allow the device BOUND_FACTOR = 16 times the largest (voronoi.BOUND_FACTOR) for its erfc, exp, sincospif and fused operations.
It is never tuned from the kernel's output."""
import math
from dataclasses import dataclass
from numbers import Integral, Real
from types import SimpleNamespace

import numpy as np

from . import crystal_batch as cb
from .tools.atomic_number_table import SYMBOL_TO_Z, symbol_of
from .voronoi import BOUND_FACTOR

NONFINITE, CELL, EMPTY, RANGE, UNASSIGNED, OVERLAP, CHARGED = 1, 2, 4, 8, 16, 32, 64
FLAG_NAMES = ((NONFINITE, "NONFINITE"), (CELL, "CELL"), (EMPTY, "EMPTY"), (RANGE, "RANGE"), (UNASSIGNED, "UNASSIGNED"), (OVERLAP, "OVERLAP"),
              (CHARGED, "CHARGED"))
INVALID_MASK = 63  # a crystal with one of the first six has no numbers; CHARGED is informational
K = 14.399645  # eV A (include/arreau_hip.h: ARREAU_EWALD_K)
MAX_SHELLS, MAX_INDEX = 8, 127  # ARREAU_SCREEN_MAX_SHELLS, ARREAU_XRD_MAX_INDEX
ROUND = 256  # box entries per round: one per thread of the workgroup
CHARGED_TOLERANCE = 1e-6  # CHARGED: |sum q| > this times sum |q|
CRYSTAL_REALS = ("energy", "real", "reciprocal", "self", "background", "net_charge", "alpha", "volume")
RESULT_KEYS = CRYSTAL_REALS + ("n_pairs", "n_reciprocal", "flags", "potential")  # arreau_ewald_result without its scratch, in its order
ATOM_KEYS = ("potential", "charge", "species")  # one row per atom
STORED_KEYS = RESULT_KEYS + ("energy_per_atom", "charge", "species")  # what SampleResult.ewald and a crystals file hold
F32 = np.float32
# measured by tools/exp/ewald_f32_deviation.py: the largest deviation of ewald_reference's float32 mode from its float64 mode over
# each batch of tests/ewald_cases.py (BATCHES, in its order), the larger of the energies' (relative to |E_self|) and the
# potentials' (relative to K 2 alpha max|q| / sqrt(pi)); the tests allow BOUND_FACTOR times the largest
F32_DEVIATION = {"textbook": 1.02e-07, "ragged": 2.23e-05, "large": 0.000124, "rounds": 7.65e-07, "rounds 0.25": 1.77e-06, "rounds 0.35": 1.27e-06,
                 "shells": 1.57e-07, "flags": 7.72e-09, "range": 0.0}
F32_BOUND = BOUND_FACTOR * max(F32_DEVIATION.values())  # 2.0e-3: the random crystals hold pairs far closer than any bond, whose 1 / r
# terms carry the float32 error of d2 at many times the self potential; the ordered crystals of `textbook` deviate by 1.0e-7
MARGIN_GUARD = 1e-9  # a crystal whose nearest lattice point lies closer than this (relative) to G_cut^2 has no exact n_reciprocal


def describe(flags) -> str:
    return cb.describe(flags, FLAG_NAMES)


def parse_charges(charges):
    """{atomic number: charge} of a dict from element symbol or atomic number to charge, or of its string form "Na=1,Cl=-1"; a
    ValueError names what is wrong (an unknown symbol, a charge that is not a finite number, an element given twice)."""
    if isinstance(charges, str):
        items = []
        for part in charges.split(","):
            if not part.strip():
                continue
            if part.count("=") != 1:
                raise ValueError(f"charges: expected ELEMENT=CHARGE, got {part.strip()!r}")
            name, value = (t.strip() for t in part.split("="))
            try:
                items.append((int(name) if name.isdigit() else name, float(value)))
            except ValueError:
                raise ValueError(f"charges: {value!r} is not a number") from None
    elif isinstance(charges, dict):
        items = list(charges.items())
    else:
        items = list(charges)  # ((Z, charge), ...): the normalised form
    out = {}
    for name, value in items:
        if isinstance(name, str):
            if name not in SYMBOL_TO_Z:
                raise ValueError(f"charges: unknown element symbol {name!r}")
            z = SYMBOL_TO_Z[name]
        elif isinstance(name, Integral) and not isinstance(name, bool) and int(name) >= 1:
            z = int(name)
        else:
            raise ValueError(f"charges: an element is a symbol or an atomic number >= 1, got {name!r}")
        if not isinstance(value, Real) or isinstance(value, bool) or not math.isfinite(value):
            raise ValueError(f"charges: the charge of {name!r} must be a finite number, got {value!r}")
        if z in out:
            raise ValueError(f"charges: element {name!r} is given twice")
        out[z] = float(value)
    return out


@dataclass(frozen=True)
class EwaldParams:
    """charges: a dict from element symbol or atomic number to charge in e, or the string form "Na=1,Cl=-1" (kept as a sorted
    tuple of (atomic number, charge); None: the caller hands `ewald` the charges themselves); accuracy in (0, 1): both sums drop
    terms of about this relative size (1e-8); alpha in 1/A: the splitting parameter for every crystal, None (or 0) for the per
    crystal sqrt(pi) (n / V^2)^(1/6); max_shells (1..8; 8): the cap on the real-space images per axis, as the screen's -- a crystal
    that needs more is flagged CELL; max_index (1..127; 64): the largest |h_k| of the reciprocal box -- a crystal that needs more
    is flagged RANGE.  Starting values, not claims."""
    charges: object = None
    accuracy: float = 1e-8
    alpha: object = None
    max_shells: int = 8
    max_index: int = 64

    def __post_init__(self):
        if self.charges is not None:
            object.__setattr__(self, "charges", tuple(sorted(parse_charges(self.charges).items())))
        a = self.accuracy
        if not isinstance(a, Real) or isinstance(a, bool) or not 0.0 < a < 1.0:
            raise ValueError(f"accuracy must lie in (0, 1), got {a!r}")
        object.__setattr__(self, "accuracy", float(a))
        if not math.sqrt(-math.log(self.accuracy)) > 0.0:
            raise ValueError(f"accuracy {a!r} is 1 in float64")
        al = self.alpha
        if al is not None:
            if not isinstance(al, Real) or isinstance(al, bool) or not math.isfinite(al) or al < 0.0:
                raise ValueError(f"alpha must be None or a finite number >= 0 (0: per crystal), got {al!r}")
            object.__setattr__(self, "alpha", float(al) if al > 0.0 else None)
        for name, lo, hi in (("max_shells", 1, MAX_SHELLS), ("max_index", 1, MAX_INDEX)):
            v = getattr(self, name)
            if not isinstance(v, Integral) or isinstance(v, bool) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must lie in {lo}..{hi}, got {v!r}")
            object.__setattr__(self, name, int(v))

    @property
    def s(self):
        """sqrt(-ln accuracy): r_cut = s / alpha, G_cut = alpha s / pi."""
        return math.sqrt(-math.log(self.accuracy))


def resolve(ewald):
    """sample(ewald=...): None / False -> None, an EwaldParams with charges -> itself.  There are no default charges, so True is
    rejected like any other value."""
    if ewald is True:
        raise ValueError("ewald needs an EwaldParams(charges=...): there are no default charges")
    if ewald is not None and ewald is not False and not isinstance(ewald, EwaldParams):
        raise ValueError(f"ewald must be None or an EwaldParams(charges=...), got {ewald!r}")
    p = cb.resolve(ewald, EwaldParams, "ewald")
    if p is not None and not p.charges:
        raise ValueError("ewald: EwaldParams.charges is required (a dict from element to charge, or \"Na=1,Cl=-1\")")
    return p


def auto_alpha(n, volume):
    """Rule 1's per-crystal alpha, float64: sqrt(pi) cbrt(sqrt(n) / V)."""
    return math.sqrt(math.pi) * float(np.cbrt(math.sqrt(float(n)) / float(volume)))


def host_charges(atomic_numbers, params):
    """The charges [N] float32 of a result's atoms under `params`: NaN where no charge is given for the species (the mask state
    included), which the launch flags UNASSIGNED."""
    if params is None or not params.charges:
        raise ValueError("ewald: EwaldParams.charges is required")
    z = np.rint(np.asarray(atomic_numbers, dtype=np.float64).reshape(-1)).astype(np.int64)
    out = np.full(z.shape, np.nan, dtype=F32)
    for zz, q in params.charges:
        out[z == zz] = F32(q)
    return out


# ------------------------------------------------------------------------------------------------------- the device call
def ewald(frac, lattice, offsets, charges_or_atomic_numbers, params=None):
    """The Ewald sums of a batch on the GPU without an engine (arreau_crystal_ewald, one launch).  frac [N,3] float32, lattice
    [B,3,3] float32 (rows a, b, c) and offsets [B+1] int32 are contiguous tensors on one cuda device; the fourth argument is a
    tensor [N] on it: of a floating dtype the charges themselves (a NaN: no charge given), of an integer dtype the atomic numbers,
    which params.charges turns into charges.  Returns a dict of device tensors (RESULT_KEYS): the eight float64 [B] reals,
    n_pairs int64 [B], n_reciprocal and flags int32 [B], potential float64 [N].  Does not synchronise."""
    import ctypes

    import torch

    from .. import _hip
    _hip.require_gpu()
    p = params if params is not None else EwaldParams()
    dev, B, N = cb.check_batch("ewald", frac, lattice, offsets, None, types_optional=True)
    c = charges_or_atomic_numbers
    if c is None or tuple(c.shape) != (N,) or c.device != dev:
        raise ValueError(f"ewald: the charges or atomic numbers must be a [{N}] tensor on the cuda device of frac")
    if c.dtype.is_floating_point:
        charges = c.to(torch.float32).contiguous()
    else:
        if not p.charges:
            raise ValueError("ewald: atomic numbers need EwaldParams.charges")
        top = max(z for z, _ in p.charges) + 1
        lut = torch.full((top + 1,), float("nan"), dtype=torch.float32)
        for z, q in p.charges:
            lut[z] = q
        charges = lut.to(dev)[c.to(torch.int64).clamp(0, top)].contiguous()  # (index `top`: NaN, as every species without a charge)
    f64 = dict(device=dev, dtype=torch.float64)
    out = {k: torch.empty(B, **f64) for k in CRYSTAL_REALS}
    out["n_pairs"] = torch.empty(B, device=dev, dtype=torch.int64)
    out["n_reciprocal"], out["flags"] = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    out["potential"] = torch.empty(N, **f64)
    work = torch.empty(N, **f64)
    cp = _hip.EwaldParamsC(p.accuracy, p.alpha or 0.0, p.max_shells, p.max_index)
    r = _hip.EwaldResultC(*[_hip.ptr(t).value if t.numel() else None for t in [out[k] for k in RESULT_KEYS] + [work]])
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().arreau_crystal_ewald(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(offsets), _hip.ptr(charges), B, N,
                                                   ctypes.byref(cp), ctypes.byref(r), _hip.stream_ptr(dev)), "arreau_crystal_ewald")
    return out


def result_to_numpy(result):
    """The dict of `ewald` as host numpy arrays (synchronises)."""
    return cb.to_numpy(result)


def sample_arrays(result, charges, atomic_numbers, num_atoms):
    """What SampleResult.ewald and a crystals file hold (STORED_KEYS) of a `result_to_numpy` dict: its arrays, energy_per_atom [B]
    (NaN for a flagged or an empty crystal), and per atom `charge` (float32, NaN where none was given) and `species` (the
    atomic numbers: what the mean per element is taken over)."""
    out = {k: np.asarray(result[k]) for k in RESULT_KEYS}
    n = np.asarray(num_atoms, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        out["energy_per_atom"] = np.where(n > 0, out["energy"] / np.where(n > 0, n, 1.0), np.nan)
    out["charge"] = np.asarray(charges, dtype=F32).reshape(-1)
    out["species"] = np.rint(np.asarray(atomic_numbers, dtype=np.float64).reshape(-1)).astype(np.int64)
    if not out["species"].shape == out["charge"].shape == out["potential"].shape or out["energy"].shape != n.shape:
        raise ValueError("ewald.sample_arrays: the charges, atomic numbers and atom counts do not match the result")
    return out


def ewald_sample_result(result, params, device="cuda"):
    """The Ewald sums of a SampleResult (or a loaded crystals file) on the GPU, its float64 arrays cast to float32: the dict of
    `sample_arrays`."""
    import torch
    frac, lattice, off, _ = cb.upload(result, device)
    q = host_charges(result.atomic_numbers, params)
    return sample_arrays(result_to_numpy(ewald(frac, lattice, off, torch.as_tensor(q, device=frac.device), params)), q,
                         result.atomic_numbers, result.num_atoms)


def madelung(result, b, r0, formula_units=1):
    """The Madelung constant of crystal b of a result referred to the distance r0 in A, for unit charges: -E r0 / (K formula
    units).  With charges +-z divide by z^2."""
    return -float(np.asarray(result["energy"]).reshape(-1)[b]) * float(r0) / (K * formula_units)


# ------------------------------------------------------------------------------------------------------------ statistics
def stats_of(result, rank=0):
    """What the summary lines need, of one rank's (or the whole set's) arrays: the crystals with an energy, the sum, minimum and
    maximum of their energy_per_atom, the crystals flagged CHARGED, per element the atoms and their summed |potential|, the count
    per flag."""
    flags = np.asarray(result["flags"], dtype=np.int64).reshape(-1)
    e = np.asarray(result["energy_per_atom"], dtype=np.float64).reshape(-1)
    ok = ((flags & INVALID_MASK) == 0) & ~np.isnan(e)
    out = {"rank": cb.rank_of(rank), "crystals": int(flags.size), "energies": int(ok.sum()), "energy_sum": float(e[ok].sum()),
           "energy_min": float(e[ok].min()) if ok.any() else None, "energy_max": float(e[ok].max()) if ok.any() else None,
           "charged": int((ok & ((flags & CHARGED) != 0)).sum()), "elements": {}, "flags": cb.flag_counts(flags, FLAG_NAMES)}
    if result.get("species") is not None:
        z, phi = np.asarray(result["species"], dtype=np.int64).reshape(-1), np.asarray(result["potential"], dtype=np.float64).reshape(-1)
        done = ~np.isnan(phi)
        out["elements"] = {int(v): [int(((z == v) & done).sum()), float(np.abs(phi[(z == v) & done]).sum())] for v in np.unique(z[done])}
    return out


def total_stats(parts):
    lows, highs = [p["energy_min"] for p in parts if p["energy_min"] is not None], [p["energy_max"] for p in parts if p["energy_max"] is not None]
    elements = {}
    for p in parts:
        for k, (a, s) in p["elements"].items():
            have = elements.get(int(k), [0, 0.0])
            elements[int(k)] = [have[0] + a, have[1] + s]
    return {"rank": "total", "crystals": sum(p["crystals"] for p in parts), "energies": sum(p["energies"] for p in parts),
            "energy_sum": sum(p["energy_sum"] for p in parts), "energy_min": min(lows) if lows else None,
            "energy_max": max(highs) if highs else None, "charged": sum(p["charged"] for p in parts),
            "elements": dict(sorted(elements.items())), "flags": {n: sum(p["flags"][n] for p in parts) for _, n in FLAG_NAMES}}


def format_stats(st) -> str:
    """'ewald rank 0: 16 crystals, 15 energies; eV per atom mean -3.412, min -4.120, max -1.003; charged 20.0%; mean |potential|
    Na: 8.92 V, Cl: 8.92 V; flags UNASSIGNED 1'."""
    k = st["energies"]
    body = (f"eV per atom mean {st['energy_sum'] / k:.3f}, min {st['energy_min']:.3f}, max {st['energy_max']:.3f}; "
            f"charged {100.0 * st['charged'] / k:.1f}%") if k else "eV per atom n/a"
    per = ", ".join(f"{symbol_of(int(z))}: {s / a:.2f} V" for z, (a, s) in sorted((int(z), v) for z, v in st["elements"].items()) if a)
    return f"ewald {cb.who(st)}: {st['crystals']} crystals, {k} energies; {body}; mean |potential| {per or 'n/a'}; flags {cb.some(st['flags'])}"


def summary_lines(parts):
    """The per-rank lines and the total line of a list of stats_of dicts."""
    return cb.summary_lines(parts, format_stats, total_stats)


# ------------------------------------------------------------------------------------------------- the numpy restatement
def _sequential(x):
    """The sum of a float64 vector in its order, one rounding per addition (numpy's cumsum does not pair)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def cuts_of(n, volume, params, alpha=None):
    """(alpha, r_cut, G_cut) of a crystal of n atoms and float64 volume under `params` (rule 1); a finite `alpha` replaces the
    rule's (a flagged crystal's NaN does not)."""
    given = alpha is not None and math.isfinite(alpha)
    a = float(alpha) if given else params.alpha if params.alpha else auto_alpha(n, volume)
    return a, params.s / a, a * params.s / math.pi


def ewald_reference(frac, lattice, counts, charges, params=None, dtype=np.float64, exact_inputs=False, alpha=None, unbounded=False):
    """The rules in numpy from the float32 inputs: frac [N,3], lattice [B,3,3], counts [B] atoms per crystal, charges [N] (NaN: none
    given).  dtype float64 is the yardstick: positions, displacements and phases in float64, nothing of the kernel's operation
    order.  dtype float32 is the kernel's split -- the wrapped positions, the image shifts, the displacement and d2 one float32
    operation at a time (bit for bit, so n_pairs is the kernel's), the cut on that d2, the reduced phase and its sine and cosine
    rounded to float32; everything else float64 -- the arithmetic whose deviation from float64 is measured for the bound.
    `alpha` [B]: per-crystal values that replace rule 1's (a GPU test hands the device's own back, so that no count hangs on an
    ulp of cbrt).  exact_inputs (float64 only) takes frac and lattice as the float64 numbers they are.  unbounded (float64 only)
    lifts max_shells and max_index: the yardstick beyond the kernel's caps.
    Returns a namespace: the RESULT_KEYS arrays; `reciprocal_margin` [B], the relative distance | |G|^2 / G_cut^2 - 1 | of the
    crystal's nearest lattice point to the cut (inf where the box holds none); `pair_margin` [B], the same of the nearest pair's
    float64 d2 to r_cut^2; `box` [B,3], `entries` [B] (box entries of the half-space walk) and `rounds` [B] of 256; `images` [B,3];
    `smallest_term` [B], the smallest kept real-space |term| in volts (NaN without one).  NaN / 0 for a flagged crystal."""
    from scipy.special import erfc
    f32 = np.dtype(dtype) == np.float32
    if exact_inputs or unbounded:
        assert not f32
    if exact_inputs:
        frac, lattice = np.asarray(frac, dtype=np.float64).reshape(-1, 3), np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3)
        counts = [int(n) for n in counts]
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    else:
        frac, lattice, counts, _, first = cb.inputs(frac, lattice, counts, None)
    charges = np.ascontiguousarray(charges, dtype=F32).reshape(-1)
    assert charges.shape[0] == frac.shape[0]
    p = params if params is not None else EwaldParams()
    B, N = len(counts), frac.shape[0]
    nan = lambda: np.full(B, np.nan)
    out = SimpleNamespace(**{k: nan() for k in CRYSTAL_REALS}, n_pairs=np.zeros(B, np.int64), n_reciprocal=np.zeros(B, np.int32),
                          flags=np.zeros(B, np.int32), potential=np.full(N, np.nan), reciprocal_margin=nan(), pair_margin=nan(),
                          box=np.zeros((B, 3), np.int64), entries=np.zeros(B, np.int64), rounds=np.zeros(B, np.int64),
                          images=np.zeros((B, 3), np.int64), smallest_term=nan())
    for b, n in enumerate(counts):
        L, f, q32 = lattice[b], frac[first[b]:first[b + 1]], charges[first[b]:first[b + 1]]
        if not (np.isfinite(L).all() and np.isfinite(f).all()):
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
        al, r_cut, g_cut = cuts_of(n, V, p, None if alpha is None else np.asarray(alpha, dtype=np.float64).reshape(-1)[b])
        with np.errstate(all="ignore"):
            _, q_shell, cell_bad = cb.cell_f32(L.astype(F32), F32(r_cut), 0.0, p.max_shells)
        if cell_bad and not unbounded:
            out.flags[b] = CELL
            continue
        H = np.floor(g_cut * np.sqrt((A * A).sum(axis=1)))
        if not (H <= p.max_index).all() and not unbounded:
            out.flags[b] = RANGE
            continue
        if not np.isfinite(q32).all():
            out.flags[b] = UNASSIGNED
            continue
        H = H.astype(np.int64)
        q = q32.astype(np.float64)
        # ---- real space
        if f32:
            nk = np.maximum(1, np.ceil(q_shell)).astype(np.int64)
            pos, _, centre, s = cb.positions_and_shifts(f.astype(F32), L.astype(F32), nk, F32)
            cut2 = F32(r_cut * r_cut)
        else:
            nk = np.maximum(1, np.ceil(cb.cell_f64(A, r_cut)[1]).astype(np.int64) + 1)
            pos, _, centre, s = cb.positions_and_shifts(f.astype(np.float64), A, nk, np.float64)
            cut2 = r_cut * r_cut
        dt = F32 if f32 else np.float64
        out.images[b] = nk
        phi_real, pairs, overlap, near, small = np.zeros(n), 0, False, np.inf, np.inf
        for i in range(n):
            disp = ((pos[:, None, :] + s[None, :, :]).astype(dt) - pos[i][None, None, :]).astype(dt)
            sq = (disp * disp).astype(dt)
            d2 = ((sq[..., 0] + sq[..., 1]).astype(dt) + sq[..., 2]).astype(dt)
            own = np.zeros(d2.shape, bool)
            own[i, centre] = True
            keep = ~own & (d2 <= cut2)
            overlap |= bool((keep & (d2 == 0)).any())
            keep &= d2 > 0
            pairs += int(keep.sum())
            near = min(near, float(np.abs(d2[~own].astype(np.float64) / (r_cut * r_cut) - 1.0).min(initial=np.inf)))
            r = np.sqrt(d2[keep].astype(np.float64))
            qj = np.broadcast_to(q[:, None], d2.shape)[keep]
            terms = qj * erfc(al * r) / r
            small = min(small, K * float(np.abs(terms[terms != 0]).min(initial=np.inf)))
            phi_real[i] = terms.sum()
        if overlap:
            out.flags[b] = OVERLAP
            continue
        # ---- reciprocal space
        Rn = R / det
        h, k, l = [a.reshape(-1) for a in np.meshgrid(np.arange(0, H[0] + 1), np.arange(-H[1], H[1] + 1), np.arange(-H[2], H[2] + 1), indexing="ij")]
        half = (h > 0) | (k > 0) | ((k == 0) & (l > 0))
        G = (h[:, None] * Rn[0][None] + k[:, None] * Rn[1][None]) + l[:, None] * Rn[2][None]
        g2 = (G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2]
        keep = half & (g2 > 0) & (g2 <= g_cut * g_cut)
        out.reciprocal_margin[b] = np.abs(g2[half] / (g_cut * g_cut) - 1.0).min(initial=np.inf)
        out.box[b], out.entries[b], out.rounds[b] = H, h.size, -(-h.size // ROUND)
        hk, g2k = np.stack([h[keep], k[keep], l[keep]], axis=1), g2[keep]
        if f32:
            x = (f - np.floor(f)).astype(F32)
            x[x >= F32(1)] = F32(0)
            hf = hk.astype(F32)
            t = ((hf[:, 0:1] * x[None, :, 0] + hf[:, 1:2] * x[None, :, 1]).astype(F32) + hf[:, 2:3] * x[None, :, 2]).astype(F32)
            ang = 2.0 * math.pi * (t - np.rint(t)).astype(F32).astype(np.float64)
            c, sn = np.cos(ang).astype(F32).astype(np.float64), np.sin(ang).astype(F32).astype(np.float64)
        else:
            x = f.astype(np.float64)
            ang = 2.0 * math.pi * (hk.astype(np.float64) @ (x - np.floor(x)).T)
            c, sn = np.cos(ang), np.sin(ang)
        w = (2.0 / (math.pi * V)) * (np.exp(-(math.pi * math.pi / (al * al)) * g2k) / g2k)
        phi_rec = (w * (c @ q)) @ c + (w * (sn @ q)) @ sn
        # ---- self, background, energies
        Q, Qabs = _sequential(q), _sequential(np.abs(q))
        phi_self, phi_bg = (-2.0 * al / math.sqrt(math.pi)) * q, np.full(n, -math.pi * Q / (V * al * al))
        phi_real, phi_rec, phi_self, phi_bg = K * phi_real, K * phi_rec, K * phi_self, K * phi_bg  # rule 6: volts
        phi = ((phi_real + phi_rec) + phi_self) + phi_bg
        out.energy[b], out.real[b], out.reciprocal[b] = 0.5 * _sequential(q * phi), 0.5 * _sequential(q * phi_real), 0.5 * _sequential(q * phi_rec)
        out.self[b], out.background[b] = 0.5 * _sequential(q * phi_self), 0.5 * _sequential(q * phi_bg)
        out.net_charge[b], out.alpha[b], out.volume[b] = Q, al, V
        out.n_pairs[b], out.n_reciprocal[b] = pairs, 2 * int(keep.sum())
        out.potential[first[b]:first[b + 1]] = phi
        out.pair_margin[b], out.smallest_term[b] = near, small if np.isfinite(small) else np.nan
        out.flags[b] = CHARGED if abs(Q) > CHARGED_TOLERANCE * Qabs else 0
    return out
