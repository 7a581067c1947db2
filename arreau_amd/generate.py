"""Batch driver of the sampler: the role of main_diffusion_generate.py:52-94, sharded over GPUs.

Crystals are independent, so the crystal index is cut into contiguous slices, one per rank (one
process per GPU); every rank samples its slice in sub-batches and rank 0 gathers the `SampleResult`s
in crystal order.  The only communication is that final gather of host arrays
(`torch.distributed.gather_object`; RCCL/gloo are not on the data path).

    python -m torch.distributed.run --nproc-per-node 8 -m arreau_amd.generate --model_path last.ckpt \
        --num_crystals 8192 --num_atoms 20 --out out/crystals.npz

Conditioned generation (structure completion): `--template crystals.npz` (the wire format below, plus optional
`position_mask` [N] / `species_mask` [N] / `lattice_mask` [B] arrays) gives the batch; `--fix positions,species,lattice`
fixes those components wherever the file has no mask for them; `--samples_per_template K` tiles the templates K times.

Respaced sampling: `--num_steps K` runs K evenly spaced denoising steps instead of every timestep (DiffusionLoss.sample).

DDIM-style sampling: `--eta X` (0..1) scales the noise every step injects into positions and lengths; 0 makes them a function
of the initial state alone, 1 is the ancestral step; the usual companion of `--num_steps` (DiffusionLoss.sample).  Not with
`--symops`.

Second-order multistep sampling: `--multistep` extrapolates the deterministic `--eta 0` step with the previous step's prediction
(DPM-Solver++ 2M): the same one network evaluation per step, fewer `--num_steps` for the same solver error
(DiffusionLoss.sample).  Not with `--template`, `--symops`, corrector steps, resampling or an `--eta` other than 0.

Species control: `--elements Li,Fe,O` restricts the elements the sampler may choose to that set (symbols or atomic numbers; one
set for every crystal of every rank): no atom ends outside it or as the mask state.  `--species_temperature X` (>= 0) scales the
Gumbel draw of the species step; 0 draws nothing, which with `--eta 0` or `--multistep` makes the run a function of its initial
state in species too (DiffusionLoss.sample).  With every other option.

Starting from given crystals: `--start_from crystals.npz --start_t K` forward-noises the file's crystals to level K (1..T-1) and
denoises from there -- variants in the neighbourhood of the given structures; with `--invert` they are instead encoded up to
level K by DDIM inversion, species held, and then decoded (PONITA_DIFFUSION.noise_to / encode; sample(initial_state=...)).  The
file defines the batch (`--num_crystals` / `--num_atoms` are not used); every rank takes its contiguous share of it.
`--num_steps` then counts the steps from K down.  `--invert` is a deterministic round trip only with `--eta 0`.  Not with
`--template`, `--symops`, `--lattice_system`.

Predictor-corrector sampling: `--corrector_steps M` runs M Langevin corrector moves on the positions before every denoising
step, with the step-size rule's `--corrector_snr` (default 0.16; DiffusionLoss.sample).

RePaint resampling: `--resample_passes R --jump_length J` runs the denoising steps in blocks of J, each R times, jumping the
state back to the block's top before every pass after the first (DiffusionLoss.sample).

Lattice systems: `--lattice_system NAME` (cubic, tetragonal, orthorhombic, hexagonal, rhombohedral, monoclinic, triclinic) gives
every crystal that system's angles and tied lengths (DiffusionLoss.sample).

Space-group symmetry: `--symops FILE` (one operation per line in xyz form, e.g. `-x,y+1/2,-z+1/2`; `#` starts a comment) with
`--lattice_system NAME` and exactly one of `--orbits K` (K orbits of general positions) or `--symmetry_template crystals.npz`
(the first crystal's positions define the orbits) samples every crystal with its atoms in the orbits of the group the operations
generate (DiffusionLoss.sample).  The spec decides the atom count (`--num_atoms` is not used).  Not with `--template`.

Structural screen: `--screen` (thresholds `--min_distance`, `--min_volume`, `--search_radius`) screens every generated crystal on
the device at the end of its sampling call -- shortest contact over all periodic images, cell volume, mask state
(diffusion/screening.py) --, prints accepted / attempted and the count per flag for every rank and in total, and stores the
metrics as screen_* arrays in the output file.  `--require_valid [--max_rounds R]` (implies --screen) keeps generating until every
rank has its share of VALID crystals, or R rounds have passed (generate_valid_crystals); a shortfall is reported, not padded.

Duplicate detection: `--unique` (`--fp_r_max`, `--fp_sigma`, `--fp_tolerance`) fingerprints the crystals on the device
(diffusion/uniqueness.py).  Every rank reports unique / attempted within its own crystals; rank 0, after the gather of host arrays,
matches the whole set once on its own GPU, prints the total and stores those arrays as unique_* in the output file.  May be
combined with --screen / --require_valid; the two do not interact.

Structure match: `--match_to FILE` (`--ltol`, `--angle_tol`, `--stol`) matches every generated crystal on the device, at the end of
its sampling call, against every target of its composition in that crystals file (diffusion/structure_match.py) and keeps the best:
match rate (matched / attempted) and mean rms_norm and rms over the matched, per rank and in total, and match_* arrays in the
output file.  The optimal assignment only with `--assignment optimal`, no supercells (combine with a reduced target file), no volume scaling.

Coordination environments: `--coordination` (`--cn_tol`, `--cn_cutoff`) finds every atom's neighbours on the device
(diffusion/coordination.py) and stores coord_* arrays.  Bond order: `--bond_order` (the same two flags; with `--coordination` the
search is shared) adds the bond-angle histogram and the Steinhardt order parameters q_2 .. q_8 of every atom's shell
(diffusion/bond_order.py): the summed histogram, mean q4 and q6 overall and per element, the count per flag, and order_* arrays.
Voronoi cells: `--voronoi` (`--vor_tol`, `--vor_cutoff`) builds every atom's Voronoi cell on the device (diffusion/voronoi.py): the
histogram of cn (faces of weight >= vor_tol), mean cn and cn_eff overall and per element, the share of OPEN atoms, the count per flag,
and voronoi_* arrays.  Not CrystalNN: no radii, no electronegativities, no distance weighting, no probabilities.
Powder diffraction: `--xrd` (`--xrd_wavelength`, `--xrd_fwhm`, `--xrd_two_theta_min`, `--xrd_two_theta_max`, `--xrd_points`,
`--xrd_b_iso`, `--xrd_scattering`) writes every crystal's powder X-ray diffraction pattern on a fixed 2 theta grid on the device
(diffusion/xrd.py): the count per flag, the mean number of lattice points kept and the mean, minimum and maximum 2 theta of the
strongest peak, and xrd_* arrays.  Z-weighted point scatterers: no form-factor tables, no anomalous dispersion, no K alpha 2.
Electrostatics: `--ewald --ewald_charges Na=1,Cl=-1` (`--ewald_accuracy`, `--ewald_alpha`) writes every crystal's Ewald energy of
those point charges and every atom's site potential on the device (diffusion/ewald.py): the count per flag, the mean, minimum and
maximum energy per atom in eV, the share of crystals that are not neutral (CHARGED: a neutralising background is in the number),
the mean |potential| per element, and ewald_* arrays.  A crystal with an element that has no charge is flagged UNASSIGNED.  No
forces, no short-range repulsion (the energy alone favours collapse), no oxidation-state guessing.

Keyed sampling: `--keyed` (needs `--seed`) makes every crystal a function of (seed, key) alone (diffusion/keyed.py).  Every rank
uses the same seed; output slot k of `--num_crystals` has key k on its first attempt.  With `--require_valid`, attempt a of slot k
has key a * num_crystals + k and the slot keeps its first valid attempt; every rank retries only the slots of its slice that are
still open, up to `--max_rounds`, and a shortfall is reported, not padded.  The file (which then also holds `crystal_keys`) is the
same for every world size and every `--batch` -- up to where the score network changes its kernels with the size of a launch
(keyed.py, rule 5).  `--keys 17,4711` regenerates those slots alone.  `--template` and `--start_from` runs key a crystal by its
index in the file times `--samples_per_template` plus the copy.  Without `--keyed` nothing changes, `seed + rank` included.

Contact guidance: `--guide_contacts [--guide_min_distance D --guide_weight W]` steers every step away from contacts shorter than D
(diffusion/contact_guidance.py): where `--require_valid` throws a crystal with a short contact away and samples again, this pushes
the contact apart while the crystal is sampled.  With every other option (an `--invert` run guides the decode, not the encode).
XRD guidance: `--guide_xrd TARGETS.npz [--guide_xrd_weight W]` steers the positions towards a target powder pattern
(diffusion/xrd_guidance.py) on the grid of the `--xrd_*` flags: TARGETS.npz holds `pattern`, one row for every crystal or one per
crystal of a batch (any other file is read as a crystals file, whose patterns are computed under the same flags).  Structure solution
from a powder pattern: give the cell (`--template --fix lattice`, `--lattice_system`) and the composition.  Prints the mean,
minimum and maximum distance to the target at the last network evaluation and the flags, per rank and in total.
It prints, per rank and in total, the contacts below D, the penalty and the flags of the last network evaluation; `--screen`
still judges the final state.
"""
import argparse
import contextlib
import os
from typing import Callable, Optional

import numpy as np

from .diffusion import instruments
from .diffusion.diffusion_loss import SampleResult
from .diffusion.instruments import COMPLETE as INSTRUMENTS


def shard_range(num_items: int, world_size: int, rank: int):
    """Contiguous slice [start, stop) of `num_items` owned by `rank` (remainder to the first ranks)."""
    base, rem = divmod(num_items, world_size)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def _screen_stats(parts):
    """The per-rank statistics the parts carry (SampleResult.info[<an instrument's stats_key>]), each in one list; None when no
    part has any."""
    out = {}
    for e in INSTRUMENTS:
        stats = [st for p in parts if p is not None and p.info for st in p.info.get(e.stats_key, [])]
        if stats:
            out[e.stats_key] = stats
    return out or None


def concat_results(parts) -> SampleResult:
    """Crystal-order concatenation with the reference's index arrays (main_diffusion_generate.py:67-92).  An instrument's arrays
    are concatenated when every part has them (instruments.concat), and the parts' statistics are collected."""
    info = _screen_stats(parts)
    parts = [p for p in parts if p is not None and p.num_atoms is not None and len(p.num_atoms)]
    if not parts:
        return SampleResult(frac_x=np.empty((0, 3)), atomic_numbers=np.empty((0,)), lattice=np.empty((0, 3, 3)),
                            idx_start=np.empty((0,), dtype=np.int64), num_atoms=np.empty((0,), dtype=np.int64), info=info)
    num_atoms = np.concatenate([np.asarray(p.num_atoms) for p in parts])
    keys = None  # keyed sampling: carried when every part has them
    if all(getattr(p, "crystal_keys", None) is not None for p in parts):
        keys = np.concatenate([np.asarray(p.crystal_keys, dtype=np.int64) for p in parts])
    return SampleResult(
        crystal_keys=keys,
        frac_x=np.concatenate([p.frac_x for p in parts]), atomic_numbers=np.concatenate([p.atomic_numbers for p in parts]),
        lattice=np.concatenate([p.lattice for p in parts]), num_atoms=num_atoms, idx_start=np.cumsum(num_atoms) - num_atoms, info=info,
        **{e.field: instruments.concat(e, [getattr(p, e.field) for p in parts]) for e in INSTRUMENTS})


def select_crystals(res: SampleResult, keep) -> SampleResult:
    """The crystals of `res` where keep [B] is true, in their order (atoms, cells, the instruments' arrays; idx_start rebuilt)."""
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    num_atoms = np.asarray(res.num_atoms, dtype=np.int64)
    atoms = np.repeat(keep, num_atoms)
    kept = num_atoms[keep]
    return SampleResult(frac_x=np.asarray(res.frac_x)[atoms], atomic_numbers=np.asarray(res.atomic_numbers)[atoms],
                        lattice=np.asarray(res.lattice)[keep], num_atoms=kept, idx_start=np.cumsum(kept) - kept,
                        crystal_keys=np.asarray(res.crystal_keys)[keep] if getattr(res, "crystal_keys", None) is not None else None,
                        **{e.field: instruments.select(e, getattr(res, e.field), keep, atoms) for e in INSTRUMENTS})


FIX_KINDS = ("positions", "species", "lattice")


def parse_fix(text: str):
    """'positions,lattice' -> {'positions': True, 'species': False, 'lattice': True}."""
    kinds = [k.strip() for k in (text or "").split(",") if k.strip()]
    bad = [k for k in kinds if k not in FIX_KINDS]
    if bad:
        raise ValueError(f"--fix: unknown component(s) {bad}; choose from {list(FIX_KINDS)}")
    return {k: k in kinds for k in FIX_KINDS}


def load_template(filename: str, fix: dict):
    """A SampleCondition from a crystals.npz / .h5 file.  Mask arrays in the file win; otherwise `fix[kind]` (bool) applies
    to every atom / crystal."""
    from .diffusion.conditioning import SampleCondition
    from .diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    res = load_sample_results_from_hdf5(filename)
    masks = {}
    names = ("position_mask", "species_mask", "lattice_mask")
    if str(filename).endswith((".h5", ".hdf5")):
        import h5py
        with h5py.File(filename, "r") as fh:
            masks = {k: fh["crystals"][k][:] for k in names if k in fh["crystals"]}
    else:
        with np.load(filename) as z:
            masks = {k: z[k] for k in names if k in z.files}
    return SampleCondition.from_sample_result(res, fix_positions=masks.get("position_mask", fix["positions"]),
                                              fix_species=masks.get("species_mask", fix["species"]),
                                              fix_lattice=masks.get("lattice_mask", fix["lattice"]))


def template_batches(num_crystals: int, batch: int, rank: int = 0, world_size: int = 1):
    """The sub-batches [start, stop) of the (tiled) template crystals that `rank` samples: its contiguous shard_range slice,
    cut into pieces of at most `batch` crystals."""
    start, stop = shard_range(num_crystals, world_size, rank)
    return [(s, min(s + batch, stop)) for s in range(start, stop, batch)]


def _gather_results(local: SampleResult, rank: int, world_size: int, gather: Optional[Callable], unique=None):
    for e in INSTRUMENTS:  # an instrument that ran: this rank's statistics, unless the caller has set them
        arrays = getattr(local, e.field)
        if e.carried and arrays is not None and not (local.info or {}).get(e.stats_key):
            local.info = dict(local.info or {}, **{e.stats_key: [e.stats_of(arrays, rank)]})
    if unique is not None:  # duplicates within this rank's crystals, on its own device
        from .diffusion import uniqueness
        local.info = dict(local.info or {}, unique_stats=[uniqueness.stats_of(uniqueness.unique_sample_result(local, unique), rank)])
    if world_size == 1:
        return local
    if gather is None:
        import torch.distributed as dist

        def gather(obj):
            out = [None] * world_size if rank == 0 else None
            dist.gather_object(obj, out, dst=0)
            return out
    parts = gather(local)
    return concat_results(parts) if rank == 0 else None


def generate_from_template(sample_fn: Callable, condition, num_crystals_per_batch: int = 256, rank: int = 0,
                           world_size: int = 1, gather: Optional[Callable] = None, unique=None) -> Optional[SampleResult]:
    """sample_fn(condition) -> SampleResult (e.g. PONITA_DIFFUSION.sample(condition=...)) over this rank's slice of the
    condition's crystals.  Returns the concatenated result on rank 0 (None elsewhere when world_size > 1).  `unique` (a
    uniqueness.FingerprintParams): every rank also counts the duplicates among its own crystals (info["unique_stats"])."""
    mine = [sample_fn(condition.slice(a, b)) for a, b in template_batches(condition.B, num_crystals_per_batch, rank, world_size)]
    return _gather_results(concat_results(mine), rank, world_size, gather, unique)


def generate_n_crystals(sample_fn: Callable[[int, int], SampleResult], num_crystals: int, num_atoms_per_sample: int,
                        num_crystals_per_batch: int = 256, rank: int = 0, world_size: int = 1,
                        gather: Optional[Callable] = None, unique=None) -> Optional[SampleResult]:
    """sample_fn(num_atoms_per_sample, num_samples_in_batch) -> SampleResult  (e.g. PONITA_DIFFUSION.sample).
    Returns the concatenated result on rank 0 (None elsewhere when world_size > 1).  `unique`: as in generate_from_template."""
    start, stop = shard_range(num_crystals, world_size, rank)
    mine = []
    for s in range(start, stop, num_crystals_per_batch):
        mine.append(sample_fn(num_atoms_per_sample, min(num_crystals_per_batch, stop - s)))
    return _gather_results(concat_results(mine), rank, world_size, gather, unique)


def generate_valid_crystals(sample_fn: Callable[[int, int], SampleResult], num_crystals: int, num_atoms_per_sample: int,
                            num_crystals_per_batch: int = 256, rank: int = 0, world_size: int = 1,
                            gather: Optional[Callable] = None, max_rounds: int = 10, unique=None) -> Optional[SampleResult]:
    """generate_n_crystals that returns VALID crystals only.  sample_fn(num_atoms_per_sample, num_samples_in_batch) ->
    SampleResult WITH metrics (e.g. PONITA_DIFFUSION.sample(..., screen=criteria)).  Every rank refills its own shard_range slice: in
    each round it samples as many crystals as it still misses (in sub-batches of at most num_crystals_per_batch), keeps the
    valid ones in generation order, and stops when the slice is full or after `max_rounds` rounds.  Ranks do not talk to each
    other until the final gather, so a rank's crystals depend on its own generator state alone.  A shortfall is warned about
    and left in the statistics (SampleResult.info["screen_stats"], one entry per rank: attempted, accepted, the count per flag
    over every attempt, requested, rounds); nothing is padded."""
    import warnings

    from .diffusion.screening import stats_of
    if int(max_rounds) < 1:
        raise ValueError(f"max_rounds must be >= 1, got {max_rounds}")
    start, stop = shard_range(num_crystals, world_size, rank)
    want, kept, flags, have, rounds = stop - start, [], [], 0, 0
    while have < want and rounds < int(max_rounds):
        rounds += 1
        missing = want - have
        for s in range(0, missing, num_crystals_per_batch):
            res = sample_fn(num_atoms_per_sample, min(num_crystals_per_batch, missing - s))
            if res.metrics is None:
                raise ValueError("generate_valid_crystals: sample_fn must return the screen's metrics (sample(..., screen=...))")
            flags.append(np.asarray(res.metrics["flags"]))
            good = select_crystals(res, res.metrics["valid"])
            kept.append(good)
            have += len(good.num_atoms)
    local = concat_results(kept)
    local.info = {"screen_stats": [stats_of(np.concatenate(flags) if flags else np.empty(0, np.int64), rank, requested=want,
                                            rounds=rounds)]}
    if have < want:
        warnings.warn(f"generate_valid_crystals: rank {rank} has {have} valid crystals of the {want} requested after {rounds} "
                      f"round(s); the result is {want - have} short")
    return _gather_results(local, rank, world_size, gather, unique)


def generate_keyed(sample_keys: Callable, slots, num_crystals: int, num_crystals_per_batch: int = 256, rank: int = 0,
                   world_size: int = 1, gather: Optional[Callable] = None, require_valid: bool = False, max_rounds: int = 10,
                   unique=None) -> Optional[SampleResult]:
    """The keyed driver (diffusion/keyed.py: fill_slots): sample_keys(keys) -> SampleResult of the crystals with those keys (e.g.
    PONITA_DIFFUSION.sample(n, len(keys), seed=s, crystal_keys=keys); with require_valid: WITH metrics).  This rank's contiguous
    share of `slots` (slots of a run of num_crystals) is sampled under slot_key(slot, attempt, num_crystals); with require_valid
    a slot keeps its first valid attempt and only open slots are retried, up to max_rounds.  The crystals come back in slot
    order with their keys (SampleResult.crystal_keys; slot = key % num_crystals), so the gathered result does not depend on
    world_size or the batch size.  A shortfall is warned about and left in the statistics; nothing is padded."""
    import warnings

    from .diffusion import keyed
    valid_of = None
    if require_valid:
        def valid_of(res):
            if res.metrics is None:
                raise ValueError("generate_keyed: sample_keys must return the screen's metrics (sample(..., screen=...))")
            return res.metrics["valid"]
    start, stop = shard_range(len(slots), world_size, rank)
    mine = list(slots)[start:stop]
    accepted, attempts = keyed.fill_slots(sample_keys, mine, num_crystals, num_crystals_per_batch, valid_of, max_rounds)
    kept = []
    for slot, key, res, i in accepted:
        keep = np.zeros(len(np.asarray(res.num_atoms)), dtype=bool)
        keep[i] = True
        one = select_crystals(res, keep)
        one.crystal_keys = np.array([key], dtype=np.int64)
        kept.append(one)
    local = concat_results(kept)
    if require_valid:
        from .diffusion.screening import stats_of
        flags = [np.asarray(res.metrics["flags"]) for res, _, _ in attempts]
        rounds = 0 if not attempts else max(k // int(num_crystals) for _, _, keys in attempts for k in keys) + 1
        local.info = {"screen_stats": [stats_of(np.concatenate(flags) if flags else np.empty(0, np.int64), rank, requested=len(mine),
                                                rounds=rounds)]}
        if len(accepted) < len(mine):
            warnings.warn(f"generate_keyed: rank {rank} has {len(accepted)} valid crystals of the {len(mine)} requested after "
                          f"{rounds} round(s); the result is {len(mine) - len(accepted)} short")
    return _gather_results(local, rank, world_size, gather, unique)


def check_keyed_arguments(args, error):
    """The combinations of --keyed / --keys; `error(message)` reports a bad one.  Returns the slots to generate (None: not keyed)."""
    if not args.keyed:
        if args.keys is not None:
            error("--keys needs --keyed")
        return None
    if args.seed is None:
        error("--keyed needs --seed: a crystal is a function of (seed, key)")
    if args.keys is None:
        return list(range(args.num_crystals))
    if args.template is not None or args.start_from is not None:
        error("--keys names output slots of --num_crystals; not with --template / --start_from")
    from .diffusion import keyed
    try:
        return keyed.parse_keys(args.keys, args.num_crystals)
    except ValueError as e:
        error(str(e))


def save_sample_results(crystals: SampleResult, filename: str):
    """The reference's crystals.h5 layout (diffusion/inference/process_generated_crystals.py:8-15)."""
    from .diffusion.inference.process_generated_crystals import save_sample_results_to_hdf5
    return save_sample_results_to_hdf5(crystals, filename)


def _corrector_steps_arg(text: str) -> int:
    from .diffusion.corrector import check_corrector
    try:
        return check_corrector(int(text), 1.0)[0]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _corrector_snr_arg(text: str) -> float:
    from .diffusion.corrector import check_corrector
    try:
        return check_corrector(1, float(text))[1]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _eta_arg(text: str) -> float:
    from .diffusion.ddim import check_eta
    try:
        return check_eta(float(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _elements_arg(text: str):
    out = [int(e) if e.isdigit() else e for e in (part.strip() for part in text.split(",")) if e]
    if not out:
        raise argparse.ArgumentTypeError("--elements needs at least one element symbol or atomic number")
    return out


def _species_temperature_arg(text: str) -> float:
    from .diffusion.species import validate_temperature
    try:
        return validate_temperature(float(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _resample_passes_arg(text: str) -> int:
    from .diffusion.resampling import check_resampling
    try:
        return check_resampling(int(text), 1)[0]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _jump_length_arg(text: str) -> int:
    from .diffusion.resampling import check_resampling
    try:
        return check_resampling(1, int(text))[1]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_path", type=str, required=True)
    ap.add_argument("--num_crystals", type=int, default=10)
    ap.add_argument("--num_atoms", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", type=str, default="out/crystals.npz")
    ap.add_argument("--seed", type=int, default=None, help="seed of the host/device generators (rank is added; with --keyed: the "
                    "seed of every crystal's stream, the same on every rank)")
    ap.add_argument("--keyed", action="store_true",
                    help="keyed sampling: every crystal is a function of (--seed, its key) alone, so the output does not depend on "
                         "the number of ranks or --batch; slot k has key k (needs --seed)")
    ap.add_argument("--keys", type=str, default=None, metavar="LIST",
                    help="--keyed: regenerate only these comma-separated output slots of --num_crystals (e.g. 17,4711)")
    ap.add_argument("--template", type=str, default=None,
                    help="crystals.npz / .h5 of templates (optional position_mask / species_mask / lattice_mask arrays)")
    ap.add_argument("--fix", type=str, default="", help="components fixed where the template has no mask: "
                    "comma-separated subset of positions,species,lattice")
    ap.add_argument("--samples_per_template", type=int, default=1, help="the templates are tiled this many times")
    ap.add_argument("--num_steps", type=int, default=None,
                    help="respaced sampling: this many evenly spaced denoising steps (2..T-1; default: every timestep)")
    ap.add_argument("--eta", type=_eta_arg, default=None,
                    help="DDIM-style sampling: scale of the noise every step injects into positions and lengths (0..1; 0 = "
                         "deterministic, 1 = ancestral; default: the sampler without it)")
    ap.add_argument("--multistep", action="store_true",
                    help="second-order multistep sampling: the deterministic --eta 0 step extrapolated with the previous step's "
                         "prediction (fewer --num_steps for the same solver error); not with --template, --symops, corrector steps, "
                         "resampling or an --eta other than 0")
    ap.add_argument("--elements", type=_elements_arg, default=None, metavar="LIST",
                    help="species control: comma-separated element symbols and / or atomic numbers the sampler may choose from "
                         "(e.g. Li,Fe,O); one set for every crystal; no atom ends outside it or as the mask state")
    ap.add_argument("--species_temperature", type=_species_temperature_arg, default=1.0, metavar="X",
                    help="species control: scale of the Gumbel draw of the species step (>= 0; 1 = the sampler as it is, 0 = no "
                         "draw: deterministic species)")
    ap.add_argument("--start_from", type=str, default=None, metavar="FILE",
                    help="start from the crystals of this crystals.npz / .h5 instead of the prior: noised to --start_t (or, with "
                         "--invert, encoded up to it), then sampled; the file defines the batch")
    ap.add_argument("--start_t", type=int, default=None, metavar="K", help="--start_from: the level the sampler enters at (1..T-1)")
    ap.add_argument("--invert", action="store_true",
                    help="--start_from: reach --start_t by DDIM inversion (species held) instead of forward noising")
    ap.add_argument("--corrector_steps", type=_corrector_steps_arg, default=0,
                    help="predictor-corrector sampling: Langevin corrector moves on the positions per denoising step (0..16)")
    ap.add_argument("--corrector_snr", type=_corrector_snr_arg, default=0.16,
                    help="signal-to-noise ratio of the corrector's step-size rule (finite, > 0)")
    ap.add_argument("--resample_passes", type=_resample_passes_arg, default=1,
                    help="RePaint resampling: passes per block of denoising steps (1..64; 1 = no resampling)")
    ap.add_argument("--jump_length", type=_jump_length_arg, default=10,
                    help="RePaint resampling: denoising steps per block (>= 1)")
    ap.add_argument("--lattice_system", type=str, default=None, choices=_lattice_system_choices(),
                    help="sample crystals of this lattice system: its angles, tied lengths (default: the reference's angles)")
    ap.add_argument("--symops", type=str, default=None,
                    help="space-group symmetry: a file of generators in xyz form, one per line (needs --lattice_system and one of "
                         "--orbits / --symmetry_template)")
    ap.add_argument("--orbits", type=int, default=None, help="space-group symmetry: K orbits of general positions")
    ap.add_argument("--symmetry_template", type=str, default=None,
                    help="space-group symmetry: crystals.npz / .h5 whose first crystal's positions define the orbits")
    add_screen_arguments(ap)
    ap.add_argument("--screen", action="store_true",
                    help="screen every generated crystal on the device (shortest contact, cell volume, mask state): summary + "
                         "screen_* arrays in the output file")
    ap.add_argument("--require_valid", action="store_true",
                    help="keep generating until every rank has its share of valid crystals (implies --screen; not with --template)")
    ap.add_argument("--max_rounds", type=int, default=10, help="--require_valid: refill rounds per rank (>= 1)")
    ap.add_argument("--unique", action="store_true",
                    help="duplicate detection on the device: unique / attempted per rank and in total + unique_* arrays in the output file")
    add_fingerprint_arguments(ap)
    ap.add_argument("--find_symmetry", action="store_true",
                    help="find every generated crystal's symmetry operations and point group on the device: histogram per rank and "
                         "in total + sym_* arrays in the output file; with --symops, how many crystals contain that group")
    add_symmetry_search_arguments(ap)
    ap.add_argument("--reduce_cell", action="store_true",
                    help="reduce every generated crystal to its primitive, Delaunay-reduced cell on the device (tolerance --symprec): "
                         "histogram of multiplicities and flags per rank and in total + reduced_* arrays in the output file")
    ap.add_argument("--symmetrize", action="store_true",
                    help="symmetrize every generated crystal on the device with the operations found within --symprec: exact "
                         "orbits, averaged positions and cell; histogram of orbit counts and flags and the largest displacement "
                         "per rank and in total + symmetrized_* arrays in the output file")
    ap.add_argument("--conventional_cell", action="store_true",
                    help="give every generated crystal its conventional cell on the device (reduction, symmetry search on the reduced "
                         "cell, conventional basis; tolerance --symprec): centring, Bravais lattice and Pearson symbol; histogram of "
                         "Bravais lattices and flags per rank and in total + conventional_* arrays in the output file")
    ap.add_argument("--match_to", default=None, metavar="FILE",
                    help="match every generated crystal against the targets of a crystals file on the device (the best target of its "
                         "composition): match rate and mean RMSD per rank and in total + match_* arrays in the output file")
    add_structure_match_arguments(ap)
    ap.add_argument("--coordination", action="store_true",
                    help="find every atom's neighbours on the device (all atoms and images within (1 + cn_tol) times its nearest "
                         "distance and within cn_cutoff): histogram of coordination numbers, mean per element, share of mutual bonds "
                         "and flags per rank and in total + coord_* arrays in the output file")
    ap.add_argument("--bond_order", action="store_true",
                    help="bond angles and Steinhardt order parameters on the device, of every atom's coordination shell (--cn_tol, "
                         "--cn_cutoff): summed angle histogram, mean q4 and q6 overall and per element and flags per rank and in "
                         "total + order_* arrays in the output file")
    add_coordination_arguments(ap)
    ap.add_argument("--voronoi", action="store_true",
                    help="build every atom's Voronoi cell on the device (--vor_tol, --vor_cutoff): solid-angle-weighted neighbours and "
                         "atom volumes; histogram of cn, mean cn and cn_eff overall and per element, share of OPEN atoms and flags "
                         "per rank and in total + voronoi_* arrays in the output file")
    add_voronoi_arguments(ap)
    ap.add_argument("--xrd", action="store_true",
                    help="write every crystal's powder X-ray diffraction pattern on a fixed 2 theta grid on the device (--xrd_wavelength, "
                         "--xrd_fwhm, --xrd_two_theta_min, --xrd_two_theta_max, --xrd_points, --xrd_b_iso, --xrd_scattering): flags, mean "
                         "lattice points kept and the strongest peak's 2 theta per rank and in total + xrd_* arrays in the output file")
    add_xrd_arguments(ap)
    ap.add_argument("--ewald", action="store_true",
                    help="write every crystal's Ewald electrostatic energy and every atom's site potential on the device, for the point "
                         "charges of --ewald_charges (--ewald_accuracy, --ewald_alpha): flags, energy per atom, the share of charged "
                         "crystals and the mean |potential| per element per rank and in total + ewald_* arrays in the output file")
    add_ewald_arguments(ap)
    ap.add_argument("--guide_contacts", action="store_true",
                    help="contact guidance: steer every sampling step away from contacts shorter than --guide_min_distance (the "
                         "gradient of a contact penalty added to the predicted eps on the device); prints the contacts and flags of "
                         "the last network evaluation per rank and in total")
    ap.add_argument("--guide_min_distance", type=float, default=0.5, help="guide_contacts: contacts below this many A are pushed apart")
    ap.add_argument("--guide_weight", type=float, default=0.5,
                    help="guide_contacts: the descent step on the predicted clean structure (0.5 resolves an isolated contact)")
    ap.add_argument("--guide_xrd", type=str, default=None, metavar="TARGETS.npz",
                    help="XRD guidance: steer the positions towards the powder pattern(s) `pattern` of this file ([n_points] or one row per "
                         "crystal of a batch, on the grid of the --xrd_* flags; another file type: a crystals file, whose patterns are "
                         "computed); prints the distance to the target and the flags of the last network evaluation per rank and in total")
    ap.add_argument("--guide_xrd_weight", type=float, default=2.0,
                    help="guide_xrd: the descent step in A^2 on the predicted clean structure (2.0: a starting value, not a claim)")
    return ap


def check_xrd_guidance_arguments(args, error):
    """The XrdGuidance --guide_xrd asks for, or None; `error(message)` reports a bad value or a file that cannot be read."""
    if not args.guide_xrd:
        return None
    from .diffusion.xrd_guidance import XrdGuidance
    params = instrument_params("xrd", args, error)
    try:
        if args.guide_xrd.endswith(".npz"):
            with np.load(args.guide_xrd) as z:
                target = np.array(z["pattern"])
        else:
            target = load_targets(args.guide_xrd, error, "--guide_xrd")
        return XrdGuidance(target, weight=args.guide_xrd_weight, params=params)
    except (OSError, KeyError, ValueError) as e:
        error(f"--guide_xrd: {e}")


def check_guidance_arguments(args, error):
    """The ContactGuidance --guide_contacts asks for, or None; `error(message)` reports a bad value."""
    if not args.guide_contacts:
        return None
    from .diffusion.contact_guidance import ContactGuidance
    try:
        return ContactGuidance(min_distance=args.guide_min_distance, weight=args.guide_weight)
    except ValueError as e:
        error(f"--guide_contacts: {e}")


def add_coordination_arguments(ap):
    """The flags of the coordination search, shared with `python -m arreau_amd.screen`; --bond_order reads them too."""
    ap.add_argument("--cn_tol", type=float, default=0.1,
                    help="coordination: a neighbour lies within (1 + cn_tol) times the atom's nearest distance (0.1: a starting value, not a claim)")
    ap.add_argument("--cn_cutoff", type=float, default=6.0, help="coordination: nothing beyond this distance in A is a neighbour")


def add_voronoi_arguments(ap):
    """The flags of the Voronoi construction, shared with `python -m arreau_amd.screen`."""
    ap.add_argument("--vor_tol", type=float, default=0.05,
                    help="voronoi: a face counts as a neighbour when its solid angle is at least vor_tol times the atom's largest "
                         "(0.05: a starting value, not a claim)")
    ap.add_argument("--vor_cutoff", type=float, default=6.0,
                    help="voronoi: the atoms within this distance in A may bound a cell; an atom whose cell they do not close is OPEN")


def add_xrd_arguments(ap):
    """The flags of the powder diffraction pattern, shared with `python -m arreau_amd.screen` (starting values, not claims)."""
    ap.add_argument("--xrd_wavelength", type=float, default=1.54184, help="xrd: the wavelength in A (1.54184: Cu K alpha)")
    ap.add_argument("--xrd_fwhm", type=float, default=0.2, help="xrd: the full width at half maximum of every reflection in degrees")
    ap.add_argument("--xrd_two_theta_min", type=float, default=5.0, help="xrd: the first grid value in degrees")
    ap.add_argument("--xrd_two_theta_max", type=float, default=90.0, help="xrd: the last grid value in degrees (at most 160)")
    ap.add_argument("--xrd_points", type=int, default=1701, help="xrd: the number of grid values, ends included (2..4096)")
    ap.add_argument("--xrd_b_iso", type=float, default=0.0, help="xrd: one isotropic Debye-Waller B in A^2 for every atom")
    ap.add_argument("--xrd_scattering", type=str, default="Z", choices=("Z", "unit"),
                    help="xrd: an atom's amplitude: its atomic number (the forward-scattering limit of the form factor) or 1")


def add_ewald_arguments(ap):
    """The flags of the Ewald sum, shared with `python -m arreau_amd.screen`."""
    ap.add_argument("--ewald_charges", type=str, default=None, metavar="Na=1,Cl=-1",
                    help="ewald: the charge in e of every element, by symbol or atomic number; an element without one flags its crystals UNASSIGNED")
    ap.add_argument("--ewald_accuracy", type=float, default=1e-8, help="ewald: both sums drop terms of about this relative size")
    ap.add_argument("--ewald_alpha", type=float, default=None,
                    help="ewald: the splitting parameter in 1/A for every crystal (default: per crystal sqrt(pi) (n / V^2)^(1/6))")


def check_ewald_arguments(asked, error):
    """--ewald needs charges: `error(message)` reports their absence before any work."""
    if asked.get("ewald") is not None and not asked["ewald"].charges:
        error("--ewald needs --ewald_charges (for instance Na=1,Cl=-1)")


def add_structure_match_arguments(ap):
    """The tolerance flags of the structure match, shared with `python -m arreau_amd.screen`."""
    ap.add_argument("--ltol", type=float, default=0.2, help="match_to: relative tolerance on the cell lengths (StructureMatcher's default)")
    ap.add_argument("--angle_tol", type=float, default=5.0, help="match_to: tolerance on the cell angles, degrees")
    ap.add_argument("--stol", type=float, default=0.3, help="match_to: a pair matches when rms / (V / n)^(1/3) is at most this")
    ap.add_argument("--assignment", choices=("nearest", "optimal"), default="nearest",
                    help="match_to: what becomes of a candidate whose nearest-partner map is not one-to-one -- nearest: it is dropped; "
                         "optimal: it gets the optimal assignment (StructureMatcher's)")


def instrument_params(keyword, args, error):
    """The parameters of one instrument (its sample() keyword: instruments.COMPLETE_KEYWORDS) from its flags -- screen: a ScreenCriteria,
    unique: a FingerprintParams, find_symmetry: a SymmetrySearchParams, reduce_cell: a CellReductionParams, symmetrize: a
    SymmetrizeParams, match_to: a StructureMatchParams, conventional_cell: a ConventionalCellParams, coordination: a CoordinationParams, bond_order: a BondOrderParams, voronoi: a VoronoiParams, xrd: an XrdParams, ewald: an EwaldParams; what has no flag keeps its default.  `error(message)` reports a bad value."""
    e = instruments.COMPLETE_KEYWORDS[keyword]
    try:
        return getattr(e.module, e.params)(**{name: getattr(args, flag) for name, flag in e.flags})
    except ValueError as err:
        error(f"{e.label}: {err}")


def instrument_lines(keyword, res, parts=None):
    """The lines one instrument's flag prints for a result that holds its arrays: its statistics per rank (`parts`: what the ranks
    carried; None: the result as one set) and in total."""
    e = instruments.COMPLETE_KEYWORDS[keyword]
    return instruments.summary_lines(e, getattr(res, e.field), parts)


def load_targets(filename, error, flag="--match_to"):
    """The crystals file of `flag` (--match_to, --start_from); `error(message)` reports a file that cannot be read."""
    from .diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    try:
        return load_sample_results_from_hdf5(filename)
    except (OSError, KeyError, ValueError) as e:
        error(f"{flag}: {e}")


def add_symmetry_search_arguments(ap):
    """The tolerance flag of the symmetry search, the cell reduction and the symmetrization, shared with `python -m arreau_amd.screen`."""
    ap.add_argument("--symprec", type=float, default=0.1,
                    help="find_symmetry / reduce_cell / symmetrize / conventional_cell: tolerance in A on cell lengths and atom distances (0.1: a starting value, not a claim)")


def symmetry_lines(res, parts=None, spec=None):
    """`instrument_lines` of the symmetry search and, with `spec`, the crystals that contain its group."""
    from .diffusion import symmetry_search
    lines = instrument_lines("find_symmetry", res, parts)
    if spec is not None:
        lines.append(symmetry_search.contains_line(res.symmetry, spec))
    return lines


def add_fingerprint_arguments(ap):
    """The fingerprint flags shared with `python -m arreau_amd.screen`."""
    ap.add_argument("--fp_r_max", type=float, default=6.0, help="unique: the fingerprint covers distances up to this many A")
    ap.add_argument("--fp_sigma", type=float, default=0.1, help="unique: Gaussian smearing of a contact, A")
    ap.add_argument("--fp_tolerance", type=float, default=0.01, help="unique: crystals of one formula within this distance (1 - cos) / 2 are duplicates")


def unique_lines(res, params, against=None, device="cuda"):
    """Match the whole set once (with itself; with `against`, also with that set) and return the lines to print: the per-rank
    lines the parts carried, the total, and the novelty line.  Stores the whole-set arrays in res.uniqueness."""
    from .diffusion import uniqueness
    res.uniqueness = uniqueness.unique_sample_result(res, params, device=device)
    parts = sorted((res.info or {}).get("unique_stats", []), key=lambda st: st["rank"])
    lines = [uniqueness.format_stats(st) for st in parts] + [uniqueness.format_stats(uniqueness.stats_of(res.uniqueness, "total"))]
    if against is not None:
        novel = uniqueness.unique_sample_result(res, params, against=against, device=device)
        lines.append(uniqueness.format_stats(uniqueness.stats_of(novel, "total"), "novel") + f"; against {len(against.num_atoms)} crystals")
    return lines


def add_screen_arguments(ap):
    """The criteria flags shared with `python -m arreau_amd.screen`."""
    ap.add_argument("--min_distance", type=float, default=0.5, help="screen: contacts below this many A are CLOSE")
    ap.add_argument("--min_volume", type=float, default=0.1, help="screen: cells below this many A^3 are flagged CELL")
    ap.add_argument("--search_radius", type=float, default=3.0, help="screen: periodic images are searched out to this many A")


def check_screen_arguments(args, error):
    """The ScreenCriteria --screen / --require_valid ask for, or None; `error(message)` reports a bad combination."""
    if args.require_valid and args.template is not None:
        error("--require_valid cannot be combined with --template (conditioned generation)")
    if args.max_rounds < 1:
        error("--max_rounds must be >= 1")
    if not (args.screen or args.require_valid):
        return None
    return instrument_params("screen", args, error)


def check_start_arguments(args, error):
    """The combinations of --start_from / --start_t / --invert; `error(message)` reports a bad one.  True when a start file is given."""
    if args.start_from is None:
        if args.start_t is not None or args.invert:
            error("--start_t / --invert need --start_from")
        return False
    for flag in ("template", "symops", "lattice_system"):
        if getattr(args, flag) is not None:
            error(f"--start_from cannot be combined with --{flag}")
    if args.require_valid:
        error("--start_from cannot be combined with --require_valid")
    if args.start_t is None or args.start_t < 1:
        error("--start_from needs --start_t K with K >= 1 (the level the sampler enters at)")
    return True


def generate_from_crystals(start_fn: Callable, crystals: SampleResult, num_crystals_per_batch: int = 256, rank: int = 0,
                           world_size: int = 1, gather: Optional[Callable] = None, unique=None) -> Optional[SampleResult]:
    """start_fn(crystals) -> SampleResult (e.g. noise_to or encode, then sample(initial_state=...)) over this rank's contiguous
    share of the given crystals, in sub-batches.  Returns the concatenated result on rank 0 (None elsewhere when world_size > 1)."""
    n = len(np.asarray(crystals.num_atoms))
    mine = []
    for a, b in template_batches(n, num_crystals_per_batch, rank, world_size):
        keep = np.zeros(n, dtype=bool)
        keep[a:b] = True
        mine.append(start_fn(select_crystals(crystals, keep)))
    return _gather_results(concat_results(mine), rank, world_size, gather, unique)


def load_symmetry(args, error):
    """The SymmetrySpec of the --symops options (None without them); `error(message)` reports a bad combination."""
    if args.symops is None:
        if args.orbits is not None or args.symmetry_template is not None:
            error("--orbits / --symmetry_template need --symops")
        return None
    if args.template is not None:
        error("--symops cannot be combined with --template (conditioned generation)")
    if args.lattice_system is None:
        error("--symops needs --lattice_system")
    if (args.orbits is None) == (args.symmetry_template is None):
        error("--symops needs exactly one of --orbits K and --symmetry_template FILE")
    from .diffusion import symmetry
    try:
        ops = symmetry.read_symops(args.symops)
        if args.orbits is not None:
            if args.orbits < 1:
                error("--orbits must be >= 1")
            return symmetry.SymmetrySpec.general_positions(ops, args.orbits, args.lattice_system)
        from .diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
        tmpl = load_sample_results_from_hdf5(args.symmetry_template)
        n0 = int(np.asarray(tmpl.num_atoms)[0])
        frac = np.asarray(tmpl.frac_x)[:n0]
        return symmetry.SymmetrySpec.from_template(frac, ops, args.lattice_system)
    except (OSError, ValueError) as e:
        error(f"--symops: {e}")


@contextlib.contextmanager
def _device_turn(lock_path):
    """Ranks that SHARE one device take turns on it: the file lock is held around a sampler call and released once the device
    has finished it."""
    import fcntl

    import torch
    with open(lock_path, "a") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            yield
            torch.cuda.synchronize()
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _lattice_system_choices():
    from .diffusion.lattice_systems import SYSTEMS
    return SYSTEMS


def main():
    import torch
    ap = build_parser()
    args = ap.parse_args()
    start = check_start_arguments(args, ap.error)
    slots = check_keyed_arguments(args, ap.error)
    guide = check_guidance_arguments(args, ap.error)
    guide_parts = []  # contact guidance: the last-evaluation statistics of every batch this rank sampled
    xguide = check_xrd_guidance_arguments(args, ap.error)
    xguide_parts = []  # XRD guidance: the same
    spec = load_symmetry(args, ap.error)
    if spec is not None and args.eta is not None:
        ap.error("--eta is not supported with --symops")
    if args.multistep:
        from .diffusion.multistep import check_multistep
        try:
            check_multistep(True, eta=args.eta, condition=args.template, corrector_steps=args.corrector_steps,
                            resample_passes=args.resample_passes, symmetry=spec)
        except ValueError as e:
            ap.error(str(e).replace("condition=", "--template").replace("symmetry=", "--symops"))
    asked = {"screen": check_screen_arguments(args, ap.error)}  # per instrument, by its sample() keyword: its parameters, or None
    for e in INSTRUMENTS[1:]:
        asked[e.keyword] = instrument_params(e.keyword, args, ap.error) if getattr(args, e.keyword) else None
    check_ewald_arguments(asked, ap.error)
    if args.match_to:
        asked["match_to"] = (load_targets(args.match_to, ap.error), asked["match_to"], "any")
    unique = asked["unique"]  # (no sample() keyword here: every rank matches its own crystals, rank 0 the whole set)
    keywords = {k: v for k, v in asked.items() if k != "unique"}
    condition = load_template(args.template, parse_fix(args.fix)).tile(args.samples_per_template) if args.template else None
    start_crystals = load_targets(args.start_from, ap.error, "--start_from") if start else None
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if start and args.invert and args.eta != 0.0 and rank == 0:
        print("note: --invert without --eta 0 decodes stochastically (positions and lengths are then no function of the encoded state)")
    # ARREAU_GENERATE_BACKEND=gloo + ARREAU_GENERATE_ONE_DEVICE=1 rehearse several ranks on a one-GPU box (the only
    # communication is the final gather of host arrays, so the backend is not on the data path)
    if os.environ.get("ARREAU_GENERATE_ONE_DEVICE", "0") == "1":
        local_rank = 0
    backend = os.environ.get("ARREAU_GENERATE_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    from .diffusion.inference.visualize_crystal import VisualizationSetting
    from .lightning_wrappers.diffusion import PONITA_DIFFUSION
    model = PONITA_DIFFUSION.load_from_checkpoint(args.model_path, map_location=f"cuda:{local_rank}", strict=False)
    if start:
        from .diffusion import inversion
        try:  # (a bad --start_t / --num_steps fails before sampling)
            inversion.check_level(model.diffusion_loss.T, args.start_t, "--start_t")
            inversion.schedule_from(model.diffusion_loss.T, args.start_t, num_steps=args.num_steps)
        except ValueError as e:
            ap.error(str(e))
    elif args.num_steps is not None:
        from .diffusion import respacing
        respacing.resolve_schedule(model.diffusion_loss.T, num_steps=args.num_steps)  # (a bad --num_steps fails before sampling)
    species_kw = dict(elements=args.elements, species_temperature=args.species_temperature)
    if args.elements is not None or args.species_temperature != 1.0:
        from .diffusion import species as species_mod
        try:  # (a bad --elements fails before sampling)
            row = species_mod.resolve_elements(args.elements, model.hparams.z_table, 1)[0]
        except ValueError as e:
            ap.error(str(e).replace("elements:", "--elements:"))
        if rank == 0:
            print(f"species control: elements {'any' if args.elements is None else 'Z in {' + species_mod.describe(row, model.hparams.z_table) + '}'}"
                  f", species temperature {args.species_temperature:g}")
    if args.seed is not None and not args.keyed:  # (a keyed run reads no generator)
        torch.manual_seed(args.seed + rank)
        np.random.seed(args.seed + rank)
    keyed_kw = lambda keys: dict(seed=args.seed, crystal_keys=[int(k) for k in keys]) if args.keyed else {}
    # ARREAU_GENERATE_GPU_LOCK=<file>: ranks that SHARE one device (the one-GPU rehearsal above) take turns on it -- a file
    # lock held around each sampler call.  On a node every rank owns its GPU and the variable is not set.
    lock_path = os.environ.get("ARREAU_GENERATE_GPU_LOCK")

    def guided(res):  # keeps the batch's guidance statistics (the drivers carry the instruments' alone)
        if guide is not None:
            from .diffusion import contact_guidance as guidance_mod
            guide_parts.append(guidance_mod.stats_of(res.info["contact_guidance"], rank))
        if xguide is not None:
            from .diffusion import xrd_guidance as xrd_guidance_mod
            xguide_parts.append(xrd_guidance_mod.stats_of(res.info["xrd_guidance"], rank))
        return res

    def fn(n, b, cond=None, keys=None):
        with _device_turn(lock_path) if lock_path else contextlib.nullcontext():
            return guided(model.sample(n, b, VisualizationSetting.NONE, False, condition=cond, num_steps=args.num_steps, **keyed_kw(keys),
                                       corrector_steps=args.corrector_steps, corrector_snr=args.corrector_snr,
                                       resample_passes=args.resample_passes, jump_length=args.jump_length,
                                       lattice_system=args.lattice_system, symmetry=spec, eta=args.eta, multistep=args.multistep,
                                       contact_guidance=guide, xrd_guidance=xguide, **species_kw, **keywords))
    def start_fn(crystals):
        with _device_turn(lock_path) if lock_path else contextlib.nullcontext():
            keys = crystals.crystal_keys if args.keyed else None  # (the crystal's index in the file: set below)
            state = (model.encode(crystals, t=args.start_t, num_steps=args.num_steps) if args.invert
                     else model.noise_to(crystals, args.start_t, **keyed_kw(keys)))
            return guided(model.sample(visualization_setting=VisualizationSetting.NONE, initial_state=state, num_steps=args.num_steps,
                                       **keyed_kw(keys),
                                       use_constant_atomic_symbols=True if args.invert else None, corrector_steps=args.corrector_steps,
                                       corrector_snr=args.corrector_snr, resample_passes=args.resample_passes,
                                       jump_length=args.jump_length, eta=args.eta, multistep=args.multistep, contact_guidance=guide,
                                       xrd_guidance=xguide, **species_kw, **keywords))
    n_atoms = spec.n_atoms if spec is not None else args.num_atoms
    if start:
        if args.keyed:  # the key of a crystal: its index in the file
            start_crystals.crystal_keys = np.arange(len(np.asarray(start_crystals.num_atoms)), dtype=np.int64)
        res = generate_from_crystals(start_fn, start_crystals, args.batch, rank, world, unique=unique)
    elif condition is not None and args.keyed:
        # the key of tiled template j (order t0, t1, ..., t0, t1, ...): its index in the file times samples_per_template plus the copy
        from .diffusion.keyed import template_key
        n_file, K = condition.B // args.samples_per_template, args.samples_per_template
        mine = [fn(None, None, condition.slice(a, b), keys=[template_key(j, n_file, K) for j in range(a, b)])
                for a, b in template_batches(condition.B, args.batch, rank, world)]
        res = _gather_results(concat_results(mine), rank, world, None, unique)
    elif condition is not None:
        res = generate_from_template(lambda c: fn(None, None, c), condition, args.batch, rank, world, unique=unique)
    elif args.keyed:
        res = generate_keyed(lambda keys: fn(n_atoms, len(keys), keys=keys), slots, args.num_crystals, args.batch, rank, world,
                             require_valid=args.require_valid, max_rounds=args.max_rounds, unique=unique)
    elif args.require_valid:
        res = generate_valid_crystals(fn, args.num_crystals, n_atoms, args.batch, rank, world, max_rounds=args.max_rounds, unique=unique)
    else:
        res = generate_n_crystals(fn, args.num_crystals, n_atoms, args.batch, rank, world, unique=unique)
    from .diffusion import contact_guidance, xrd_guidance
    # every rank's batches summed, gathered like the results; rank 0 prints
    for guidance_mod, parts in ((contact_guidance, guide_parts if guide is not None else None), (xrd_guidance, xguide_parts if xguide is not None else None)):
        if parts is None:
            continue
        mine = guidance_mod.total_stats(parts, rank)
        ranks = [mine]
        if world > 1:
            ranks = [None] * world if rank == 0 else None
            dist.gather_object(mine, ranks, dst=0)
        if rank == 0:
            for line in guidance_mod.summary_lines(ranks):
                print(line)
    if rank == 0:
        special = {"unique": lambda parts: unique_lines(res, unique, device=f"cuda:{local_rank}"),
                   "find_symmetry": lambda parts: symmetry_lines(res, parts, spec)}
        for e in INSTRUMENTS:
            if asked[e.keyword] is not None:
                lines = special.get(e.keyword, lambda parts: instrument_lines(e.keyword, res, parts))
                for line in lines((res.info or {}).get(e.stats_key)):
                    print(line)
        print("wrote", save_sample_results(res, args.out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
