"""The per-crystal instruments that run on the final sampled state -- screen, duplicate detection, symmetry search, cell reduction,
symmetrization, structure match -- as one table, in the order their arrays appear in a crystals file, after them the DERIVED
ones, which chain those launches (the conventional cell: reduction, search on the reduced cell, conventional basis), and last the
LOCAL ones, which describe each atom's surroundings (the coordination environments); EVERY is all of them.  SHELL holds what
is built on a LOCAL one's neighbour lists (the bond angles and order parameters); TABLE is EVERY and SHELL, the whole table, and
KEYWORDS maps a sample() keyword to its entry.  CELLS holds what builds each atom's Voronoi cell (its own launch, after the
bond order); WHOLE is TABLE and CELLS -- what the file layer, the batch driver, the screen and sample() loop over -- and
WHOLE_KEYWORDS its keyword map.  PATTERNS holds what walks reciprocal space (the powder diffraction pattern: its own launch,
after the cells); FULL is WHOLE and PATTERNS, and FULL_KEYWORDS its keyword map.  ENERGIES holds what needs the user's charges
besides the geometry (the Ewald sum: its own launch, after the pattern); COMPLETE is FULL and ENERGIES -- what those four loop
over now -- and COMPLETE_KEYWORDS its keyword map.  An entry holds what the
instruments differ in for the host-side plumbing: the file layer (inference/process_generated_crystals.py), the batch driver
(generate.py) and `python -m arreau_amd.screen` loop over it, and so does DiffusionLoss.sample, which calls every asked-for
entry's `run` on the final device state (DeviceState) in table order: an entry that shares a launch comes after the entry that
makes it.  The stored keys are the owning modules' own tuples.  Needs numpy alone at import, as the modules do."""
from dataclasses import dataclass, field
from types import ModuleType
from typing import Callable, Optional

import numpy as np

from . import (bond_order, cell_reduction, conventional_cell, coordination, ewald, screening, structure_match, symmetrize,
               symmetry_search, uniqueness, voronoi, xrd)
from .tools.atomic_number_table import atomic_number_indexes_to_atomic_numbers


@dataclass
class DeviceState:
    """What an entry's `run` reads: the final state of a sample() call where it lies on the device, and `launched`, the device
    results of this run's launches that a later entry shares (keyed by the keyword of the entry that made them)."""
    eng: object
    frac: object          # [N,3] f32
    lattice: object       # [B,3,3] f32
    offsets: object       # [B+1] i32
    types: object         # [N] i32 class indices
    z_table: object
    num_atoms: np.ndarray
    atomic_numbers: np.ndarray  # of `types`
    mask_type: int        # what the screen takes for the mask state: S - 1, or -1 when the species were held constant
    launched: dict = field(default_factory=dict)

    @property
    def batch(self):
        return self.frac, self.lattice, self.offsets, self.types


def _run_screen(s, params):
    return screening.metrics_to_numpy(s.eng.screen(*s.batch, params.with_mask_type(s.mask_type)))


def _run_unique(s, params):
    return uniqueness.uniqueness_to_numpy(uniqueness.unique_batch(*s.batch, params))


def _run_find_symmetry(s, params):
    s.launched["find_symmetry"] = s.eng.find_symmetry(*s.batch, params)
    return symmetry_search.result_to_numpy(s.launched["find_symmetry"])


def _run_reduce_cell(s, params):
    s.launched["reduce_cell"] = s.eng.reduce_cells(*s.batch, params)
    reduced = cell_reduction.result_to_numpy(s.launched["reduce_cell"])
    return cell_reduction.sample_arrays(reduced, atomic_number_indexes_to_atomic_numbers(s.z_table, reduced["types"]))


def _run_symmetrize(s, params):  # (the search's launch is shared)
    return symmetrize.sample_arrays(symmetrize.result_to_numpy(s.eng.symmetrize(*s.batch, params, s.launched.get("find_symmetry"))))


def _run_match(s, params):  # (the atomic numbers are the species ids the targets carry: one small upload)
    import torch
    species = np.rint(np.asarray(s.atomic_numbers).reshape(-1)).astype(np.int32)
    return structure_match.sample_arrays(structure_match.match_batches(
        (s.frac, s.lattice, s.offsets, torch.as_tensor(species, device=s.frac.device)), s.num_atoms, species, *params))


def _run_conventional_cell(s, params):  # (the reduction's launch is shared)
    found = conventional_cell.result_to_numpy(s.eng.conventional_cell(*s.batch, params, s.launched.get("reduce_cell")))
    return conventional_cell.sample_arrays(found, atomic_number_indexes_to_atomic_numbers(s.z_table, found["types"]))


def _run_coordination(s, params):
    s.launched["coordination"] = s.eng.coordination(s.frac, s.lattice, s.offsets, params)
    return coordination.sample_arrays(coordination.result_to_numpy(s.launched["coordination"]), s.atomic_numbers)


def _run_bond_order(s, params):  # (the coordination launch is shared)
    return bond_order.sample_arrays(bond_order.result_to_numpy(
        s.eng.bond_order(s.frac, s.lattice, s.offsets, params, s.launched.get("coordination"))), s.atomic_numbers)


def _run_voronoi(s, params):
    s.launched["voronoi"] = s.eng.voronoi(s.frac, s.lattice, s.offsets, params)
    return voronoi.sample_arrays(voronoi.result_to_numpy(s.launched["voronoi"]), s.atomic_numbers)


def _run_xrd(s, params):  # (the atomic numbers are the amplitudes: one small upload)
    import torch
    weights = torch.as_tensor(xrd.host_weights(s.atomic_numbers, params), device=s.frac.device)
    return xrd.sample_arrays(xrd.result_to_numpy(s.eng.xrd(s.frac, s.lattice, s.offsets, weights, xrd.for_weights(params))), params)


def _run_ewald(s, params):  # (the charges of the atomic numbers: one small upload)
    import torch
    charges = ewald.host_charges(s.atomic_numbers, params)
    found = ewald.result_to_numpy(s.eng.ewald(s.frac, s.lattice, s.offsets, torch.as_tensor(charges, device=s.frac.device), params))
    return ewald.sample_arrays(found, charges, s.atomic_numbers, s.num_atoms)


@dataclass(frozen=True)
class Instrument:
    keyword: str       # sample(<keyword>=...), and the command-line flag of that name
    field: str         # SampleResult.<field>: the dict of its arrays
    prefix: str        # its arrays in a crystals file: <prefix><key>
    stats_key: str     # SampleResult.info[<stats_key>]: one statistics dict per rank
    module: ModuleType  # the owner: stats_of, summary_lines, the parameter class
    keys: tuple        # the stored keys, in file order
    params: str        # the module's parameter class ...
    flags: tuple       # ... and its (field, command-line flag) pairs
    label: str         # what a bad flag value is reported under
    atom_keys: tuple = ()  # the keys with one row per atom (the others: one row per crystal) ...
    atoms_from: Optional[str] = None  # ... of the result's crystals, or of the instrument's own crystals with these atom counts
    shape: object = None  # beyond the leading dimension: a trailing shape (exact), an ndim, or None for no requirement ...
    shapes: tuple = ()    # ... and the (key, requirement) pairs that differ from it
    carried: bool = True  # concat_results / select_crystals carry it (uniqueness indexes into the whole set: they do not)
    stats_from: Optional[str] = None  # stats_of reads this one array (None: the dict)
    run: Optional[Callable] = None    # run(DeviceState, resolved parameters) -> the dict of SampleResult.<field>: sample()'s launch

    def stats_of(self, arrays, rank=0):
        return self.module.stats_of(arrays if self.stats_from is None else arrays[self.stats_from], rank)


_SYMPREC = (("symprec", "symprec"),)
INSTRUMENTS = (
    Instrument("screen", "metrics", "screen_", "screen_stats", screening, screening.STORED_KEYS, "ScreenCriteria",
               (("min_distance", "min_distance"), ("min_volume", "min_volume"), ("search_radius", "search_radius")), "screen criteria",
               shape=(), shapes=(("pair", (5,)),), stats_from="flags", run=_run_screen),
    Instrument("unique", "uniqueness", "unique_", "unique_stats", uniqueness, uniqueness.UNIQUE_KEYS, "FingerprintParams",
               (("r_max", "fp_r_max"), ("sigma", "fp_sigma"), ("tolerance", "fp_tolerance")), "fingerprint parameters",
               shape=(), carried=False, run=_run_unique),
    Instrument("find_symmetry", "symmetry", "sym_", "symmetry_stats", symmetry_search, symmetry_search.SYM_KEYS, "SymmetrySearchParams",
               _SYMPREC, "symmetry search", shape=1, shapes=(("ops_rotation", 2), ("ops_translation", 3), ("ops_residual", 2)), run=_run_find_symmetry),
    Instrument("reduce_cell", "reduced", "reduced_", "reduce_stats", cell_reduction, cell_reduction.REDUCED_KEYS, "CellReductionParams",
               _SYMPREC, "cell reduction", atom_keys=cell_reduction.PER_ATOM_KEYS, atoms_from="num_atoms", run=_run_reduce_cell),
    Instrument("symmetrize", "symmetrized", "symmetrized_", "symmetrize_stats", symmetrize, symmetrize.SYMMETRIZED_KEYS,
               "SymmetrizeParams", _SYMPREC, "symmetrize", atom_keys=symmetrize.ATOM_KEYS, run=_run_symmetrize),
    Instrument("match_to", "match", "match_", "match_stats", structure_match, structure_match.MATCH_KEYS, "StructureMatchParams",
               (("ltol", "ltol"), ("angle_tol", "angle_tol"), ("stol", "stol"), ("assignment", "assignment")), "structure match", atom_keys=structure_match.ATOM_KEYS, run=_run_match),
)
# what is built on the six above: in a crystals file, in the summaries and on the command lines after them
DERIVED = (
    Instrument("conventional_cell", "conventional", "conventional_", "conventional_stats", conventional_cell,
               conventional_cell.CONVENTIONAL_KEYS, "ConventionalCellParams", _SYMPREC, "conventional cell",
               atom_keys=conventional_cell.ATOM_KEYS, atoms_from="num_atoms", run=_run_conventional_cell),
)
ALL = INSTRUMENTS + DERIVED
# what looks at each atom's surroundings, not at the crystal as a whole: after every other instrument's arrays
LOCAL = (
    Instrument("coordination", "coordination", "coord_", "coordination_stats", coordination, coordination.STORED_KEYS,
               "CoordinationParams", (("tol", "cn_tol"), ("cutoff", "cn_cutoff")), "coordination", atom_keys=coordination.ATOM_KEYS,
               shape=(), shapes=(("neighbors", 3),), run=_run_coordination),
)
EVERY = ALL + LOCAL
BY_KEYWORD = {e.keyword: e for e in EVERY}
# what chains on the coordination launch and reads its neighbour lists: after the coordination arrays
SHELL = (
    Instrument("bond_order", "bond_order", "order_", "bond_order_stats", bond_order, bond_order.STORED_KEYS, "BondOrderParams",
               (("tol", "cn_tol"), ("cutoff", "cn_cutoff")), "bond order", atom_keys=bond_order.ATOM_KEYS, shape=(),
               shapes=(("q", (len(bond_order.L_VALUES),)), ("q2", (len(bond_order.L_VALUES),)), ("mean_q", (len(bond_order.L_VALUES),)),
                       ("angles", (bond_order.ANGLE_BINS,)), ("angle_hist", (bond_order.ANGLE_BINS,))), run=_run_bond_order),
)
TABLE = EVERY + SHELL  # the whole table: what the file layer, the batch driver and the screen loop over
KEYWORDS = {e.keyword: e for e in TABLE}
# what builds each atom's Voronoi cell: a launch of its own, after the bond order; its arrays after order_*
CELLS = (
    Instrument("voronoi", "voronoi", "voronoi_", "voronoi_stats", voronoi, voronoi.STORED_KEYS, "VoronoiParams",
               (("tol", "vor_tol"), ("cutoff", "vor_cutoff")), "voronoi", atom_keys=voronoi.ATOM_KEYS, shape=(),
               shapes=(("neighbors", 3),) + tuple((k, 2) for k in voronoi.FACE_KEYS), run=_run_voronoi),
)
WHOLE = TABLE + CELLS  # the whole table with the cells: what the file layer, the batch driver, the screen and sample() loop over
WHOLE_KEYWORDS = {e.keyword: e for e in WHOLE}
# what walks reciprocal space: a launch of its own, after the cells; its arrays after voronoi_*
PATTERNS = (
    Instrument("xrd", "xrd", "xrd_", "xrd_stats", xrd, xrd.STORED_KEYS, "XrdParams",
               (("wavelength", "xrd_wavelength"), ("fwhm", "xrd_fwhm"), ("two_theta_min", "xrd_two_theta_min"),
                ("two_theta_max", "xrd_two_theta_max"), ("n_points", "xrd_points"), ("b_iso", "xrd_b_iso"),
                ("scattering", "xrd_scattering")), "xrd", shape=(), shapes=(("pattern", 2), ("grid", (len(xrd.GRID_KEYS),))), run=_run_xrd),
)
FULL = WHOLE + PATTERNS  # every instrument that reads geometry alone
FULL_KEYWORDS = {e.keyword: e for e in FULL}
# what needs more than the geometry -- the user's charges: a launch of its own, after the pattern; its arrays after xrd_*
ENERGIES = (
    Instrument("ewald", "ewald", "ewald_", "ewald_stats", ewald, ewald.STORED_KEYS, "EwaldParams",
               (("charges", "ewald_charges"), ("accuracy", "ewald_accuracy"), ("alpha", "ewald_alpha")), "ewald",
               atom_keys=ewald.ATOM_KEYS, shape=(), run=_run_ewald),
)
COMPLETE = FULL + ENERGIES  # every instrument: what the file layer, the batch driver, the screen and sample() loop over
COMPLETE_KEYWORDS = {e.keyword: e for e in COMPLETE}


def concat(entry, parts):
    """The arrays of `parts` (one dict per piece, in crystal order) as one dict; None when a piece has none or the entry is not
    carried.  Pieces of one run share their row widths (one max_ops)."""
    if not entry.carried or not parts or any(p is None for p in parts):
        return None
    return {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in parts[0]}


def select(entry, arrays, keep, atoms):
    """The rows of the crystals `keep` of an entry's dict, and of their atoms: `atoms` for the result's own (both a mask or
    indices), worked out here from the dict's own atom counts where the entry has its own crystals.  None as in `concat`."""
    if not entry.carried or arrays is None:
        return None
    if entry.atoms_from is not None:
        first = np.concatenate([[0], np.cumsum(np.asarray(arrays[entry.atoms_from], dtype=np.int64))])
        crystals = np.arange(len(first) - 1)[np.asarray(keep)]
        atoms = np.concatenate([np.arange(first[b], first[b + 1]) for b in crystals] + [np.empty(0, dtype=np.int64)]).astype(np.int64)
    return {k: np.asarray(v)[atoms if k in entry.atom_keys else keep] for k, v in arrays.items()}


def file_fields(entry, arrays, B, n_atoms):
    """{<prefix><key>: array} of an entry's dict for a file of B crystals with n_atoms atoms; a ValueError names the key that is
    missing or does not have its rows (one per crystal, or per atom) and its shape."""
    if entry.atoms_from is not None:
        n_atoms = int(np.asarray(arrays[entry.atoms_from]).sum()) if entry.atoms_from in arrays else -1
    rules, out = dict(entry.shapes), {}
    for k in entry.keys:
        if k not in arrays:
            raise ValueError(f"SampleResult.{entry.field}[{k!r}] is missing")
        v, rule = np.asarray(arrays[k]), rules.get(k, entry.shape)
        fits = v.shape[1:] == rule if isinstance(rule, tuple) else rule is None or v.ndim == rule
        if v.shape[:1] != ((n_atoms if k in entry.atom_keys else B),) or not fits:
            raise ValueError(f"SampleResult.{entry.field}[{k!r}] does not hold one entry per crystal"
                             + (" (or per atom)" if entry.atom_keys else ""))
        out[entry.prefix + k] = v
    return out


def summary_lines(entry, arrays, parts=None):
    """The lines an instrument's flag prints: one per rank (`parts`: the statistics the ranks carried; none: `arrays` as one set)
    and the total."""
    return entry.module.summary_lines(parts if parts else [entry.stats_of(arrays)] if arrays is not None else [])
