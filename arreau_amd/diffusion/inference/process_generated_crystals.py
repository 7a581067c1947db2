"""Result wire format of the sampler: the `crystals` group of out/crystals.h5
(diffusion/inference/process_generated_crystals.py:8-47 of the reference) -- writer, reader and the
per-crystal slicing helpers, so `main_diffusion_process_results.py`, the notebook viewer and the MACE
relaxation of the reference keep working on files written here.

Layout (main_diffusion_generate.py:67-92): frac_x [sum n, 3] float64, atomic_numbers [sum n] float64 (the
reference fills an `np.empty` float array), lattice [B, 3, 3] float64, idx_start [B] int64 (first atom of
each crystal), num_atoms [B] int64.  HDF5 when h5py is importable (it is not in this image); `.npz`
with the same five keys otherwise.

A result that carries the structural screen's metrics (SampleResult.metrics, diffusion/screening.py) gets seven more arrays,
one entry per crystal: screen_min_distance, screen_pair [B,5], screen_n_close, screen_volume, screen_number_density,
screen_flags, screen_valid.  Readers of the five keys above are not affected; a result without metrics is written with
exactly those five.  A result that carries duplicate detection's arrays (SampleResult.uniqueness, diffusion/uniqueness.py) gets
six more in the same way: unique_duplicate_of, unique_distance, unique_nearest, unique_nearest_distance, unique_flags,
unique_unique; without them none is written.  A result that carries the symmetry search's arrays (SampleResult.symmetry,
diffusion/symmetry_search.py) gets sym_n_lattice, sym_n_ops, sym_n_translations, sym_ops_rotation [B,max_ops], sym_ops_translation
[B,max_ops,3], sym_ops_residual [B,max_ops], sym_residual, sym_point_group, sym_flags and sym_symprec; a reader gets them back with
`lattice` filled in from the file's cells.  A result that carries the cell reduction's arrays (SampleResult.reduced,
diffusion/cell_reduction.py) gets reduced_multiplicity, reduced_n_translations, reduced_lattice [B,3,3], reduced_transform [B,3,3],
reduced_num_atoms, reduced_flags, reduced_selling_steps, reduced_symprec, and the reduced crystals' atoms reduced_frac_x [sum
reduced_num_atoms, 3], reduced_atomic_numbers and reduced_keep.  A result that carries the symmetrization's arrays
(SampleResult.symmetrized, diffusion/symmetrize.py) gets symmetrized_frac_x [sum n, 3], symmetrized_orbit, symmetrized_orbit_size and
symmetrized_site_order [sum n], and per crystal symmetrized_lattice [B,3,3], symmetrized_lengths, symmetrized_angles [B,3],
symmetrized_n_orbits, symmetrized_max_displacement, symmetrized_rms_displacement, symmetrized_ops_translation [B,max_ops,3] and
symmetrized_flags.  A result that carries a structure match against targets (SampleResult.match,
diffusion/structure_match.py) gets match_partner [sum n] and per crystal match_target, match_n_comparable, match_rms, match_rms_norm,
match_max_dist, match_mapping, match_translation [B,3], match_n_mappings, match_n_candidates, match_n_permutations, match_matched and
match_flags."""
import os

import numpy as np

from ..diffusion_loss import SampleResult

KEYS = ("frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms")
METRIC_KEYS = ("min_distance", "pair", "n_close", "volume", "number_density", "flags", "valid")
METRIC_PREFIX = "screen_"
UNIQUE_KEYS = ("duplicate_of", "distance", "nearest", "nearest_distance", "flags", "unique")
UNIQUE_PREFIX = "unique_"
SYM_KEYS = ("n_lattice", "n_ops", "n_translations", "ops_rotation", "ops_translation", "ops_residual", "residual", "point_group",
            "flags", "symprec")
SYM_PREFIX = "sym_"
REDUCED_KEYS = ("multiplicity", "n_translations", "lattice", "transform", "num_atoms", "flags", "selling_steps", "symprec", "frac_x",
                "atomic_numbers", "keep")  # cell_reduction.REDUCED_KEYS
REDUCED_PREFIX = "reduced_"
SYMMETRIZED_KEYS = ("frac_x", "lattice", "lengths", "angles", "orbit", "orbit_size", "site_order", "n_orbits", "max_displacement",
                    "rms_displacement", "ops_translation", "flags")  # symmetrize.SYMMETRIZED_KEYS
SYMMETRIZED_PREFIX = "symmetrized_"
MATCH_KEYS = ("target", "n_comparable", "rms", "rms_norm", "max_dist", "mapping", "translation", "partner", "n_mappings", "n_candidates",
              "n_permutations", "matched", "flags")  # structure_match.MATCH_KEYS
MATCH_PREFIX = "match_"
_DTYPES = dict(frac_x=np.float64, atomic_numbers=np.float64, lattice=np.float64, idx_start=np.int64,
               num_atoms=np.int64)


def _fields(crystals: SampleResult):
    out = {}
    for k in KEYS:
        v = getattr(crystals, k)
        if v is None:
            raise ValueError(f"SampleResult.{k} is missing")
        out[k] = np.asarray(v).astype(_DTYPES[k], copy=False)
    B = out["num_atoms"].shape[0]
    n_tot = int(out["num_atoms"].sum())
    if out["frac_x"].shape != (n_tot, 3) or out["atomic_numbers"].shape != (n_tot,) or \
            out["lattice"].shape != (B, 3, 3) or out["idx_start"].shape != (B,):
        raise ValueError("SampleResult arrays do not have the crystals.h5 layout")
    metrics = getattr(crystals, "metrics", None)
    if metrics is not None:
        for k in METRIC_KEYS:
            if k not in metrics:
                raise ValueError(f"SampleResult.metrics[{k!r}] is missing")
            v = np.asarray(metrics[k])
            if v.shape != ((B, 5) if k == "pair" else (B,)):
                raise ValueError(f"SampleResult.metrics[{k!r}] does not hold one entry per crystal")
            out[METRIC_PREFIX + k] = v
    uniqueness = getattr(crystals, "uniqueness", None)
    if uniqueness is not None:
        for k in UNIQUE_KEYS:
            if k not in uniqueness:
                raise ValueError(f"SampleResult.uniqueness[{k!r}] is missing")
            v = np.asarray(uniqueness[k])
            if v.shape != (B,):
                raise ValueError(f"SampleResult.uniqueness[{k!r}] does not hold one entry per crystal")
            out[UNIQUE_PREFIX + k] = v
    symmetry = getattr(crystals, "symmetry", None)
    if symmetry is not None:
        for k in SYM_KEYS:
            if k not in symmetry:
                raise ValueError(f"SampleResult.symmetry[{k!r}] is missing")
            v = np.asarray(symmetry[k])
            if v.shape[:1] != (B,) or v.ndim != {"ops_rotation": 2, "ops_translation": 3, "ops_residual": 2}.get(k, 1):
                raise ValueError(f"SampleResult.symmetry[{k!r}] does not hold one row per crystal")
            out[SYM_PREFIX + k] = v
    reduced = getattr(crystals, "reduced", None)
    if reduced is not None:
        n_red = int(np.asarray(reduced["num_atoms"]).sum()) if "num_atoms" in reduced else -1
        for k in REDUCED_KEYS:
            if k not in reduced:
                raise ValueError(f"SampleResult.reduced[{k!r}] is missing")
            v = np.asarray(reduced[k])
            if v.shape[:1] != ((n_red,) if k in ("frac_x", "atomic_numbers", "keep") else (B,)):
                raise ValueError(f"SampleResult.reduced[{k!r}] does not hold one row per crystal (or per reduced atom)")
            out[REDUCED_PREFIX + k] = v
    symmetrized = getattr(crystals, "symmetrized", None)
    if symmetrized is not None:
        for k in SYMMETRIZED_KEYS:
            if k not in symmetrized:
                raise ValueError(f"SampleResult.symmetrized[{k!r}] is missing")
            v = np.asarray(symmetrized[k])
            if v.shape[:1] != ((n_tot,) if k in ("frac_x", "orbit", "orbit_size", "site_order") else (B,)):
                raise ValueError(f"SampleResult.symmetrized[{k!r}] does not hold one row per crystal (or per atom)")
            out[SYMMETRIZED_PREFIX + k] = v
    match = getattr(crystals, "match", None)
    if match is not None:
        for k in MATCH_KEYS:
            if k not in match:
                raise ValueError(f"SampleResult.match[{k!r}] is missing")
            v = np.asarray(match[k])
            if v.shape[:1] != ((n_tot,) if k == "partner" else (B,)):
                raise ValueError(f"SampleResult.match[{k!r}] does not hold one row per crystal (or per atom)")
            out[MATCH_PREFIX + k] = v
    return out


def _metrics_from(has, get, prefix=METRIC_PREFIX, keys=METRIC_KEYS):
    """The metrics dict of a file's screen_* arrays (or the uniqueness dict of its unique_* arrays), or None when the file has none."""
    if not all(has(prefix + k) for k in keys):
        return None
    return {k: get(prefix + k) for k in keys}


def _is_h5(filename):
    return str(filename).endswith((".h5", ".hdf5"))


def save_sample_results_to_hdf5(crystals: SampleResult, filename: str):
    """process_generated_crystals.py:8-15.  `.h5`/`.hdf5` needs h5py (raises ImportError otherwise: the caller
    asked for HDF5 explicitly); any other name is written as `.npz` with the same keys."""
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    fields = _fields(crystals)
    if _is_h5(filename):
        import h5py
        with h5py.File(filename, "w") as fh:
            group = fh.create_group("crystals")
            for k, v in fields.items():
                group.create_dataset(k, data=v)
    else:
        np.savez(filename, **fields)
    return filename


def load_sample_results_from_hdf5(filename: str) -> SampleResult:
    """process_generated_crystals.py:18-30 (the path is taken as given, not relative to the package)."""
    if _is_h5(filename):
        import h5py
        with h5py.File(filename, "r") as fh:
            data = {k: fh["crystals"][k][:] for k in KEYS}
            metrics = _metrics_from(lambda k: k in fh["crystals"], lambda k: fh["crystals"][k][:])
            uniqueness = _metrics_from(lambda k: k in fh["crystals"], lambda k: fh["crystals"][k][:], UNIQUE_PREFIX, UNIQUE_KEYS)
            symmetry = _metrics_from(lambda k: k in fh["crystals"], lambda k: fh["crystals"][k][:], SYM_PREFIX, SYM_KEYS)
            reduced = _metrics_from(lambda k: k in fh["crystals"], lambda k: fh["crystals"][k][:], REDUCED_PREFIX, REDUCED_KEYS)
            symmetrized = _metrics_from(lambda k: k in fh["crystals"], lambda k: fh["crystals"][k][:], SYMMETRIZED_PREFIX, SYMMETRIZED_KEYS)
            match = _metrics_from(lambda k: k in fh["crystals"], lambda k: fh["crystals"][k][:], MATCH_PREFIX, MATCH_KEYS)
    else:
        with np.load(filename) as z:
            data = {k: z[k] for k in KEYS}
            metrics = _metrics_from(lambda k: k in z.files, lambda k: z[k])
            uniqueness = _metrics_from(lambda k: k in z.files, lambda k: z[k], UNIQUE_PREFIX, UNIQUE_KEYS)
            symmetry = _metrics_from(lambda k: k in z.files, lambda k: z[k], SYM_PREFIX, SYM_KEYS)
            reduced = _metrics_from(lambda k: k in z.files, lambda k: z[k], REDUCED_PREFIX, REDUCED_KEYS)
            symmetrized = _metrics_from(lambda k: k in z.files, lambda k: z[k], SYMMETRIZED_PREFIX, SYMMETRIZED_KEYS)
            match = _metrics_from(lambda k: k in z.files, lambda k: z[k], MATCH_PREFIX, MATCH_KEYS)
    if symmetry is not None:  # (the search saw the float32 cells)
        symmetry["lattice"] = np.asarray(data["lattice"], dtype=np.float32).reshape(-1, 3, 3)
    return SampleResult(**data, metrics=metrics, uniqueness=uniqueness, symmetry=symmetry, reduced=reduced,
                        symmetrized=symmetrized, match=match)


def get_crystal_indexes(sample_result: SampleResult, sample_idx: int):
    """process_generated_crystals.py:33-37."""
    crystal_start_idx = sample_result.idx_start[sample_idx]
    num_atoms = sample_result.num_atoms[sample_idx]
    return crystal_start_idx, crystal_start_idx + num_atoms


def get_one_crystal(sample_result: SampleResult, sample_idx: int):
    """process_generated_crystals.py:40-47: (lattice [3,3], frac_x [n,3], atomic_numbers [n])."""
    lattice = sample_result.lattice[sample_idx]
    start, end = get_crystal_indexes(sample_result, sample_idx)
    return lattice, sample_result.frac_x[start:end], sample_result.atomic_numbers[start:end]
