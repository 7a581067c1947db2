"""Result wire format of the sampler: the `crystals` group of out/crystals.h5
(diffusion/inference/process_generated_crystals.py:8-47 of the reference) -- writer, reader and the
per-crystal slicing helpers, so `main_diffusion_process_results.py`, the notebook viewer and the MACE
relaxation of the reference keep working on files written here.

Layout (main_diffusion_generate.py:67-92): frac_x [sum n, 3] float64, atomic_numbers [sum n] float64 (the
reference fills an `np.empty` float array), lattice [B, 3, 3] float64, idx_start [B] int64 (first atom of
each crystal), num_atoms [B] int64.  HDF5 when h5py is importable (it is not in this image); `.npz`
with the same five keys otherwise.

A result that carries an instrument's arrays (diffusion/instruments.py: SampleResult.metrics, .uniqueness, .symmetry, .reduced,
.symmetrized, .match, .conventional, .coordination, .bond_order, .voronoi, .xrd, .ewald) gets one more array per stored key, <prefix><key>: screen_*, unique_*, sym_*, reduced_*,
symmetrized_*, match_*, conventional_*, coord_*, order_*, voronoi_*, xrd_*, ewald_*, in that order, each instrument's keys in the order of its module's tuple (screening.STORED_KEYS, uniqueness.UNIQUE_KEYS,
symmetry_search.SYM_KEYS, cell_reduction.REDUCED_KEYS, symmetrize.SYMMETRIZED_KEYS, structure_match.MATCH_KEYS,
conventional_cell.CONVENTIONAL_KEYS, coordination.STORED_KEYS, bond_order.STORED_KEYS, voronoi.STORED_KEYS, xrd.STORED_KEYS, ewald.STORED_KEYS; the modules say what each holds).  One row per crystal, except the per-atom keys: of the
result's atoms [sum n] for symmetrized_*, match_*, coord_*, order_* and voronoi_*, of the reduced crystals' [sum reduced_num_atoms] for reduced_*, of the
conventional crystals' [sum conventional_num_atoms] for conventional_*.  Readers of the five keys above are not affected; a result without an
instrument's arrays is written without them, and a reader gets back None.  A reader gets the symmetry search's arrays back with
`lattice` filled in from the file's cells.

A keyed result (SampleResult.crystal_keys; diffusion/keyed.py) gets one more array, `crystal_keys` [B] int64, after all of those; a
result without keys is written exactly as before, and a reader of a file without the array gets back None."""
import os

import numpy as np

from ..diffusion_loss import SampleResult
from ..instruments import COMPLETE as INSTRUMENTS, file_fields

KEYS = ("frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms")
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
    for e in INSTRUMENTS:
        arrays = getattr(crystals, e.field, None)
        if arrays is not None:
            out.update(file_fields(e, arrays, B, n_tot))
    keys = getattr(crystals, "crystal_keys", None)
    if keys is not None:
        keys = np.asarray(keys).astype(np.int64, copy=False)
        if keys.shape != (B,):
            raise ValueError("SampleResult.crystal_keys must hold one key per crystal")
        out["crystal_keys"] = keys
    return out


def _read(has, get):
    """The SampleResult of a file's arrays: the five keys, and every instrument's dict (None when the file lacks one of its keys)."""
    data = {k: get(k) for k in KEYS}
    for e in INSTRUMENTS:
        data[e.field] = {k: get(e.prefix + k) for k in e.keys} if all(has(e.prefix + k) for k in e.keys) else None
    if data["symmetry"] is not None:  # (the search saw the float32 cells)
        data["symmetry"]["lattice"] = np.asarray(data["lattice"], dtype=np.float32).reshape(-1, 3, 3)
    if has("crystal_keys"):
        data["crystal_keys"] = np.asarray(get("crystal_keys"), dtype=np.int64)
    return SampleResult(**data)


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
            return _read(lambda k: k in fh["crystals"], lambda k: fh["crystals"][k][:])
    with np.load(filename) as z:
        return _read(lambda k: k in z.files, lambda k: z[k])


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
