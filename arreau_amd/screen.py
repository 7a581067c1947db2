"""Screen an existing file of crystals on the GPU: generated crystals or a training set in the crystals.npz / .h5 layout.

    python -m arreau_amd.screen out/crystals.npz [--min_distance 0.5] [--min_volume 0.1] [--search_radius 3.0] [--out screened.npz]
    python -m arreau_amd.screen out/crystals.npz --find_symmetry [--symprec 0.1]
    python -m arreau_amd.screen out/crystals.npz --reduce_cell [--symprec 0.1] [--out reduced.npz]
    python -m arreau_amd.screen out/crystals.npz --symmetrize [--symprec 0.1] [--out symmetrized.npz]
    python -m arreau_amd.screen out/crystals.npz --unique [--against train.npz] [--fp_r_max 6] [--fp_sigma 0.1] [--fp_tolerance 0.01]

Prints the summary `python -m arreau_amd.generate --screen` prints (accepted / attempted and the count per flag) and, with
`--out`, writes the crystals again with the screen_* arrays (diffusion/inference/process_generated_crystals.py).  The species
check looks for the mask state's atomic number (2001).  The rules are in include/arreau_hip.h (arreau_crystal_screen).
`--unique` adds duplicate detection (diffusion/uniqueness.py): unique / attempted of the file, the unique_* arrays with `--out`,
and with `--against FILE` the novelty -- the share of crystals with no match in that other set.
`--find_symmetry [--symprec 0.1]` adds the symmetry search (diffusion/symmetry_search.py): the count per crystal system, point
group and flag, and the sym_* arrays with `--out`.  No space-group number, no standardised cell.
`--reduce_cell [--symprec 0.1]` adds the cell reduction (diffusion/cell_reduction.py): the count per multiplicity and flag; `--out`
then writes a crystals file of the REDUCED crystals (primitive, Delaunay-reduced cells; the screen_* / unique_* / sym_* arrays of
this run describe the cells as given and are not written to it), on which the other options can be run in turn.
`--symmetrize [--symprec 0.1]` adds the symmetrization (diffusion/symmetrize.py): the count per number of orbits and flag and the
largest displacement; `--out` then writes a crystals file of the SYMMETRIZED crystals (averaged positions, rebuilt cells, and the
symmetrized_* arrays) in the same way.  With `--reduce_cell` too the reduction runs first and its crystals are symmetrized.
"""
import argparse


def build_parser() -> argparse.ArgumentParser:
    from .generate import add_fingerprint_arguments, add_screen_arguments, add_symmetry_search_arguments
    ap = argparse.ArgumentParser(prog="python -m arreau_amd.screen", description="structural screen of a crystals file")
    ap.add_argument("file", type=str, help="crystals.npz / .h5")
    add_screen_arguments(ap)
    ap.add_argument("--out", type=str, default=None, help="write the crystals with their screen_* arrays to this file")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--unique", action="store_true", help="also detect duplicates within the file")
    ap.add_argument("--against", type=str, default=None, help="--unique: a second crystals file (e.g. the training set) for novelty")
    add_fingerprint_arguments(ap)
    ap.add_argument("--find_symmetry", action="store_true", help="also find every crystal's symmetry operations and point group")
    add_symmetry_search_arguments(ap)
    ap.add_argument("--reduce_cell", action="store_true",
                    help="also reduce every crystal to its primitive, Delaunay-reduced cell; --out then writes the reduced crystals")
    ap.add_argument("--symmetrize", action="store_true",
                    help="also symmetrize every crystal with the operations found within --symprec; --out then writes the "
                         "symmetrized crystals (after --reduce_cell: of the reduced crystals)")
    return ap


def main(argv=None):
    from .diffusion import screening
    from .diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from .generate import (cell_reduction_params, fingerprint_params, reduce_lines, screen_criteria, symmetrize_lines,
                           symmetrize_params, symmetry_lines, symmetry_search_params, unique_lines)
    ap = build_parser()
    args = ap.parse_args(argv)
    criteria = screen_criteria(args, ap.error)
    if args.against is not None and not args.unique:
        ap.error("--against needs --unique")
    unique = fingerprint_params(args, ap.error) if args.unique else None
    find_sym = symmetry_search_params(args, ap.error) if args.find_symmetry else None
    reduce_cell = cell_reduction_params(args, ap.error) if args.reduce_cell else None
    symmetrize = symmetrize_params(args, ap.error) if args.symmetrize else None

    def load(name):
        try:
            return load_sample_results_from_hdf5(name)
        except (OSError, KeyError) as e:
            ap.error(f"{name}: {e}")

    res = load(args.file)
    against = load(args.against) if args.against is not None else None
    res.metrics = screening.screen_sample_result(res, criteria, args.device)
    for line in screening.summary_lines([screening.stats_of(res.metrics["flags"])]):
        print(line)
    if unique is not None:
        res.info = None  # (no per-rank parts: the file is one set)
        for line in unique_lines(res, unique, against, args.device):
            print(line)
    if find_sym is not None:
        from .diffusion import symmetry_search
        res.symmetry = symmetry_search.symmetry_sample_result(res, find_sym, args.device)
        for line in symmetry_lines(res):
            print(line)
    if reduce_cell is not None:
        from .diffusion import cell_reduction
        from .diffusion.diffusion_loss import SampleResult
        res.reduced = cell_reduction.sample_arrays(cell_reduction.reduce_sample_result(res, reduce_cell, args.device))
        for line in reduce_lines(res):
            print(line)
        reduced = SampleResult(**cell_reduction.reduced_crystals(res.reduced), reduced=res.reduced)
        if symmetrize is not None:
            _symmetrize(reduced, symmetrize, args, symmetrize_lines, save_sample_results_to_hdf5)
        elif args.out:
            print("wrote", save_sample_results_to_hdf5(reduced, args.out))
        return res
    if symmetrize is not None:
        _symmetrize(res, symmetrize, args, symmetrize_lines, save_sample_results_to_hdf5)
        return res
    if args.out:
        print("wrote", save_sample_results_to_hdf5(res, args.out))
    return res


def _symmetrize(crystals, params, args, lines, save):
    """Symmetrize `crystals` (the file's, or its reduced ones), print the summary and, with --out, write the symmetrized crystals."""
    from .diffusion import symmetrize
    from .diffusion.diffusion_loss import SampleResult
    crystals.symmetrized = symmetrize.sample_arrays(symmetrize.symmetrize_sample_result(crystals, params, args.device))
    for line in lines(crystals):
        print(line)
    if args.out:
        arrays = symmetrize.symmetrized_crystals(crystals.symmetrized, crystals.atomic_numbers, crystals.num_atoms)
        print("wrote", save(SampleResult(**arrays, reduced=crystals.reduced, symmetrized=crystals.symmetrized), args.out))


if __name__ == "__main__":
    main()
