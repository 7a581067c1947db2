"""Screen an existing file of crystals on the GPU: generated crystals or a training set in the crystals.npz / .h5 layout.

    python -m arreau_amd.screen out/crystals.npz [--min_distance 0.5] [--min_volume 0.1] [--search_radius 3.0] [--out screened.npz]
    python -m arreau_amd.screen out/crystals.npz --find_symmetry [--symprec 0.1]
    python -m arreau_amd.screen out/crystals.npz --reduce_cell [--symprec 0.1] [--out reduced.npz]
    python -m arreau_amd.screen out/crystals.npz --symmetrize [--symprec 0.1] [--out symmetrized.npz]
    python -m arreau_amd.screen out/crystals.npz --conventional_cell [--symprec 0.1] [--out conventional.npz]
    python -m arreau_amd.screen out/crystals.npz --match_to targets.npz [--match_mode paired|any] [--ltol 0.2] [--angle_tol 5] [--stol 0.3]
    python -m arreau_amd.screen out/crystals.npz --coordination [--cn_tol 0.1] [--cn_cutoff 6.0]
    python -m arreau_amd.screen out/crystals.npz --bond_order [--cn_tol 0.1] [--cn_cutoff 6.0]
    python -m arreau_amd.screen out/crystals.npz --voronoi [--vor_tol 0.05] [--vor_cutoff 6.0]
    python -m arreau_amd.screen out/crystals.npz --xrd [--xrd_wavelength 1.54184] [--xrd_fwhm 0.2] [--xrd_against targets.npz]
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
`--conventional_cell [--symprec 0.1]` adds the conventional cells (diffusion/conventional_cell.py: the reduction, the symmetry search
on the reduced cells, the conventional basis): the count per Bravais lattice and flag; `--out` then writes a crystals file of the
CONVENTIONAL crystals (with the conventional_* arrays alone: the other arrays of this run describe the crystals as given).  It reads the crystals as given; `--out` together with `--reduce_cell` or
`--symmetrize` is rejected: run them in turn, each on the file the one before wrote.  No space-group number, no idealised metric.
`--match_to TARGETS` adds the structure match (diffusion/structure_match.py) against the crystals of a second file: match rate, mean
rms_norm and rms over the matched, and the count per flag; `--match_mode paired` matches crystal b against target b, `any` against
every target of its composition (the best one counts); without the flag the match is paired when the two files hold equally many
crystals.  It runs after `--reduce_cell` and `--symmetrize` when those are given, on their crystals, and the targets are then put
through the same reduction and symmetrization; `--out` gets the match_* arrays.  The optimal assignment only with `--assignment optimal`, no supercells, no
volume scaling.
`--coordination [--cn_tol 0.1] [--cn_cutoff 6.0]` adds the coordination environments (diffusion/coordination.py: every atom's
neighbours within (1 + cn_tol) times its nearest distance and within cn_cutoff): the histogram of coordination numbers, the mean per
element, the share of bonds both ends agree on and the count per flag, and the coord_* arrays with `--out`.  It runs last, on the
crystals `--out` writes: the file's, or those of `--reduce_cell` / `--symmetrize` / `--conventional_cell --out`.  No Voronoi
weighting (not CrystalNN), no radii, no chemistry.
`--bond_order [--cn_tol 0.1] [--cn_cutoff 6.0]` adds the bond angles and Steinhardt order parameters of every atom's coordination
shell (diffusion/bond_order.py): the summed angle histogram, the mean q4 and q6 overall and per element and the count per flag, and
the order_* arrays with `--out`.  It runs last too, beside `--coordination`, on the same crystals.  No w_l, no neighbour-averaged
parameters, no classification of environments.
`--voronoi [--vor_tol 0.05] [--vor_cutoff 6.0]` adds every atom's Voronoi cell (diffusion/voronoi.py: the neighbours behind its faces,
each weighted by its solid angle over the atom's largest; a face counts at weight >= vor_tol): the histogram of cn, the mean cn and
cn_eff overall and per element, the share of atoms whose cell vor_cutoff does not close (OPEN) and the count per flag, and the
voronoi_* arrays with `--out`.  It runs last too, beside `--coordination` / `--bond_order`, on the same crystals.  Not CrystalNN: no
radii, no electronegativities, no distance weighting, no probabilities.
`--xrd [--xrd_wavelength --xrd_fwhm --xrd_two_theta_min --xrd_two_theta_max --xrd_points --xrd_b_iso --xrd_scattering]` adds every
crystal's powder X-ray diffraction pattern on a fixed 2 theta grid (diffusion/xrd.py): the count per flag, the mean number of lattice
points kept and the mean, minimum and maximum 2 theta of the strongest peak, and the xrd_* arrays with `--out`.  It runs last, on the
same crystals.  `--xrd_against TARGETS` gives every crystal of TARGETS a pattern under the same parameters: with as many targets as
crystals it prints the paired mean and median distance ((1 - cos) / 2 of the two patterns), otherwise each crystal's smallest distance to
any target.  Z-weighted point scatterers: no form-factor tables, no anomalous dispersion, no peak list, no K alpha 2.
`--ewald --ewald_charges Na=1,Cl=-1 [--ewald_accuracy 1e-8] [--ewald_alpha A]` adds every crystal's Ewald electrostatic energy of
those point charges and every atom's site potential (diffusion/ewald.py): the count per flag, the mean, minimum and maximum energy
per atom in eV, the share of crystals that are not neutral (CHARGED), the mean |potential| per element, and the ewald_* arrays with
`--out`.  It runs last, on the same crystals.  No forces, no short-range repulsion (the energy alone favours collapse), no
oxidation-state guessing: an element without a charge flags its crystals UNASSIGNED.
"""
import argparse


def build_parser() -> argparse.ArgumentParser:
    from .generate import (add_coordination_arguments, add_ewald_arguments, add_fingerprint_arguments, add_voronoi_arguments, add_xrd_arguments, add_screen_arguments,
                           add_structure_match_arguments, add_symmetry_search_arguments)
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
    ap.add_argument("--conventional_cell", action="store_true",
                    help="also give every crystal its conventional cell, centring and Bravais lattice; --out then writes the "
                         "conventional crystals (not together with --reduce_cell or --symmetrize: run them in turn)")
    ap.add_argument("--match_to", type=str, default=None, metavar="TARGETS",
                    help="also match every crystal against the crystals of this file (after --reduce_cell / --symmetrize, which the "
                         "targets then go through too): match rate and mean RMSD")
    ap.add_argument("--match_mode", choices=("paired", "any"), default=None,
                    help="--match_to: crystal b against target b, or against every target of its composition (default: paired when "
                         "the files hold equally many crystals)")
    add_structure_match_arguments(ap)
    ap.add_argument("--coordination", action="store_true",
                    help="also find every atom's neighbours and coordination number (last: on the crystals --out writes)")
    ap.add_argument("--bond_order", action="store_true",
                    help="also find every atom's bond-angle histogram and Steinhardt order parameters (last: on the crystals --out writes)")
    add_coordination_arguments(ap)
    ap.add_argument("--voronoi", action="store_true",
                    help="also build every atom's Voronoi cell: solid-angle-weighted neighbours and atom volumes (last: on the crystals --out writes)")
    add_voronoi_arguments(ap)
    ap.add_argument("--xrd", action="store_true",
                    help="also write every crystal's powder X-ray diffraction pattern on a fixed 2 theta grid (last: on the crystals --out writes)")
    ap.add_argument("--xrd_against", type=str, default=None,
                    help="with --xrd: a crystals file whose patterns (same parameters) the crystals' are compared with: paired mean and "
                         "median distance with as many targets as crystals, else each crystal's smallest distance to any target")
    add_xrd_arguments(ap)
    ap.add_argument("--ewald", action="store_true",
                    help="also write every crystal's Ewald energy and every atom's site potential for the point charges of --ewald_charges "
                         "(last: on the crystals --out writes)")
    add_ewald_arguments(ap)
    return ap


def main(argv=None):
    from .diffusion import cell_reduction, screening, structure_match, symmetry_search
    from .diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from .diffusion.diffusion_loss import SampleResult
    from .diffusion.instruments import COMPLETE as INSTRUMENTS
    from .generate import check_ewald_arguments, instrument_lines, instrument_params, unique_lines
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.against is not None and not args.unique:
        ap.error("--against needs --unique")
    if args.match_mode is not None and args.match_to is None:
        ap.error("--match_mode needs --match_to")
    if args.xrd_against is not None and not args.xrd:
        ap.error("--xrd_against needs --xrd")
    if args.conventional_cell and args.out and (args.reduce_cell or args.symmetrize):
        ap.error("--conventional_cell with --out writes the conventional crystals and --reduce_cell / --symmetrize theirs: run them in "
                 "turn, each on the file the one before wrote")
    asked = {e.keyword: instrument_params(e.keyword, args, ap.error) if getattr(args, e.keyword, True) else None
             for e in INSTRUMENTS}  # (by sample() keyword; None: not asked for.  The screen has no flag here: it always runs)
    check_ewald_arguments(asked, ap.error)

    def load(name):
        try:
            return load_sample_results_from_hdf5(name)
        except (OSError, KeyError) as e:
            ap.error(f"{name}: {e}")

    def report(keyword, crystals):
        for line in instrument_lines(keyword, crystals):
            print(line)

    res = load(args.file)
    against = load(args.against) if args.against is not None else None
    targets = load(args.match_to) if args.match_to is not None else None
    xrd_targets = load(args.xrd_against) if args.xrd_against is not None else None
    res.metrics = screening.screen_sample_result(res, asked["screen"], args.device)
    report("screen", res)
    if asked["unique"] is not None:
        res.info = None  # (no per-rank parts: the file is one set)
        for line in unique_lines(res, asked["unique"], against, args.device):
            print(line)
    if asked["find_symmetry"] is not None:
        res.symmetry = symmetry_search.symmetry_sample_result(res, asked["find_symmetry"], args.device)
        report("find_symmetry", res)
    current = res  # the crystals the next step reads and --out writes: the file's, its reduced ones, their symmetrized ones
    if asked["reduce_cell"] is not None:
        reduce = lambda crystals: cell_reduction.sample_arrays(cell_reduction.reduce_sample_result(crystals, asked["reduce_cell"], args.device))
        res.reduced = reduce(res)
        report("reduce_cell", res)
        current = SampleResult(**cell_reduction.reduced_crystals(res.reduced), reduced=res.reduced)
        if targets is not None:
            targets = SampleResult(**cell_reduction.reduced_crystals(reduce(targets)))
    if asked["symmetrize"] is not None:
        current = _symmetrize(current, asked["symmetrize"], args)
        report("symmetrize", current)
        if targets is not None:
            targets = _symmetrize(targets, asked["symmetrize"], args)
    if targets is not None:
        try:
            matched = structure_match.match_crystals(current, targets, asked["match_to"], args.match_mode, args.device)
        except ValueError as e:
            ap.error(f"--match_to: {e}")
        current.match = res.match = structure_match.sample_arrays(matched)
        report("match_to", current)
    if asked["conventional_cell"] is not None:  # (of the crystals as given: the chain reduces them itself)
        from .diffusion import conventional_cell
        res.conventional = conventional_cell.sample_arrays(conventional_cell.conventional_sample_result(res, asked["conventional_cell"], args.device))
        report("conventional_cell", res)
        if args.out:
            current = SampleResult(**conventional_cell.conventional_crystals(res.conventional), conventional=res.conventional)
    if asked["coordination"] is not None:  # (of the crystals --out writes)
        from .diffusion import coordination
        current.coordination = coordination.coordination_sample_result(current, asked["coordination"], args.device)
        report("coordination", current)
    if asked["bond_order"] is not None:  # (of the same crystals)
        from .diffusion import bond_order
        current.bond_order = bond_order.bond_order_sample_result(current, asked["bond_order"], args.device)
        report("bond_order", current)
    if asked["voronoi"] is not None:  # (of the same crystals)
        from .diffusion import voronoi
        current.voronoi = voronoi.voronoi_sample_result(current, asked["voronoi"], args.device)
        report("voronoi", current)
    if asked["xrd"] is not None:  # (of the same crystals)
        from .diffusion import xrd
        current.xrd = xrd.xrd_sample_result(current, asked["xrd"], args.device)
        report("xrd", current)
        if xrd_targets is not None:
            for line in xrd.against_lines(current.xrd["pattern"], xrd.xrd_sample_result(xrd_targets, asked["xrd"], args.device)["pattern"]):
                print(line)
    if asked["ewald"] is not None:  # (of the same crystals)
        from .diffusion import ewald
        current.ewald = ewald.ewald_sample_result(current, asked["ewald"], args.device)
        report("ewald", current)
    if args.out:
        print("wrote", save_sample_results_to_hdf5(current, args.out))
    return res


def _symmetrize(crystals, params, args):
    """Symmetrize `crystals` (the file's, its reduced ones, or the targets of a match; they get the arrays too) and return the
    symmetrized crystals as the SampleResult that --out writes."""
    from .diffusion import symmetrize
    from .diffusion.diffusion_loss import SampleResult
    crystals.symmetrized = symmetrize.sample_arrays(symmetrize.symmetrize_sample_result(crystals, params, args.device))
    arrays = symmetrize.symmetrized_crystals(crystals.symmetrized, crystals.atomic_numbers, crystals.num_atoms)
    return SampleResult(**arrays, reduced=crystals.reduced, symmetrized=crystals.symmetrized)


if __name__ == "__main__":
    main()
