"""Screen an existing file of crystals on the GPU: generated crystals or a training set in the crystals.npz / .h5 layout.

    python -m arreau_amd.screen out/crystals.npz [--min_distance 0.5] [--min_volume 0.1] [--search_radius 3.0] [--out screened.npz]

Prints the summary `python -m arreau_amd.generate --screen` prints (accepted / attempted and the count per flag) and, with
`--out`, writes the crystals again with the screen_* arrays (diffusion/inference/process_generated_crystals.py).  The species
check looks for the mask state's atomic number (2001).  The rules are in include/arreau_hip.h (arreau_crystal_screen).
"""
import argparse


def build_parser() -> argparse.ArgumentParser:
    from .generate import add_screen_arguments
    ap = argparse.ArgumentParser(prog="python -m arreau_amd.screen", description="structural screen of a crystals file")
    ap.add_argument("file", type=str, help="crystals.npz / .h5")
    add_screen_arguments(ap)
    ap.add_argument("--out", type=str, default=None, help="write the crystals with their screen_* arrays to this file")
    ap.add_argument("--device", type=str, default="cuda")
    return ap


def main(argv=None):
    from .diffusion import screening
    from .diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from .generate import screen_criteria
    ap = build_parser()
    args = ap.parse_args(argv)
    criteria = screen_criteria(args, ap.error)
    try:
        res = load_sample_results_from_hdf5(args.file)
    except (OSError, KeyError) as e:
        ap.error(f"{args.file}: {e}")
    res.metrics = screening.screen_sample_result(res, criteria, args.device)
    for line in screening.summary_lines([screening.stats_of(res.metrics["flags"])]):
        print(line)
    if args.out:
        print("wrote", save_sample_results_to_hdf5(res, args.out))
    return res


if __name__ == "__main__":
    main()
