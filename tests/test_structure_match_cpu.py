"""The structure match without a GPU: the float64 restatement of rules 1-7 (diffusion/structure_match.py) on the pairs of
tests/structure_match_cases.py -- the analytic rms of displaced copies, invariance under the six transformations, the symmetry of
the match in x and y, the flags and the guards --, then parameter validation, the pairing helpers, the per-crystal reduction, the
statistics lines and the header."""
import math
import os

import numpy as np
import pytest

from arreau_amd.diffusion import instruments
from arreau_amd.diffusion import structure_match as sm
from arreau_amd.diffusion.diffusion_loss import SampleResult
from tests import structure_match_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = list(enumerate(cases.pairs()))
ids = lambda kp: kp[1].name


def test_every_case_is_guarded_and_flagged_as_expected():
    ref = cases.reference()  # (asserts the guard of every pair; no pair is exempt)
    cases.overflow_reference()
    for k, pair in PAIRS:
        assert int(ref.flags[k]) == pair.flags, (pair.name, sm.describe(ref.flags[k]))
        if pair.n_mappings is not None:
            assert int(ref.n_mappings[k]) == pair.n_mappings, pair.name
        if pair.flags & sm.NO_RESULT_MASK:
            assert np.isinf(ref.rms[k]) and np.isinf(ref.rms_norm[k]) and np.isinf(ref.max_dist[k]) and ref.mapping[k] == -1, pair.name
            assert ref.matched[k] == 0 and (ref.partner[k] == -1).all() and not ref.translation[k].any(), pair.name
    names = [p.name for _, p in PAIRS]
    assert len(set(names)) == len(names) and sum(p.x == 0 for _, p in PAIRS) >= 12  # the base crystal sits in many pairs


@pytest.mark.parametrize("kp", [kp for kp in PAIRS if kp[1].exact], ids=ids)
def test_a_transformed_copy_matches_with_rms_zero(kp):
    k, pair = kp
    ref = cases.reference()
    tol = cases.input_rounding(pair)
    print(f"{pair.name}: rms {ref.rms[k]:.3e} A, max {ref.max_dist[k]:.3e} A (the inputs' float32 rounding: {tol:.3e})")
    assert ref.flags[k] == 0 and ref.matched[k] == 1 and ref.n_permutations[k] >= 1
    assert ref.rms[k] <= tol and ref.max_dist[k] <= tol
    x, y = cases.crystals()[pair.x], cases.crystals()[pair.y]
    part = ref.partner[k, :x.n]
    assert sorted(part.tolist()) == list(range(x.n)) and np.array_equal(y.types[part], x.types)
    if pair.name == "P1: atoms permuted":
        assert np.array_equal(y.frac[part], x.frac)


@pytest.mark.parametrize("kp", [kp for kp in PAIRS if kp[1].rms is not None], ids=ids)
def test_displaced_copies_have_the_analytic_rms(kp):
    """sqrt(mean |u|^2), written out where the case is built: zero-mean displacements leave the least-squares translation at 0."""
    k, pair = kp
    ref = cases.reference()
    print(f"{pair.name}: rms {ref.rms[k]:.9f} A, analytic {pair.rms:.9f} A")
    assert abs(ref.rms[k] - pair.rms) <= cases.input_rounding(pair)
    n = cases.crystals()[pair.x].n
    L = cases.crystals()[pair.x].lattice.astype(np.float64)
    ell = (abs(np.linalg.det(L)) / n) ** (1.0 / 3.0)
    assert abs(ref.rms_norm[k] - pair.rms / ell) <= cases.input_rounding(pair) and np.abs(ref.translation[k] - np.rint(ref.translation[k])).max() < 1e-6


def test_matched_follows_stol():
    ref, stol = cases.reference(), cases.PARAMS.stol
    small, large = cases.pair_index("P1: displaced 0.03 A (matched)"), cases.pair_index("P1: displaced 0.25 A (a permutation, not matched)")
    assert ref.rms_norm[small] <= stol / 2 and ref.matched[small] == 1
    assert ref.rms_norm[large] >= 2 * stol and ref.matched[large] == 0 and ref.n_permutations[large] >= 1 and ref.flags[large] == 0


def test_the_match_is_symmetric_in_x_and_y():
    ref = cases.reference()
    swapped = np.array([[p.y, p.x] for _, p in PAIRS if not p.flags], dtype=np.int32)
    back = sm.structure_match_reference_f64(cases.batch(), cases.batch(), swapped, cases.PARAMS)
    for at, (k, pair) in enumerate((k, p) for k, p in PAIRS if not p.flags):
        n = cases.crystals()[pair.x].n
        bound = cases.bounds(ref, k, n)
        assert back.flags[at] == 0 and back.n_mappings[at] == ref.n_mappings[k], pair.name
        assert abs(back.rms[at] - ref.rms[k]) <= bound["rms"] and abs(back.rms_norm[at] - ref.rms_norm[k]) <= bound["rms_norm"], pair.name
        if pair.decisive:  # one surviving candidate: the maps are inverse to each other
            fwd, inv = ref.partner[k, :n], back.partner[at, :n]
            assert np.array_equal(inv[fwd], np.arange(n)), pair.name


def test_overflow_uses_the_first_mappings():
    ref, full = cases.overflow_reference(), cases.reference()
    k = cases.pair_index("rock salt against a perturbed copy")
    assert ref.flags[0] == sm.OVERFLOW and ref.n_mappings[0] == 48 and ref.n_candidates[0] == 2 * 4 and full.n_candidates[k] == 48 * 4
    assert ref.rms[0] >= full.rms[k] - 1e-12 and np.isfinite(ref.rms[0])


def test_bounds_come_from_the_rules_and_the_cell():
    assert sm.translation_bound(7, 0.0) == 64 * sm.U and sm.difference_bound(7, 0.0) == 88 * sm.U
    assert sm.distance_bound(7, 8.0, 0.0, 0.0) == pytest.approx(3 * 8.0 * 88 * sm.U + math.sqrt(sm.msd_bound(7, 8.0, 0.0)))
    big, small = sm.distance_bound(7, 8.0, 0.05, 1e-9), sm.distance_bound(7, 8.0, 0.05, 0.1)
    assert small < big  # far from zero the square root does not amplify the error of the mean square
    assert sm.norm_bound(7, 8.0, 0.05, 0.1, 2.5, 8.0 ** 6 / 4) > sm.distance_bound(7, 8.0, 0.05, 0.1) / 2.5


def test_parameter_validation():
    p = sm.StructureMatchParams()
    assert (p.ltol, p.angle_tol, p.stol, p.max_mappings) == (0.2, 5.0, 0.3, 192) and p.angle_tol_rad == float(np.float32(math.radians(5.0)))
    for bad in (dict(ltol=0.0), dict(ltol=-1.0), dict(ltol=float("nan")), dict(ltol="0.2"), dict(angle_tol=0), dict(angle_tol=float("inf")),
                dict(stol=True), dict(stol=-0.3), dict(max_mappings=0), dict(max_mappings=4097), dict(max_mappings=1.5), dict(max_mappings=True)):
        with pytest.raises(ValueError):
            sm.StructureMatchParams(**bad)
    assert sm.StructureMatchParams(max_mappings=4096).max_mappings == sm.MAX_MAPPINGS_CAP
    assert sm.describe(0) == "ok" and sm.describe(sm.EMPTY | sm.DIFFERENT) == "EMPTY|DIFFERENT"
    assert [bit for bit, _ in sm.FLAG_NAMES] == [1, 2, 4, 8, 16, 32, 64, 128]
    targets = SampleResult(frac_x=np.zeros((1, 3)), lattice=np.eye(3)[None], num_atoms=np.array([1]), atomic_numbers=np.array([6]))
    assert sm.resolve(None) is None and sm.resolve(targets) == (targets, sm.StructureMatchParams(), None)
    assert sm.resolve((targets, cases.PARAMS)) == (targets, cases.PARAMS, None) and sm.resolve((targets, cases.PARAMS, "any"))[2] == "any"
    for bad in ((targets, 0.3), SampleResult(), "targets.npz", (targets,), (targets, cases.PARAMS, "best")):
        with pytest.raises(ValueError):
            sm.resolve(bad)


def _set(counts, types):
    return SampleResult(num_atoms=np.asarray(counts), atomic_numbers=np.asarray(types))


def test_pairing_helpers():
    assert np.array_equal(sm.paired(3), [[0, 0], [1, 1], [2, 2]]) and sm.paired(3).dtype == np.int32 and sm.paired(0).shape == (0, 2)
    x = _set([2, 3, 0, 2], [11, 17, 8, 8, 26, 17, 11])
    y = _set([3, 2, 2, 2], [8, 26, 8, 17, 11, 11, 11, 11, 17])
    assert sm.compositions(x) == [((11, 1), (17, 1)), ((8, 2), (26, 1)), (), ((11, 1), (17, 1))]
    pairs = sm.same_composition(x, y)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[0, 1], [0, 3], [1, 0], [3, 1], [3, 3]]  # (the empty crystal pairs with nothing)
    assert sm.same_composition(x, _set([1], [5])).shape == (0, 2)
    assert sm.same_composition(([2], [1, 1]), ([2, 2], [1, 1, 1, 2])).tolist() == [[0, 0]]
    res = {"rms_norm": np.array([0.2, 0.1, np.inf, 0.3, 0.3])}
    best = sm.best_per_x(pairs, res, 4)
    assert best["best"].tolist() == [3, -1, -1, 1] and best["n_comparable"].tolist() == [2, 1, 0, 2] and best["row"].tolist() == [1, -1, -1, 3]
    assert best["best_rms_norm"].tolist() == [0.1, np.inf, np.inf, 0.3]


def _pair_results(P, stride):
    return {"rms": np.arange(P, dtype=np.float32), "rms_norm": np.arange(P, dtype=np.float32) / 10, "max_dist": np.arange(P, dtype=np.float32) * 2,
            "mapping": np.full(P, 16484, np.int32), "translation": np.ones((P, 3), np.float32), "partner": np.tile(np.arange(stride, dtype=np.int32), (P, 1)),
            "n_mappings": np.full(P, 2, np.int32), "n_candidates": np.full(P, 2, np.int32), "n_permutations": np.ones(P, np.int32),
            "matched": np.ones(P, np.int32), "flags": np.zeros(P, np.int32)}


def test_per_crystal_reduction():
    counts = [2, 3, 1]
    res = _pair_results(3, 3)
    out = sm.per_crystal(res, sm.paired(3), counts, "paired")
    assert set(out) == set(sm.MATCH_KEYS) and out["target"].tolist() == [0, 1, 2] and out["partner"].tolist() == [0, 1, 0, 1, 2, 0]
    assert out["rms"].tolist() == [0, 1, 2] and out["n_comparable"].tolist() == [1, 1, 1]
    res = _pair_results(3, 3)
    res["rms_norm"][:] = [0.5, 0.25, np.inf]
    res["rms"][2], res["flags"][2], res["matched"][2] = np.inf, sm.NO_PERMUTATION, 0
    out = sm.per_crystal(res, np.array([[0, 4], [0, 2], [2, 7]]), counts, "any")
    assert out["target"].tolist() == [2, -1, -1] and out["n_comparable"].tolist() == [2, 0, 1]
    assert out["flags"].tolist() == [0, sm.DIFFERENT, sm.NO_PERMUTATION] and out["matched"].tolist() == [1, 0, 0]
    assert out["rms"][0] == 1 and np.isinf(out["rms"][1]) and np.isinf(out["rms"][2]) and out["mapping"].tolist() == [16484, -1, 16484]
    assert out["partner"].tolist() == [0, 1, -1, -1, -1, 0] and out["translation"].shape == (3, 3) and not out["translation"][1].any()
    kept = instruments.select(instruments.BY_KEYWORD["match_to"], sm.sample_arrays(out), [0, 2], [0, 1, 5])
    assert kept["target"].tolist() == [2, -1] and kept["partner"].tolist() == [0, 1, 0]
    both = instruments.concat(instruments.BY_KEYWORD["match_to"], [sm.sample_arrays(out), sm.sample_arrays(out)])
    assert both["flags"].shape == (6,) and both["partner"].shape == (12,)


def test_summary_lines():
    a = {"flags": np.array([0, 0, sm.DIFFERENT, sm.NO_MAPPING]), "matched": np.array([1, 0, 0, 0]), "rms_norm": np.array([0.04, 0.5, np.inf, np.inf]),
         "rms": np.array([0.1, 1.2, np.inf, np.inf])}
    b = {"flags": np.array([0, 0]), "matched": np.array([1, 1]), "rms_norm": np.array([0.02, 0.06]), "rms": np.array([0.05, 0.15])}
    sa, sb = sm.stats_of(a, 1), sm.stats_of(b, 0)
    assert sa["attempted"] == 4 and sa["matched"] == 1 and sa["flags"]["DIFFERENT"] == 1 and sm.match_rate(sa) == 0.25
    lines = sm.summary_lines([sa, sb])
    assert lines[0] == "match rank 0: matched 2 / attempted 2 (rate 1); mean rms_norm 0.04, mean rms 0.1 A; flags none"
    assert lines[1] == "match rank 1: matched 1 / attempted 4 (rate 0.25); mean rms_norm 0.04, mean rms 0.1 A; flags DIFFERENT 1, NO_MAPPING 1"
    assert lines[2] == "match total: matched 3 / attempted 6 (rate 0.5); mean rms_norm 0.04, mean rms 0.1 A; flags DIFFERENT 1, NO_MAPPING 1"
    none = sm.stats_of({"flags": np.array([sm.DIFFERENT]), "matched": np.array([0]), "rms_norm": np.array([np.inf]), "rms": np.array([np.inf])})
    assert sm.format_stats(none) == "match rank 0: matched 0 / attempted 1 (rate 0); mean rms_norm n/a; flags DIFFERENT 1"
    assert sm.format_stats(sm.total_stats([])).startswith("match total: matched 0 / attempted 0 (rate 0)")


def test_the_header_states_the_rules_and_the_constants():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        text = fh.read()
    assert "int arreau_structure_match(" in text and "typedef struct arreau_structure_match_params" in text
    for bit, name in sm.FLAG_NAMES:
        assert f"#define ARREAU_SM_{name} {bit}\n" in text
    assert f"#define ARREAU_SM_MAX_MAPPINGS_CAP {sm.MAX_MAPPINGS_CAP}\n" in text
    block = text[text.index("---- structure match"):text.index("#define ARREAU_SM_NONFINITE")]
    for k in range(1, 10):
        assert f"\n *   {k}. " in block
    for word in ("NOT computed", "Hungarian", "supercells", "outside {-1, 0, 1}"):
        assert word in block, word


def test_match_arrays_travel_through_files_and_the_driver(tmp_path):
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results, select_crystals
    counts = np.array([2, 3, 1])
    match = sm.sample_arrays(sm.per_crystal(_pair_results(3, 3), sm.paired(3), counts, "paired"))
    res = SampleResult(frac_x=np.zeros((6, 3)), atomic_numbers=np.ones(6), lattice=np.tile(np.eye(3), (3, 1, 1)), num_atoms=counts,
                       idx_start=np.array([0, 2, 5]), match=match)
    name = save_sample_results_to_hdf5(res, str(tmp_path / "m.npz"))
    back = load_sample_results_from_hdf5(name)
    assert set(back.match) == set(sm.MATCH_KEYS) and all(np.array_equal(back.match[k], match[k]) for k in sm.MATCH_KEYS)
    res.match = None
    plain = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "p.npz")))
    assert plain.match is None and not any(k.startswith("match_") for k in np.load(str(tmp_path / "p.npz")).files)
    both = concat_results([back, back])
    assert both.match["rms"].shape == (6,) and both.match["partner"].shape == (12,) and concat_results([back, plain]).match is None
    kept = select_crystals(back, [True, False, True])
    assert kept.match["target"].tolist() == [0, 2] and kept.match["partner"].tolist() == [0, 1, 0]
    broken = SampleResult(frac_x=np.zeros((6, 3)), atomic_numbers=np.ones(6), lattice=np.tile(np.eye(3), (3, 1, 1)), num_atoms=counts,
                          idx_start=np.array([0, 2, 5]), match={k: v for k, v in match.items() if k != "rms"})
    with pytest.raises(ValueError, match="match"):
        save_sample_results_to_hdf5(broken, str(tmp_path / "b.npz"))
