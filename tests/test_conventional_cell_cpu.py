"""The conventional-cell instrument without a GPU: the float64 restatement of the chain (diffusion/conventional_cell.py) on the
disguised crystals of tests/conventional_cell_cases.py -- Bravais lattice, centring, Pearson symbol, lengths and angles, the
obverse setting, the round trip through the reduction and the structure match, the rotations in the conventional basis, the copy
of flagged crystals, the margins of the deciding comparisons and the enumeration range --, then argument validation, the
statistics lines, the file round trip, select and concat, the parsers, the header and the argument errors of
sample(conventional_cell=...)."""
import os
import re

import numpy as np
import pytest

from arreau_amd import _hip
from arreau_amd.diffusion import cell_reduction as cr
from arreau_amd.diffusion import conventional_cell as cc
from arreau_amd.diffusion import structure_match as sm
from arreau_amd.diffusion import symmetry_search as ss
from arreau_amd.diffusion.diffusion_loss import SampleResult
from tests import conventional_cell_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = list(enumerate(cases.CASES))
# the cell is exact (only atoms are displaced) up to the float32 rounding of the handed-over rows, which a change of basis with
# entries up to 2 and the conventional transform (entries up to 3) carry: some 40 u of a 15 A row
LENGTH_TOL, ANGLE_TOL = 1e-4, 2e-5
# reduce(conventional) against reduce(input): the positions differ by the float32 rounding of the handed-on fractions (u of
# cells up to 15 A, through transforms with entries up to 3): below 2e-5 A, five hundred times below the displacement noise
ROUND_TRIP_RMS = 2e-5


def rows(ref, b):
    first = np.concatenate([[0], np.cumsum(ref.num_atoms)])
    return slice(int(first[b]), int(first[b + 1]))


def check_case(ref, b, case):
    assert int(ref.flags[b]) == 0, (case.name, cc.describe(ref.flags[b]))
    centring = case.expect_centring or case.centring
    assert cc.BRAVAIS_NAMES[ref.bravais[b]] == case.bravais and cc.CENTRING_NAMES[ref.centring[b]] == centring, case.name
    assert int(ref.n_points[b]) == len(cases.CENTRING_VECTORS[centring]) and int(ref.num_atoms[b]) == case.n_conventional, case.name
    assert cc.pearson_symbol(ref.bravais[b], ref.num_atoms[b]) == case.pearson, case.name
    P = ref.transform[b].astype(np.int64)
    assert cc._idet(P) == int(ref.n_points[b]), case.name
    if case.bravais != "aP":  # (the triclinic cell is the reduced cell as given, not the construction's)
        lengths, angles = cases.expected_cell(case)
        assert np.abs(ref.lengths[b] - lengths).max() <= LENGTH_TOL and np.abs(ref.angles[b] - angles).max() <= ANGLE_TOL, \
            (case.name, ref.lengths[b], np.rad2deg(ref.angles[b]))
    # every rotation is an integer matrix in the conventional basis
    A = cc._adjugate(P)
    for W in ref.rotations[b]:
        assert ((A.T @ W @ P.T) % cc._idet(P) == 0).all(), case.name
    src = ref.source[rows(ref, b)]
    n = int(ref.reduced.n_out[b])
    assert np.array_equal(src, np.tile(np.arange(n), int(ref.n_points[b]))), case.name


@pytest.mark.parametrize("b,case", CLEAN, ids=[c.name for c in cases.CASES])
def test_every_case_gets_its_conventional_cell(b, case):
    _, _, ref = cases.clean_batch()
    check_case(ref, b, case)
    margins = cc.decision_margins(ref, b)
    print(case.name, case.pearson, "margins", [f"{m:.3g}" for m in margins])
    assert all(m >= cc.GUARD_MARGIN for m in margins), (case.name, margins)  # a condition: no listed case is left undecided
    assert cc.search_guarded(ref.found, b, cases.SYMPREC), case.name


def test_rhombohedral_cells_come_out_obverse():
    _, _, ref = cases.clean_batch()
    hr = [b for b, c in CLEAN if c.bravais == "hR"]
    assert len(hr) == 4
    for b in hr:
        P = ref.transform[b].astype(np.int64)
        # (2/3, 1/3, 1/3) of the conventional cell is a lattice point -- an integer row of the reduced basis --, (1/3, 2/3, 1/3) is not
        assert not ((np.array([2, 1, 1]) @ P) % 3).any() and ((np.array([1, 2, 1]) @ P) % 3).any(), cases.CASES[b].name
        assert int(ref.centring[b]) == cc.CENTRING_R
        assert abs(np.rad2deg(ref.angles[b][2]) - 120.0) < 1e-3 and int(ref.n_points[b]) == 3


def _round_trip_rms(ref, b, batch_red):
    frac, lattice, counts, types = batch_red
    first = np.concatenate([[0], np.cumsum(counts)])
    x = (frac[first[b]:first[b + 1]], lattice[b:b + 1], [counts[b]], types[first[b]:first[b + 1]])
    sl = rows(ref, b)
    conv = (ref.frac_x[sl].astype(np.float32), ref.lattice[b:b + 1].astype(np.float32), [int(ref.num_atoms[b])], ref.types[sl])
    red = cr.reduce_reference_f64(*conv, cases.PARAMS.reduction())
    assert int(red.flags[0]) == 0 and int(red.n_out[0]) == counts[b]
    y = cc.reduced_arrays_f64(red, conv[2])
    out = sm.structure_match_reference_f64(x, y, [[0, 0]])
    assert int(out.flags[0]) & sm.NO_RESULT_MASK == 0
    return float(out.rms[0])


@pytest.mark.parametrize("noise", [False, True], ids=["clean", "noisy"])
def test_round_trip_through_the_reduction(noise):
    """reduce(conventional crystal) is reduce(input) under the structure match's float64 restatement: the conventional cell holds
    the same crystal, atoms displaced by rounding alone -- not by the displacement noise."""
    _, _, ref = cases.noisy_batch(2) if noise else cases.clean_batch()
    names = [c.name for c in cases.CASES if not (noise and c.name == cases.LARGEST)]
    for b, name in enumerate(names):
        if name == cases.LARGEST:
            continue  # (48 atoms through the matcher's every candidate: covered by its smaller Fm-3m siblings)
        rms = _round_trip_rms(ref, b, ref.batch)
        print(name, f"rms {rms:.2e} A")
        assert rms <= ROUND_TRIP_RMS, (name, rms)


def test_noisy_variants_are_decided_and_mostly_guarded():
    """Every case under every seed keeps its Bravais lattice, centring and Pearson symbol.  A variant is skipped as unguarded when
    the reduction's restatement flags its disguised cell (then no reduced cell is handed on: rule 3 of the reduction looks for
    the primitive vectors among the nearest images only, which a change of basis with entries of 2 can defeat), when a deciding
    comparison has a relative gap below 1e-3 or when a decision quantity of the search lies between symprec / 2 and 2 symprec: at
    most one in ten may be."""
    total = unguarded = 0
    noisy = [c for c in cases.CASES if c.name != cases.LARGEST]
    for seed in cases.NOISY_SEEDS:
        _, _, ref = cases.noisy_batch(seed)
        for b, case in enumerate(noisy):
            total += 1
            if int(ref.reduced.flags[b]):
                print(f"seed {seed} {case.name}: the reduction flags it {cr.describe(ref.reduced.flags[b])}")
                unguarded += 1
                continue
            check_case(ref, b, case)
            unguarded += not (cc.guarded(ref, b) and cc.search_guarded(ref.found, b, cases.SYMPREC))
    print(f"unguarded {unguarded} / {total}")
    assert total == len(noisy) * 10 and 10 * unguarded <= total


def test_a_wider_enumeration_changes_nothing():
    """The plane vectors are searched among entries -3..3 (DESIGN.md section 7 argues why that holds the shortest ones of a
    Delaunay-reduced cell): entries -5..5 give the same transforms on every case."""
    _, batch, ref = cases.clean_batch()
    wide = cc.conventional_stage_f64(*ref.batch, ref.found, enum_range=5)
    assert np.array_equal(wide.transform, ref.transform) and np.array_equal(wide.bravais, ref.bravais)
    assert np.abs(ref.transform).max() <= 3


def test_flagged_crystals_are_copied_through():
    for name, (f, L, t), params, flag in cases.flagged_items():
        ref = cc.conventional_reference_f64(f, L[None], [len(f)], t, params)
        assert int(ref.flags[0]) == flag, (name, cc.describe(ref.flags[0]))
        assert np.array_equal(ref.transform[0], np.eye(3)) and int(ref.bravais[0]) == -1 and int(ref.n_points[0]) == 1, name
        assert int(ref.num_atoms[0]) == len(f) and np.array_equal(ref.source, np.arange(len(f))), name
        # what is copied is the crystal the chain handed on: the input's own for the first three, the reduced one for the last
        assert np.array_equal(ref.frac_x, ref.batch[0].astype(np.float64), equal_nan=True) and np.array_equal(ref.lattice[0], ref.batch[1][0].astype(np.float64)), name
        if flag != cc.NO_GROUP:
            assert np.array_equal(ref.batch[0], f, equal_nan=True) and np.array_equal(ref.batch[1][0], L), name
        assert cc.pearson_symbol(ref.bravais[0], ref.num_atoms[0]) == "none" and cc.decision_margins(ref, 0) == []
    # a group whose rotations give no admissible basis: a search result that is not the cell's (a 4-fold in an orthorhombic cell)
    f, L, t = cases.build(cases.BY_NAME["ortho-P"], seed=0)
    ref = cc.conventional_reference_f64(f, L[None], [len(f)], t, cases.PARAMS)
    found = ref.found
    found.point_group = np.array([8], np.int32)  # "4": there is no part of order 4
    out = cc.conventional_stage_f64(*ref.batch, found)
    assert int(out.flags[0]) == cc.NO_BASIS and int(out.bravais[0]) == -1 and np.array_equal(out.transform[0], np.eye(3))


def test_argument_validation():
    assert cc.resolve(None) is None and cc.resolve(False) is None and cc.resolve(True) == cc.ConventionalCellParams()
    p = cc.ConventionalCellParams(symprec=0.05, max_ops=48)
    assert cc.resolve(p) is p and (cc.ConventionalCellParams().symprec, cc.ConventionalCellParams().max_ops) == (0.1, 192)
    assert p.search() == ss.SymmetrySearchParams(symprec=0.05, max_ops=48) and p.reduction() == cr.CellReductionParams(symprec=0.05)
    for bad in (0, -1.0, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="symprec"):
            cc.ConventionalCellParams(symprec=bad)
    for bad in (0, 4097, 1.5, True):
        with pytest.raises(ValueError, match="max_ops"):
            cc.ConventionalCellParams(max_ops=bad)
    with pytest.raises(ValueError, match="conventional_cell must be None, True or a ConventionalCellParams"):
        cc.resolve(5)
    cc.check_shared(None, cr.CellReductionParams(symprec=0.3))
    cc.check_shared(p, cr.CellReductionParams(symprec=0.05), ss.SymmetrySearchParams(symprec=0.05, max_ops=48))
    with pytest.raises(ValueError, match="share one reduction"):
        cc.check_shared(p, cr.CellReductionParams(symprec=0.1))
    with pytest.raises(ValueError, match="find_symmetry search with one tolerance"):
        cc.check_shared(p, None, ss.SymmetrySearchParams(symprec=0.05, max_ops=192))
    assert cc.pearson_symbol(13, 8) == "cF8" and cc.pearson_symbol(9, 3) == "hR3" and cc.pearson_symbol(-1, 5) == "none"
    assert len(cc.BRAVAIS_NAMES) == 14 and cc.CENTRING_NAMES == ("P", "A", "B", "C", "I", "F", "R")


class NoEngine:
    def engine(self):
        raise AssertionError("the engine was touched")


def test_sample_rejects_a_bad_conventional_cell_before_any_engine():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    loss = object.__new__(DiffusionLoss)
    loss.T = 100
    state = np.random.get_state()
    kw = dict(model=NoEngine(), z_table=None, num_atoms_per_sample=4, num_samples_in_batch=2)
    with pytest.raises(ValueError, match="conventional_cell must be None, True or a ConventionalCellParams"):
        DiffusionLoss.sample(loss, conventional_cell=5, **kw)
    with pytest.raises(ValueError, match="share one reduction"):
        DiffusionLoss.sample(loss, conventional_cell=True, reduce_cell=cr.CellReductionParams(symprec=0.05), **kw)
    with pytest.raises(ValueError, match="search with one tolerance"):
        DiffusionLoss.sample(loss, conventional_cell=True, find_symmetry=ss.SymmetrySearchParams(max_ops=48), **kw)
    assert np.array_equal(np.random.get_state()[1], state[1])  # nothing drawn
    assert SampleResult().conventional is None


def test_parsers_take_the_flag():
    from arreau_amd import generate, screen
    for parser in (generate.build_parser(), screen.build_parser()):
        flags = {s for a in parser._actions for s in a.option_strings}
        assert {"--conventional_cell", "--symprec"} <= flags
    args = screen.build_parser().parse_args(["f.npz", "--conventional_cell", "--symprec", "0.05", "--out", "c.npz"])
    assert args.conventional_cell and generate.instrument_params("conventional_cell", args, None) == cc.ConventionalCellParams(symprec=0.05)
    assert not screen.build_parser().parse_args(["f.npz"]).conventional_cell
    for other in ("--reduce_cell", "--symmetrize"):
        with pytest.raises(SystemExit):
            screen.main(["f.npz", "--conventional_cell", other, "--out", "c.npz"])
    args.symprec = -1.0
    errors = []
    generate.instrument_params("conventional_cell", args, errors.append)
    assert errors and "conventional cell" in errors[0]


def test_screen_rejects_out_with_the_other_cells(capsys):
    from arreau_amd import screen
    with pytest.raises(SystemExit):
        screen.main(["f.npz", "--conventional_cell", "--reduce_cell", "--out", "c.npz"])
    assert "run them in turn" in capsys.readouterr().err


def test_header_and_binding_agree():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        text = fh.read()
    assert "int arreau_crystal_conventional(const float* d_frac, const int32_t* d_types, const float* d_lattice" in text
    defs = {k: int(v) for k, v in re.findall(r"#define ARREAU_CONV_(\w+) (\d+)", text)}
    assert defs == {name: bit for bit, name in cc.FLAG_NAMES}
    fields = re.search(r"typedef struct arreau_conventional_result \{(.*?)\} arreau_conventional_result;", text, re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == cc.RESULT_KEYS
    assert tuple(n for n, _ in _hip.ConventionalResultC._fields_) == cc.RESULT_KEYS and "arreau_crystal_conventional" in _hip.EXPORTS
    assert "entries in -3..3" in text and cc.ENUM_RANGE == 3
    with open(os.path.join(ROOT, "arreau_amd", "csrc", "conventional.hip")) as fh:
        assert "#define CONV_RANGE 3 " in fh.read()


def _result(ref, batch):
    frac, lattice, counts, types = batch
    num = np.array(counts, dtype=np.int64)
    return SampleResult(frac_x=frac.astype(np.float64), atomic_numbers=types.astype(np.float64), lattice=lattice.astype(np.float64),
                        num_atoms=num, idx_start=np.cumsum(num) - num, conventional=cases.reference_arrays(ref))


def test_summary_lines():
    _, _, ref = cases.clean_batch()
    arrays = cases.reference_arrays(ref)
    arrays["flags"] = arrays["flags"].copy()
    arrays["bravais"] = arrays["bravais"].copy()
    arrays["flags"][0], arrays["bravais"][0] = cc.NO_GROUP, -1
    lines = cc.summary_lines([cc.stats_of(arrays, 0)])
    assert lines[0] == ("conventional cell rank 0: classified 23 / attempted 24; aP 1, mP 1, mS 1, oP 2, oS 2, oI 1, oF 1, tP 1, tI 1, hR 4, "
                        "hP 1, cP 2, cI 1, cF 4; flags NO_GROUP 1")
    assert lines[1].startswith("conventional cell total: classified 23 / attempted 24")
    two = cc.summary_lines([cc.stats_of(arrays, 0), cc.stats_of(arrays, 1)])
    assert len(two) == 3 and "classified 46 / attempted 48" in two[2] and "cF 8" in two[2]


def test_file_round_trip_select_and_concat(tmp_path):
    from arreau_amd.diffusion import instruments
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results, select_crystals
    _, batch, ref = cases.clean_batch()
    res = _result(ref, batch)
    back = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "c.npz")))
    assert set(back.conventional) == set(cc.CONVENTIONAL_KEYS)
    for k in cc.CONVENTIONAL_KEYS:
        assert np.array_equal(back.conventional[k], res.conventional[k]), k
    stored = [k for k in np.load(str(tmp_path / "c.npz")).files if k.startswith("conventional_")]
    assert stored == ["conventional_" + k for k in cc.CONVENTIONAL_KEYS]
    # a file without the field loads with None, and is written as before
    res.conventional = None
    plain = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "p.npz")))
    assert plain.conventional is None and list(np.load(str(tmp_path / "p.npz")).files) == ["frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms"]
    res.conventional = cases.reference_arrays(ref)
    # select: the rows of the kept crystals and of THEIR conventional atoms
    keep = np.zeros(len(cases.CASES), dtype=bool)
    keep[[3, 9]] = True  # fcc (4 atoms), rhombohedral-70 (3 atoms)
    some = select_crystals(res, keep)
    assert some.conventional["num_atoms"].tolist() == [4, 3] and some.conventional["frac_x"].shape == (7, 3)
    assert some.conventional["source"].tolist() == [0] * 7 and [cc.BRAVAIS_NAMES[k] for k in some.conventional["bravais"]] == ["cF", "hR"]
    sl = rows(ref, 9)
    assert np.array_equal(some.conventional["frac_x"][4:], ref.frac_x[sl])
    both = concat_results([some, some])
    assert both.conventional["num_atoms"].tolist() == [4, 3, 4, 3] and both.conventional["atomic_numbers"].shape == (14,)
    assert concat_results([some, select_crystals(plain, keep)]).conventional is None
    with pytest.raises(ValueError, match="conventional"):
        res.conventional = {k: v for k, v in res.conventional.items() if k != "source"}
        save_sample_results_to_hdf5(res, str(tmp_path / "bad.npz"))
    # the table: the six stay six, the derived one follows them
    assert len(instruments.INSTRUMENTS) == 6 and [e.keyword for e in instruments.DERIVED] == ["conventional_cell"]
    assert instruments.ALL == instruments.INSTRUMENTS + instruments.DERIVED and instruments.BY_KEYWORD["conventional_cell"].field == "conventional"

