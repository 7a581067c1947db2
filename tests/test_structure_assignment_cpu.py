"""The structure match's assignment step without a GPU (rule 6b; diffusion/structure_match.py): the module's solver against brute
force and against scipy, the gap to the runner-up assignment, the guards of tests/structure_assignment_cases.py, "nearest" as it
was, what "optimal" changes and what it leaves, the derived solver bound, the parameter, the flag, the command-line flag and the
header."""
import argparse
import itertools
import math
import os

import numpy as np
import pytest

from arreau_amd import _hip
from arreau_amd.diffusion import instruments
from arreau_amd.diffusion import structure_match as sm
from arreau_amd.diffusion import symmetry_search as ss
from tests import structure_assignment_cases as cases
from tests import structure_match_cases as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = 16484  # the code of W = 1


def brute(C):
    """(the smallest sum, the maps that attain it, the smallest sum of any other map) over all permutations."""
    n = C.shape[0]
    sums = sorted((float(C[np.arange(n), list(p)].sum()), p) for p in itertools.permutations(range(n)))
    best = sums[0][0]
    return best, [p for s, p in sums if s == best], (sums[1][0] if len(sums) > 1 else math.inf)


def matrices():
    rng = np.random.default_rng(4)
    out = []
    for n in range(1, 8):
        for _ in range(4):
            out.append(rng.uniform(0.0, 9.0, (n, n)))
            out.append(rng.integers(0, 4, (n, n)).astype(np.float64))  # tied: many equal sums, exact in float64
        if n >= 3:  # two species: the pairs across them are excluded
            C = rng.uniform(0.0, 9.0, (n, n))
            kind = np.arange(n) % 2
            C[kind[:, None] != kind[None, :]] = np.inf
            out.append(C)
    return out


def test_the_solver_against_brute_force():
    for C in matrices():
        n = C.shape[0]
        cols, duals = sm.linear_assignment(C)
        best, maps, second = brute(C)
        assert sorted(cols.tolist()) == list(range(n)) and tuple(cols.tolist()) in maps, C
        assert abs(C[np.arange(n), cols].sum() - best) <= 1e-12 * max(1.0, best)
        gap = sm.assignment_gap(C, cols, duals)
        want = second - best if n > 1 else math.inf
        assert gap == want or abs(gap - want) <= 1e-9, (n, gap, want)
    with pytest.raises(ValueError, match="no one-to-one map"):
        sm.linear_assignment(np.array([[1.0, np.inf], [2.0, np.inf]]))


def test_the_solver_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(9)
    for n in (2, 3, 8, 17, 33, 64):
        for tied in (False, True):
            C = rng.integers(0, 6, (n, n)).astype(np.float64) if tied else rng.uniform(0.0, 9.0, (n, n))
            cols, duals = sm.linear_assignment(C)
            r, c = opt.linear_sum_assignment(C)
            assert sorted(cols.tolist()) == list(range(n))
            assert abs(C[np.arange(n), cols].sum() - C[r, c].sum()) <= 1e-9
            if sm.assignment_gap(C, cols, duals) > 1e-9:
                assert np.array_equal(cols, c)


def test_every_case_is_guarded_and_flagged_as_expected():
    ref, near = cases.reference(), cases.nearest_reference()  # (assert the guards of every pair under both rules; none exempt)
    solved = 0
    for k, pair in enumerate(cases.pairs()):
        assert int(ref.flags[k]) == pair.flags, (pair.name, sm.describe(ref.flags[k]))
        if pair.n_mappings is not None:
            assert int(ref.n_mappings[k]) == pair.n_mappings, pair.name
        solved += len(ref.solved[k] or [])
        print(f"{pair.name}: rms {ref.rms[k]:.6f} A, rms_norm {ref.rms_norm[k]:.4f}, {len(ref.solved[k] or [])} of {ref.n_candidates[k]} candidates solved; "
              + ", ".join(f"gap {s['gap']:.4g} (4 x bound {4 * cases.solver_error(ref, k, s):.3g})" for s in (ref.solved[k] or [])[:2]))
    names = [p.name for p in cases.pairs()]
    assert len(set(names)) == len(names) and solved >= 12 and set(cases.TIE_CASES) <= set(names)
    sizes = sorted(cases.crystals()[p.x].n for p in cases.pairs())
    assert {1, 70, cases.ABOVE_LDS, 257} <= set(sizes) and cases.ABOVE_LDS == sm.ASSIGN_LDS_ATOMS + 1
    assert near.flags.tolist().count(sm.NO_PERMUTATION) >= 5


def test_nearest_is_the_existing_reference_on_the_existing_cases():
    ref = base.reference()
    again = sm.structure_match_reference_f64(base.batch(), base.batch(), base.pair_list(), sm.StructureMatchParams(
        ltol=base.PARAMS.ltol, angle_tol=base.PARAMS.angle_tol, stol=base.PARAMS.stol, max_mappings=base.PARAMS.max_mappings, assignment="nearest"),
        details=True)
    assert base.PARAMS.assignment == "nearest" and sm.StructureMatchParams().assignment == "nearest"
    for k in sm.PAIR_KEYS + ("D", "ell", "det_gm", "l1"):
        assert np.array_equal(getattr(ref, k), getattr(again, k), equal_nan=True), k
    assert ref.survivors == again.survivors and again.contenders == again.survivors and not any(again.solved[k] for k in range(len(base.pairs())))
    assert not (again.flags & sm.ASSIGNED).any()


def test_optimal_keeps_the_counts_and_drops_no_pair():
    ref, near = cases.reference(), cases.nearest_reference()
    for k in ("n_mappings", "n_candidates", "n_permutations"):
        assert np.array_equal(getattr(ref, k), getattr(near, k)), k
    assert not (ref.flags & sm.NO_PERMUTATION).any()
    for k, pair in enumerate(cases.pairs()):
        if int(ref.flags[k]) & sm.NO_RESULT_MASK:
            assert int(ref.flags[k]) == int(near.flags[k]), pair.name
            continue
        assert len(ref.contenders[k]) == ref.n_candidates[k] and len(ref.solved[k]) == ref.n_candidates[k] - ref.n_permutations[k], pair.name
        n = cases.crystals()[pair.x].n
        part = ref.partner[k, :n]
        assert sorted(part.tolist()) == list(range(n)) and np.array_equal(cases.crystals()[pair.y].types[part], cases.crystals()[pair.x].types)
        # ASSIGNED exactly where the winning candidate was solved
        _, code, q = ref.contenders[k][0]
        won_solved = any(s["code"] == code and s["q"] == q for s in ref.solved[k])
        assert bool(int(ref.flags[k]) & sm.ASSIGNED) == won_solved and int(ref.mapping[k]) == code, pair.name
        if not won_solved:  # the winner is the nearest rule's
            assert ref.rms[k] == near.rms[k] and np.array_equal(ref.partner[k], near.partner[k]), pair.name


@pytest.mark.parametrize("name", [p.name for p in cases.pairs() if p.rms is not None])
def test_solved_pairs_have_the_rms_written_out_where_they_are_built(name):
    ref, k = cases.reference(), cases.pair_index(name)
    pair = cases.pairs()[k]
    print(f"{name}: rms {ref.rms[k]:.9f} A, written out {pair.rms:.9f} A")
    assert abs(ref.rms[k] - pair.rms) <= cases.input_rounding(pair)
    assert ref.matched[k] == 1 and ref.rms_norm[k] <= cases.PARAMS.stol / 2 and int(ref.mapping[k]) == IDENTITY
    assert ref.partner[k, :cases.crystals()[pair.x].n].tolist() == list(range(cases.crystals()[pair.x].n))
    assert cases.nearest_reference().matched[k] == 0


def candidate(pair, code, assignment):
    Z = cases.crystals()
    x, y = Z[pair.x], Z[pair.y]
    A, B = x.lattice.astype(np.float64), y.lattice.astype(np.float64)
    W = ss.decode_rotation(code)
    Gp = W.T.astype(np.float64) @ (B @ B.T) @ W.astype(np.float64)
    return sm.evaluate_candidate(ss._wrap01(x.frac.astype(np.float64)), ss._wrap01(y.frac.astype(np.float64)), x.types, y.types, A @ A.T, Gp, W,
                                 q=0, p0=0, assignment=assignment)


def test_the_chain_is_a_path_through_four_atoms():
    pair = cases.pairs()[cases.pair_index("chain: a path through four atoms")]
    near, best = candidate(pair, IDENTITY, "nearest"), candidate(pair, IDENTITY, "optimal")
    assert near.partner.tolist() == [0, 2, 3, 4, 4] and not near.permutation and not near.solved  # the last row is the free one
    assert best.partner.tolist() == [0, 1, 2, 3, 4] and best.solved and not best.permutation and best.gap > 1.0


def test_the_species_are_excluded():
    """Three species: the nearest atom of y of ANY species belongs to the other species for some atom of x; the map keeps the species."""
    k = cases.pair_index("three species: collisions in two of them")
    pair, Z = cases.pairs()[k], cases.crystals()
    x, y = Z[pair.x], Z[pair.y]
    L = x.lattice.astype(np.float64)
    d = y.frac.astype(np.float64)[None] - x.frac.astype(np.float64)[:, None]
    dist = np.linalg.norm((d - np.rint(d)) @ L, axis=2)
    assert (y.types[dist.argmin(axis=1)] != x.types).any()
    assert cases.reference().partner[k, :5].tolist() == [0, 1, 2, 3, 4]


def test_the_winner_changes_with_the_assignment():
    k = cases.pair_index("two candidates: the winner changes with the assignment")
    ref, near = cases.reference(), cases.nearest_reference()
    assert int(ref.mapping[k]) == IDENTITY and int(near.mapping[k]) != IDENTITY and near.flags[k] == 0 and ref.flags[k] == sm.ASSIGNED
    assert ref.n_permutations[k] == near.n_permutations[k] == 1
    assert near.rms[k] > 4 * ref.rms[k] and ref.matched[k] == 1 and near.matched[k] == 0


def test_the_tie_is_a_tie():
    k = cases.pair_index(cases.TIE_CASES[0])
    ref = cases.reference()
    assert ref.n_permutations[k] == 0 and len(ref.solved[k]) == 192
    won = [s for s in ref.solved[k] if (s["code"], s["q"]) == ref.contenders[k][0][1:]]
    print("gap of the winning candidate:", won[0]["gap"])
    assert won[0]["gap"] <= 4 * cases.solver_error(ref, k, won[0])  # (a case the gap guard would refuse)
    assert ref.matched[k] == 0 and ref.rms_norm[k] >= 2 * cases.PARAMS.stol


def test_the_existing_no_permutation_pair_gets_a_result():
    k = base.pair_index("two atoms of x at one atom of y")
    params = sm.StructureMatchParams(ltol=0.2, angle_tol=5.0, stol=0.05, max_mappings=192, assignment="optimal")
    ref = sm.structure_match_reference_f64(base.batch(), base.batch(), base.pair_list()[k:k + 1], params)
    assert base.reference().flags[k] == sm.NO_PERMUTATION and ref.flags[0] == sm.ASSIGNED and np.isfinite(ref.rms[0]) and ref.n_permutations[0] == 0
    assert sorted(ref.partner[0, :3].tolist()) == [0, 1, 2]


def test_the_solver_bound():
    """From the module's derivation: it grows with the optimum, the cell and the atom count, and covers a cost entry's own bound."""
    b = sm.solver_bound(20, 8.0, 16.0, 1.0)
    assert 0.0 < b < 1e-2 and sm.solver_bound(20, 8.0, 16.0, 4.0) > b and sm.solver_bound(20, 16.0, 16.0, 1.0) > b and sm.solver_bound(40, 8.0, 16.0, 1.0) > b
    assert sm.solver_bound(1, 8.0, 16.0, 1.0) >= 2 * sm.cost_bound(8.0, 16.0, 1.0) > 2.0 ** -24
    a, bb, c0 = 342 * sm.U * 64 / 16, 216 * sm.U * 8, (108 * sm.U * 8) ** 2 + 2.0 ** -25
    f = a + bb * math.sqrt(20) + 20 * c0
    x = sm.solver_bound(20, 8.0, 16.0, 1.0)
    assert x * (1 - a) - bb * math.sqrt(20 * x) - 2 * f == pytest.approx(0.0, abs=1e-12)


def test_the_parameter_and_the_flag():
    assert sm.StructureMatchParams(assignment="optimal").assignment == "optimal" and sm.ASSIGNMENTS == {"nearest": 0, "optimal": 1}
    for bad in ("hungarian", "", None, 1, "Optimal"):
        with pytest.raises(ValueError, match="assignment"):
            sm.StructureMatchParams(assignment=bad)
    assert sm.ASSIGNED == 256 and not sm.ASSIGNED & sm.NO_RESULT_MASK and (sm.ASSIGNED, "ASSIGNED") in sm.ALL_FLAG_NAMES
    assert sm.ALL_FLAG_NAMES[:len(sm.FLAG_NAMES)] == sm.FLAG_NAMES
    assert sm.describe(sm.ASSIGNED) == "ASSIGNED" and sm.describe(sm.OVERFLOW | sm.ASSIGNED) == "OVERFLOW|ASSIGNED"
    a = {"flags": np.array([sm.ASSIGNED, 0, sm.ASSIGNED | sm.OVERFLOW, sm.DIFFERENT]), "matched": np.array([1, 1, 0, 0]),
         "rms_norm": np.array([0.04, 0.02, 0.5, np.inf]), "rms": np.array([0.1, 0.05, 1.2, np.inf])}
    st = sm.stats_of(a)
    assert st["flags"]["ASSIGNED"] == 2 and st["matched"] == 2
    old = dict(st, flags={n: v for n, v in st["flags"].items() if n != "ASSIGNED"})  # (statistics written before the flag existed)
    assert sm.total_stats([st, old])["flags"]["ASSIGNED"] == 2
    assert sm.summary_lines([st])[0].endswith("flags DIFFERENT 1, OVERFLOW 1, ASSIGNED 2")


def test_the_command_line_flag():
    from arreau_amd.generate import add_structure_match_arguments, instrument_params
    assert ("assignment", "assignment") in instruments.BY_KEYWORD["match_to"].flags
    ap = argparse.ArgumentParser()
    add_structure_match_arguments(ap)
    assert instrument_params("match_to", ap.parse_args([]), ap.error) == sm.StructureMatchParams()
    got = instrument_params("match_to", ap.parse_args(["--assignment", "optimal", "--stol", "0.2"]), ap.error)
    assert got == sm.StructureMatchParams(stol=0.2, assignment="optimal")
    with pytest.raises(SystemExit):
        ap.parse_args(["--assignment", "best"])


def test_the_header_states_rule_6b_and_the_constants():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        text = fh.read()
    assert "int arreau_structure_match_assigned(" in text and "arreau_structure_match_assigned" in _hip.EXPORTS
    for name, value in (("ASSIGNED", sm.ASSIGNED), ("ASSIGN_NEAREST", 0), ("ASSIGN_OPTIMAL", 1), ("ASSIGN_LDS_ATOMS", sm.ASSIGN_LDS_ATOMS),
                        ("ASSIGN_STATE_ROWS", sm.ASSIGN_STATE_ROWS)):
        assert f"#define ARREAU_SM_{name} {value}" in text, name
    block = text[text.index("---- structure match"):text.index("#define ARREAU_SM_NONFINITE")]
    for word in ("\n *  6b. ", "UNREFINED", "ascending i", "smallest j", "excluded", "ASSIGNED", "n_permutations keeps its meaning"):
        assert word in block, word
    assert "no Hungarian" not in text
