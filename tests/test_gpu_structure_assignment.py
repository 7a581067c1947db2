"""The structure match's assignment step on the device (arreau_structure_match_assigned, csrc/match.hip, rule 6b) against the
float64 restatement on the guarded pairs of tests/structure_assignment_cases.py, one ragged launch with X and Y the same batch:
integers, flags, mapping and partner equal where the restatement's winner stands clear, the reals within the bounds derived in
diffusion/structure_match.py, the device's own choice checked in float64 where candidates or assignments tie.  Then: NEAREST
through the new entry point is arreau_structure_match bit for bit, OPTIMAL leaves every pair of the existing batch whose winner
does not change as it was, repeated runs, a permuted pair list and a split launch agree bit for bit, sample(match_to=...), the
command lines, the argument errors, the symbol.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import structure_match as sm
from arreau_amd.diffusion import symmetry_search as ss
from tests import structure_assignment_cases as cases
from tests import structure_match_cases as base
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("flags", "n_mappings", "n_candidates", "n_permutations", "matched")
BASE_OPTIMAL = sm.StructureMatchParams(ltol=base.PARAMS.ltol, angle_tol=base.PARAMS.angle_tol, stol=base.PARAMS.stol,
                                       max_mappings=base.PARAMS.max_mappings, assignment="optimal")
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, batch):
    frac, lattice, counts, types = batch
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return up(dev, frac.reshape(-1, 3)), up(dev, lattice), up(dev, off), up(dev, types)


def launch(dev, batch, pair_list, params, **kw):
    z = device_batch(dev, batch)
    return sm.result_to_numpy(sm.match(z, z, pair_list, params, **kw))  # (Y is X: the same tensors)


def run(dev, what):
    """The launches more than one test reads (cached): the new cases under OPTIMAL, the existing batch under both rules."""
    if what not in _RUN:
        _RUN[what] = {"new": lambda: launch(dev, cases.batch(), cases.pair_list(), cases.PARAMS),
                      "base nearest": lambda: launch(dev, base.batch(), base.pair_list(), base.PARAMS),
                      "base optimal": lambda: launch(dev, base.batch(), base.pair_list(), BASE_OPTIMAL)}[what]()
    return _RUN[what]


def mod1(d):
    return np.abs(d - np.rint(d))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def atoms_of(pair):
    return cases.crystals()[pair.x].n


def clear(ref, k, pair):
    """Compared exactly: no named tie case, and the restatement's best contender stands clear of the next."""
    return pair.name not in cases.TIE_CASES and cases.decisive(ref, k, cases.bounds(ref, k, atoms_of(pair))["rms"])


def test_integers_flags_mapping_and_partner_equal_the_f64_restatement(dev):
    got, ref = run(dev, "new"), cases.reference()
    for k in INT_KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), (k, got[k], getattr(ref, k))
    assert not (got["flags"] & sm.NO_PERMUTATION).any() and got["partner"].shape == (len(cases.pairs()), 257)
    exact = 0
    for k, pair in enumerate(cases.pairs()):
        n = atoms_of(pair)
        if int(ref.flags[k]) & sm.NO_RESULT_MASK:
            assert np.isposinf(got["rms"][k]) and got["mapping"][k] == -1 and (got["partner"][k] == -1).all(), pair.name
            continue
        assert sorted(got["partner"][k, :n].tolist()) == list(range(n)) and (got["partner"][k, n:] == -1).all(), pair.name
        assert np.array_equal(cases.crystals()[pair.y].types[got["partner"][k, :n]], cases.crystals()[pair.x].types), pair.name
        if clear(ref, k, pair):
            assert got["mapping"][k] == ref.mapping[k] and np.array_equal(got["partner"][k, :n], ref.partner[k, :n]), pair.name
            exact += 1
    assert exact >= 7  # every solved case but the tie


def test_reals_stay_within_the_derived_bounds(dev):
    got, ref = run(dev, "new"), cases.reference()
    for k, pair in enumerate(cases.pairs()):
        if int(ref.flags[k]) & sm.NO_RESULT_MASK:
            continue
        bound = cases.bounds(ref, k, atoms_of(pair))
        err = {"rms": abs(float(got["rms"][k]) - ref.rms[k]), "max_dist": abs(float(got["max_dist"][k]) - ref.max_dist[k]),
               "rms_norm": abs(float(got["rms_norm"][k]) - ref.rms_norm[k])}
        if clear(ref, k, pair):
            err["translation"] = float(mod1(got["translation"][k] - ref.translation[k]).max())
        else:  # (another of the tied maps may hold another largest distance: the test below checks the device's own)
            del err["max_dist"]
        print(f"{pair.name}: " + ", ".join(f"{q} {err[q]:.3e} (bound {bound[q]:.3e})" for q in err))
        for q in err:
            assert err[q] <= bound[q], (pair.name, q, err[q], bound[q])


def test_where_maps_tie_the_device_holds_one_of_the_best(dev):
    got, ref = run(dev, "new"), cases.reference()
    Z, tied = cases.crystals(), 0
    for k, pair in enumerate(cases.pairs()):
        if int(ref.flags[k]) & sm.NO_RESULT_MASK or clear(ref, k, pair):
            continue
        tied += 1
        n, bound = atoms_of(pair), cases.bounds(ref, k, atoms_of(pair))
        x, y = Z[pair.x], Z[pair.y]
        A, B = x.lattice.astype(np.float64), y.lattice.astype(np.float64)
        W = ss.decode_rotation(int(got["mapping"][k]))
        assert abs(round(np.linalg.det(W))) == 1
        Gp = W.T.astype(np.float64) @ (B @ B.T) @ W.astype(np.float64)
        c = sm.evaluate_candidate(ss._wrap01(x.frac.astype(np.float64)), ss._wrap01(y.frac.astype(np.float64)), x.types, y.types, A @ A.T, Gp, W,
                                  t=got["translation"][k].astype(np.float64), partner=got["partner"][k, :n])
        slack = bound["rms"] + 3.0 * float(ref.l1[k]) * bound["translation"]
        print(f"{pair.name}: device rms {got['rms'][k]:.6e}, its choice in float64 {c.rms:.6e}, the restatement's minimum {ref.rms[k]:.6e} (bound {slack:.3e})")
        assert abs(c.rms - float(got["rms"][k])) <= slack and abs(float(got["rms"][k]) - ref.rms[k]) <= bound["rms"], pair.name
        assert abs(c.max_dist - float(got["max_dist"][k])) <= bound["max_dist"] + 3.0 * float(ref.l1[k]) * bound["translation"], pair.name
    assert tied >= 2  # (the rock salt tie and the one atom)


def call_assigned(dev, z, pairs, params, out, scratch, assignment, cost):
    c = _hip.StructureMatchParamsC(params.ltol, params.angle_tol_rad, params.stol, params.max_mappings)
    r = _hip.StructureMatchResultC(*[_hip.ptr(out[k]).value for k in sm.PAIR_KEYS], _hip.ptr(scratch).value, int(out["partner"].shape[1]))
    side = [_hip.ptr(z[0]), _hip.ptr(z[3]), _hip.ptr(z[1]), _hip.ptr(z[2]), int(z[1].shape[0]), int(z[0].shape[0])]
    return _hip.lib().arreau_structure_match_assigned(*side, *side, _hip.ptr(pairs), int(pairs.shape[0]), ctypes.byref(c), ctypes.byref(r), assignment,
                                                      _hip.ptr(cost), _hip.stream_ptr(dev))


def empty_outputs(dev, P, stride):
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    out = {k: torch.full((P,), -7, **(f32 if k in ("rms", "rms_norm", "max_dist") else i32)) for k in sm.PAIR_KEYS}
    out["translation"], out["partner"] = torch.full((P, 3), -7.0, **f32), torch.full((P, stride), -7, **i32)
    return out, torch.empty((P, sm.WAVES, stride), **i32)


def test_nearest_through_the_new_entry_point_is_the_old_one_bit_for_bit(dev):
    want = run(dev, "base nearest")
    z, pairs = device_batch(dev, base.batch()), up(dev, base.pair_list())
    out, scratch = empty_outputs(dev, int(pairs.shape[0]), 257)
    assert call_assigned(dev, z, pairs, base.PARAMS, out, scratch, 0, None) == 0  # (NEAREST needs no d_cost)
    got = sm.result_to_numpy(out)
    for k in sm.PAIR_KEYS:
        assert np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.fixture(scope="module")
def base_optimal_reference():
    return sm.structure_match_reference_f64(base.batch(), base.batch(), base.pair_list(), BASE_OPTIMAL, details=True)


def test_optimal_leaves_the_pairs_whose_winner_stays(dev, base_optimal_reference):
    near, best, ref, opt = run(dev, "base nearest"), run(dev, "base optimal"), base.reference(), base_optimal_reference
    same = 0
    for k, pair in enumerate(base.pairs()):
        stays = int(opt.flags[k]) == int(ref.flags[k]) and int(opt.mapping[k]) == int(ref.mapping[k]) and np.array_equal(opt.partner[k], ref.partner[k]) \
            and (not np.isfinite(ref.rms[k]) or opt.rms[k] == ref.rms[k])
        if not stays:
            continue
        same += 1
        for key in sm.PAIR_KEYS:
            if key != "flags":
                assert np.array_equal(bits(best[key][k]), bits(near[key][k])), (pair.name, key)
        assert int(best["flags"][k]) & ~sm.ASSIGNED == int(near["flags"][k]), pair.name
    k = base.pair_index("two atoms of x at one atom of y")
    assert same >= len(base.pairs()) - 1 and near["flags"][k] == sm.NO_PERMUTATION and best["flags"][k] == sm.ASSIGNED and np.isfinite(best["rms"][k])
    assert np.array_equal(best["n_permutations"], near["n_permutations"])


def test_repeated_runs_a_permuted_pair_list_and_a_split_launch_agree_bit_for_bit(dev):
    got = run(dev, "new")
    again = launch(dev, cases.batch(), cases.pair_list(), cases.PARAMS)
    order = np.random.default_rng(5).permutation(len(cases.pairs()))
    perm = launch(dev, cases.batch(), cases.pair_list()[order], cases.PARAMS)
    # a budget of three pairs' cost matrices at stride 257: four launches
    split = launch(dev, cases.batch(), cases.pair_list(), cases.PARAMS, cost_budget=3 * sm.WAVES * (257 + sm.ASSIGN_STATE_ROWS) * 257 * 4)
    one = launch(dev, cases.batch(), cases.pair_list(), cases.PARAMS, cost_budget=1)  # one pair per launch
    for k in sm.PAIR_KEYS:
        assert np.array_equal(bits(got[k]), bits(again[k])), k
        assert np.array_equal(bits(perm[k]), bits(got[k][order])), k
        assert np.array_equal(bits(split[k]), bits(got[k])) and np.array_equal(bits(one[k]), bits(got[k])), k
    assert sm.COST_BUDGET_BYTES >= sm.WAVES * (257 + sm.ASSIGN_STATE_ROWS) * 257 * 4


def test_sample_with_match_to_optimal(dev, fused_model):
    m, _ = fused_model
    counts = [4, 7, 1]

    def sample(**kw):
        torch.manual_seed(3)
        np.random.seed(3)
        return m.sample(counts, 3, seed=777, max_steps=6, lattice_system="orthorhombic", **kw)

    plain = sample()
    near = sample(match_to=plain)
    best = sample(match_to=(plain, sm.StructureMatchParams(assignment="optimal")))
    assert np.array_equal(plain.frac_x, best.frac_x) and set(best.match) == set(sm.MATCH_KEYS)
    host = (plain.frac_x, plain.lattice, plain.num_atoms, np.rint(plain.atomic_numbers))
    ref = sm.structure_match_reference_f64(host, host, sm.paired(3), sm.StructureMatchParams(assignment="optimal"))
    assert np.array_equal(best.match["flags"], ref.flags) and best.match["matched"].tolist() == [1, 1, 1]
    assert np.array_equal(best.match["n_permutations"], near.match["n_permutations"]) and np.array_equal(best.match["n_candidates"], ref.n_candidates)
    # a crystal against itself: the identity is one-to-one and wins with rms 0, whatever else was solved
    for k in ("rms", "mapping", "partner", "target"):
        assert np.array_equal(bits(np.asarray(best.match[k])), bits(np.asarray(near.match[k]))), k
    direct = sm.match_crystals(plain, plain, sm.StructureMatchParams(assignment="optimal"), device=dev)
    for k in sm.MATCH_KEYS:
        assert np.array_equal(bits(np.asarray(direct[k])), bits(np.asarray(best.match[k]))), k


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_round_trip_with_assignment_optimal(dev, tmp_path):
    """generate writes a small file; generate --match_to ... --assignment optimal matches a second run against it; screen matches
    the first file against itself with the flag: each a fresh process.  The stored keys are MATCH_KEYS, no more."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out, out2, out3 = (str(tmp_path / "out" / name) for name in ("targets.npz", "matched.npz", "again.npz"))
    common = ["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--batch", "4", "--num_atoms", "6", "--num_steps", "10", "--seed", "5",
              "--lattice_system", "orthorhombic"]
    _child(common + ["--out", out], 300)
    text = _child(["arreau_amd.screen", out, "--match_to", out, "--match_mode", "paired", "--assignment", "optimal", "--out", out2], 180)
    assert re.search(r"match rank 0: matched 5 / attempted 5 \(rate 1\); mean rms_norm ", text) and "match total: matched 5 / attempted 5" in text, text
    back = load_sample_results_from_hdf5(out2)
    assert set(back.match) == set(sm.MATCH_KEYS) and back.match["target"].tolist() == [0, 1, 2, 3, 4] and (back.match["rms"] < 1e-3).all()
    stored = {k[len("match_"):] for k in np.load(out2).files if k.startswith("match_")}
    assert stored == set(sm.MATCH_KEYS), stored
    text = _child(common + ["--match_to", out, "--stol", "0.25", "--assignment", "optimal", "--out", out3], 300)
    assert re.search(r"match rank 0: matched \d / attempted 5 \(rate [0-9.]+\); ", text) and "match total: matched " in text, text
    match = load_sample_results_from_hdf5(out3).match
    assert set(match) == set(sm.MATCH_KEYS) and match["rms"].shape == (5,) and match["partner"].shape == (30,)
    assert not (match["flags"] & sm.NO_PERMUTATION).any()  # under "optimal" every comparable crystal gets a result
    comparable = match["n_comparable"] > 0
    assert np.isfinite(match["rms"][comparable & ((match["flags"] & sm.NO_RESULT_MASK) == 0)]).all()


def test_the_two_new_argument_errors_touch_nothing(dev):
    z, pairs = device_batch(dev, cases.batch()), up(dev, cases.pair_list()[:3])
    out, scratch = empty_outputs(dev, 3, 257)
    before = {k: out[k].clone() for k in sm.PAIR_KEYS}
    cost = torch.empty(3 * sm.WAVES * (257 + sm.ASSIGN_STATE_ROWS) * 257, device=dev, dtype=torch.float32)
    EINVAL = -1  # ARREAU_EINVAL
    for assignment, d_cost in ((2, cost), (-1, cost), (1, None)):  # an assignment outside {0, 1}; OPTIMAL above the LDS bound without d_cost
        assert call_assigned(dev, z, pairs, cases.PARAMS, out, scratch, assignment, d_cost) == EINVAL, (assignment, d_cost is None)
        assert b"arreau_structure_match_assigned" in _hip.lib().arreau_last_error()
    torch.cuda.synchronize()
    for k in sm.PAIR_KEYS:
        assert torch.equal(before[k], out[k]), k
    with pytest.raises(ValueError, match="assignment"):
        sm.match(z, z, pairs, sm.StructureMatchParams(assignment="hungarian"))
    # at a stride within the LDS bound OPTIMAL needs no d_cost
    small = [k for k, p in enumerate(cases.pairs()) if 0 < atoms_of(p) <= sm.ASSIGN_LDS_ATOMS][:3]
    sub = up(dev, cases.pair_list()[small])
    out, scratch = empty_outputs(dev, 3, sm.ASSIGN_LDS_ATOMS)
    assert call_assigned(dev, z, sub, cases.PARAMS, out, scratch, 1, None) == 0
    got, want = sm.result_to_numpy(out), run(dev, "new")
    for k in ("rms", "mapping", "flags", "translation"):
        assert np.array_equal(bits(got[k]), bits(want[k][small])), k


def test_the_symbol_is_exported_everywhere():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_structure_match_assigned(" in fh.read()
    assert "arreau_structure_match_assigned" in _hip.EXPORTS
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_structure_match_assigned")
