"""Structure match on the device (arreau_structure_match, csrc/match.hip) against the float64 restatement on the guarded pairs of
tests/structure_match_cases.py, one ragged launch with X and Y the same batch: flags, counts and `matched` equal; rms, max_dist,
rms_norm and the translation (modulo 1) within the bounds derived in diffusion/structure_match.py (never from the kernel's
output); mapping and partner equal where the restatement's best candidate stands clear of the next, and the device's own choice
checked in float64 where candidates tie.  Then repeated runs, a permuted pair list, the overflow, sample(match_to=...), the two
command lines and the argument errors.  Needs an MI355X: `-m gpu`."""
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
from tests import structure_match_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("flags", "n_mappings", "n_candidates", "n_permutations", "matched")
REAL_KEYS = ("rms", "max_dist", "rms_norm", "translation")
MUST_BE_DECISIVE = ("P1: atoms permuted", "P1: common translation", "P1: lattice translations of single atoms", "P1: unimodular change of basis",
                    "P1: rigid rotation", "P1: mirror", "P1: strained 8 %", "P1: gamma + 2 degrees", "P1: displaced 0.03 A (matched)",
                    "P1: displaced 0.25 A (a permutation, not matched)", "257 atoms against a perturbed copy")
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, batch):
    frac, lattice, counts, types = batch
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return up(dev, frac.reshape(-1, 3)), up(dev, lattice), up(dev, off), up(dev, types)


def launch(dev, pair_list, params=cases.PARAMS):
    z = device_batch(dev, cases.batch())
    return sm.result_to_numpy(sm.match(z, z, pair_list, params))  # (Y is X: the same tensors)


def batch_run(dev):
    """Every pair in ONE ragged launch (cached)."""
    if "all" not in _RUN:
        _RUN["all"] = launch(dev, cases.pair_list())
    return _RUN["all"]


def mod1(d):
    return np.abs(d - np.rint(d))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def atoms_of(pair):
    return cases.crystals()[pair.x].n


def test_integers_equal_the_f64_restatement(dev):
    got, ref = batch_run(dev), cases.reference()
    for k in INT_KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), (k, got[k], getattr(ref, k))
    for k, pair in enumerate(cases.pairs()):
        if int(ref.flags[k]) & sm.NO_RESULT_MASK:
            assert np.isposinf(got["rms"][k]) and np.isposinf(got["rms_norm"][k]) and np.isposinf(got["max_dist"][k]), pair.name
            assert got["mapping"][k] == -1 and (got["partner"][k] == -1).all() and not got["translation"][k].any(), pair.name
        else:
            n = atoms_of(pair)
            assert sorted(got["partner"][k, :n].tolist()) == list(range(n)) and (got["partner"][k, n:] == -1).all(), pair.name
    assert got["partner"].shape == (len(cases.pairs()), 257)


def test_reals_stay_within_the_derived_bounds(dev):
    got, ref = batch_run(dev), cases.reference()
    worst = {}
    for k, pair in enumerate(cases.pairs()):
        if int(ref.flags[k]) & sm.NO_RESULT_MASK:
            continue
        bound = cases.bounds(ref, k, atoms_of(pair))
        err = {"rms": abs(float(got["rms"][k]) - ref.rms[k]), "max_dist": abs(float(got["max_dist"][k]) - ref.max_dist[k]),
               "rms_norm": abs(float(got["rms_norm"][k]) - ref.rms_norm[k])}
        clear = decisive(ref, k, bound["rms"])
        if clear:  # (where candidates tie the device may hold another of them: its translation is checked in the test below)
            err["translation"] = float(mod1(got["translation"][k] - ref.translation[k]).max())
        print(f"{pair.name}: " + ", ".join(f"{q} {err[q]:.3e} (bound {bound[q]:.3e})" for q in err))
        for q in err:
            worst[q] = max(worst.get(q, 0.0), err[q] / bound[q])
            assert err[q] <= bound[q], (pair.name, q, err[q], bound[q])
        if pair.exact:  # the expected rms is 0: the restatement's own value is the rounding of the inputs
            assert float(got["rms"][k]) <= bound["rms"] + cases.input_rounding(pair), pair.name
    print("largest deviation / bound:", worst)
    assert set(worst) == set(REAL_KEYS)


def decisive(ref, k, rms_bound):
    """The restatement's best and second-best rms differ by more than four times the bound (or there is no second)."""
    sv = ref.survivors[k]
    return len(sv) == 1 or sv[1][0] - sv[0][0] > 4.0 * rms_bound


def test_the_decisive_cases_are_decisive():
    """On the CPU: which pairs the argmin test compares exactly."""
    ref = cases.reference()
    for name in MUST_BE_DECISIVE:
        k = cases.pair_index(name)
        assert decisive(ref, k, cases.bounds(ref, k, atoms_of(cases.pairs()[k]))["rms"]), name
        assert cases.pairs()[k].decisive, name


def test_argmin_mapping_and_partner(dev):
    got, ref = batch_run(dev), cases.reference()
    Z = cases.crystals()
    exact = tied = 0
    for k, pair in enumerate(cases.pairs()):
        if int(ref.flags[k]) & sm.NO_RESULT_MASK:
            continue
        n, bound = atoms_of(pair), cases.bounds(ref, k, atoms_of(pair))
        if decisive(ref, k, bound["rms"]):
            assert got["mapping"][k] == ref.mapping[k] and np.array_equal(got["partner"][k, :n], ref.partner[k, :n]), pair.name
            exact += 1
            continue
        # candidates tie: the device's own mapping, translation and partner in float64 reproduce its rms, and that is the minimum
        tied += 1
        x, y = Z[pair.x], Z[pair.y]
        A, B = x.lattice.astype(np.float64), y.lattice.astype(np.float64)
        W = ss.decode_rotation(int(got["mapping"][k]))
        assert abs(round(np.linalg.det(W))) == 1
        Gp = W.T.astype(np.float64) @ (B @ B.T) @ W.astype(np.float64)
        c = sm.evaluate_candidate(ss._wrap01(x.frac.astype(np.float64)), ss._wrap01(y.frac.astype(np.float64)), x.types, y.types, A @ A.T, Gp, W,
                                  t=got["translation"][k].astype(np.float64), partner=got["partner"][k, :n])
        assert np.array_equal(y.types[got["partner"][k, :n]], x.types), pair.name
        # (the device's translation carries its own bound on top of the distance's)
        slack = bound["rms"] + 3.0 * float(ref.l1[k]) * bound["translation"]
        print(f"{pair.name}: device rms {got['rms'][k]:.6e}, its choice in float64 {c.rms:.6e}, the restatement's minimum {ref.rms[k]:.6e} (bound {slack:.3e})")
        assert abs(c.rms - float(got["rms"][k])) <= slack and abs(float(got["rms"][k]) - ref.rms[k]) <= bound["rms"], pair.name
        assert abs(c.max_dist - float(got["max_dist"][k])) <= bound["max_dist"] + 3.0 * float(ref.l1[k]) * bound["translation"], pair.name
    assert exact >= len(MUST_BE_DECISIVE) and tied >= 2  # (rock salt and diamond tie)


def test_repeated_runs_and_a_permuted_pair_list_agree_bit_for_bit(dev):
    got = batch_run(dev)
    again = launch(dev, cases.pair_list())
    for k in sm.PAIR_KEYS:
        assert np.array_equal(bits(got[k]), bits(again[k])), k
    order = np.random.default_rng(5).permutation(len(cases.pairs()))
    perm = launch(dev, cases.pair_list()[order])
    for k in sm.PAIR_KEYS:
        assert np.array_equal(bits(perm[k]), bits(got[k][order])), k


def test_overflow_keeps_the_first_mappings(dev):
    got, ref = launch(dev, cases.overflow_pair_list(), cases.OVERFLOW_PARAMS), cases.overflow_reference()
    for k in INT_KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), k
    assert got["flags"][0] == sm.OVERFLOW and got["n_mappings"][0] == 48 and got["n_candidates"][0] == 8
    bound = cases.bounds(ref, 0, 8)
    assert abs(float(got["rms"][0]) - ref.rms[0]) <= bound["rms"] and abs(float(got["rms_norm"][0]) - ref.rms_norm[0]) <= bound["rms_norm"]
    W = ss.decode_rotation(int(got["mapping"][0]))
    assert int(got["mapping"][0]) in {code for _, code, _ in ref.survivors[0]} and abs(round(np.linalg.det(W))) == 1


def test_sample_with_match_to(dev, fused_model):
    m, _ = fused_model
    counts = [4, 7, 1]

    def run(**kw):
        torch.manual_seed(3)
        np.random.seed(3)
        # (orthorhombic: the sampler's default cells, monoclinic angles in degrees read as radians, can come out without volume)
        r = m.sample(counts, 3, seed=777, max_steps=6, lattice_system="orthorhombic", **kw)
        return r, torch.random.get_rng_state(), np.random.uniform()

    plain, rng0, after0 = run()
    assert plain.match is None
    host = (plain.frac_x, plain.lattice, plain.num_atoms, np.rint(plain.atomic_numbers))
    ref = sm.structure_match_reference_f64(host, host, sm.paired(3))
    assert not ref.flags.any() and ref.matched.tolist() == [1, 1, 1], ref.flags  # the restatement on the returned arrays
    outs = [run(match_to=plain), run(match_to=(plain, sm.StructureMatchParams(stol=0.1), "any")), run(match_to=None)]
    for r, rng, after in outs:
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and np.array_equal(plain.num_atoms, r.num_atoms)
        assert torch.equal(rng0, rng) and after0 == after
        assert r.metrics is None and r.symmetry is None and r.reduced is None and r.symmetrized is None
    assert outs[2][0].match is None
    first = np.concatenate([[0], np.cumsum(counts)])
    for (r, _, _), mode in zip(outs[:2], ("paired", "any")):
        match = r.match
        assert set(match) == set(sm.MATCH_KEYS) and match["partner"].shape == (12,) and match["translation"].shape == (3, 3)
        assert np.array_equal(match["flags"], ref.flags) and np.array_equal(match["n_mappings"], ref.n_mappings), (mode, match["flags"])
        assert not match["flags"].any() and match["matched"].tolist() == [1, 1, 1], (mode, match["flags"])
        assert sm.match_rate(sm.stats_of(match)) == 1.0
        for b, n in enumerate(counts):
            L = plain.lattice[b]
            bound = sm.distance_bound(n, sm.longest_edge(L, 0.2), 0.0, 0.0)
            print(f"{mode}, crystal {b}: rms {match['rms'][b]:.3e} A (bound {bound:.3e}), target {match['target'][b]}")
            assert 0.0 <= match["rms"][b] <= bound and 0.0 <= match["max_dist"][b] <= bound
            part = match["partner"][first[b]:first[b + 1]]
            assert sorted(part.tolist()) == list(range(n))
            target = int(match["target"][b])
            t0 = int(np.concatenate([[0], np.cumsum(plain.num_atoms)])[target])
            assert np.array_equal(plain.atomic_numbers[t0 + part], plain.atomic_numbers[first[b]:first[b + 1]])
        if mode == "paired":
            assert match["target"].tolist() == [0, 1, 2] and match["n_comparable"].tolist() == [1, 1, 1]
    # consistent with the engine-free entry point on the returned arrays
    direct = sm.match_crystals(plain, plain, device=dev)
    assert direct["mode"] == "paired"
    for k in sm.MATCH_KEYS:
        assert np.array_equal(bits(np.asarray(direct[k])), bits(np.asarray(outs[0][0].match[k]))), k
    with pytest.raises(ValueError, match="match_to"):
        m.sample(counts, 3, seed=777, max_steps=1, match_to="targets.npz")
    with pytest.raises(ValueError, match="paired match needs as many targets"):
        m.sample([4, 7], 2, seed=777, max_steps=1, match_to=(plain, sm.StructureMatchParams(), "paired"))


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_round_trip_through_a_file(dev, tmp_path):
    """generate writes a small file; screen --match_to matches it against itself, paired, after the reduction and symmetrization of
    both; generate --match_to matches a second run against it: each a fresh process."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out, out2, out3 = (str(tmp_path / "out" / name) for name in ("targets.npz", "matched.npz", "again.npz"))
    common = ["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--batch", "4", "--num_atoms", "6", "--num_steps", "10", "--seed", "5",
              "--lattice_system", "orthorhombic"]
    _child(common + ["--out", out], 300)
    targets = load_sample_results_from_hdf5(out)
    assert targets.match is None and len(targets.num_atoms) == 5
    text = _child(["arreau_amd.screen", out, "--match_to", out, "--match_mode", "paired", "--reduce_cell", "--symmetrize", "--symprec", "0.001",
                   "--out", out2], 180)
    assert re.search(r"match rank 0: matched 5 / attempted 5 \(rate 1\); mean rms_norm ", text) and "match total: matched 5 / attempted 5" in text, text
    back = load_sample_results_from_hdf5(out2)
    assert set(back.match) == set(sm.MATCH_KEYS) and back.match["target"].tolist() == [0, 1, 2, 3, 4] and (back.match["rms"] < 1e-3).all()
    assert back.match["partner"].shape == (int(back.num_atoms.sum()),) and back.symmetrized is not None
    text = _child(common + ["--match_to", out, "--stol", "0.25", "--out", out3], 300)
    assert re.search(r"match rank 0: matched \d / attempted 5 \(rate [0-9.]+\); ", text) and "match total: matched " in text, text
    res = load_sample_results_from_hdf5(out3)
    match = res.match
    assert set(match) == set(sm.MATCH_KEYS) and match["rms"].shape == (5,) and match["partner"].shape == (30,)
    want = sm.best_per_x(sm.same_composition(res, targets), {"rms_norm": np.full(25, np.inf)}, 5)["n_comparable"]
    assert np.array_equal(match["n_comparable"], want)
    assert (match["flags"][want == 0] == sm.DIFFERENT).all() and (match["n_comparable"] >= 0).all()
    ok = match["matched"] == 1
    assert (match["rms_norm"][ok] <= 0.25).all() and (match["target"][ok] >= 0).all() and np.isinf(match["rms"][match["target"] < 0]).all()


def test_argument_errors_touch_nothing(dev):
    z = device_batch(dev, cases.batch())
    with pytest.raises(ValueError, match=r"match \(x\): types"):
        sm.match((z[0], z[1], z[2], z[3].to(torch.int64)), z, cases.pair_list())
    with pytest.raises(ValueError, match="pairs"):
        sm.match(z, z, up(dev, cases.pair_list().astype(np.int64)))
    pairs = up(dev, cases.pair_list()[:3])
    out = sm.match(z, z, pairs, cases.PARAMS)
    assert sm.result_to_numpy(sm.match(z, z, cases.pair_list()[:0]))["rms"].shape == (0,)  # P = 0: a no-op
    B, N, stride = int(z[1].shape[0]), int(z[0].shape[0]), int(out["partner"].shape[1])
    scratch = torch.empty((3, sm.WAVES, stride), device=dev, dtype=torch.int32)
    good = lambda: _hip.StructureMatchResultC(*[_hip.ptr(out[k]).value for k in sm.PAIR_KEYS], _hip.ptr(scratch).value, stride)
    before = {k: out[k].clone() for k in sm.PAIR_KEYS}
    par = lambda **kw: _hip.StructureMatchParamsC(*[kw.get(k, v) for k, v in (("ltol", 0.2), ("angle_tol", 0.087), ("stol", 0.3), ("max_mappings", 192))])
    side = [_hip.ptr(z[0]), _hip.ptr(z[3]), _hip.ptr(z[1]), _hip.ptr(z[2]), B, N]
    call = _hip.lib().arreau_structure_match
    EINVAL = -1  # ARREAU_EINVAL
    no_partner, no_scratch, no_rms = good(), good(), good()
    no_partner.partner, no_scratch.scratch, no_rms.rms = None, None, None
    tries = [(side, side, _hip.ptr(pairs), 3, None, good()), (side, side, _hip.ptr(pairs), 3, par(), None),
             (side[:4] + [-1, N], side, _hip.ptr(pairs), 3, par(), good()), (side, side[:4] + [B, -1], _hip.ptr(pairs), 3, par(), good()),
             (side, side, _hip.ptr(pairs), -3, par(), good()), (side, side, None, 3, par(), good()),
             ([None] + side[1:], side, _hip.ptr(pairs), 3, par(), good()), (side, side[:3] + [None] + side[4:], _hip.ptr(pairs), 3, par(), good()),
             (side, side, _hip.ptr(pairs), 3, par(), no_partner), (side, side, _hip.ptr(pairs), 3, par(), no_scratch),
             (side, side, _hip.ptr(pairs), 3, par(), no_rms)]
    for bad in (dict(ltol=0.0), dict(ltol=float("nan")), dict(angle_tol=-1.0), dict(angle_tol=float("inf")), dict(stol=0.0),
                dict(max_mappings=0), dict(max_mappings=4097)):
        tries.append((side, side, _hip.ptr(pairs), 3, par(**bad), good()))
    for x, y, pr, P, params, res in tries:
        rc = call(*x, *y, pr, P, ctypes.byref(params) if params is not None else None, ctypes.byref(res) if res is not None else None,
                  _hip.stream_ptr(dev))
        assert rc == EINVAL, (P, params, res)
        assert b"arreau_structure_match" in _hip.lib().arreau_last_error()
    torch.cuda.synchronize()
    for k in sm.PAIR_KEYS:
        assert torch.equal(before[k], out[k]), k


def test_the_symbol_is_exported_everywhere():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_structure_match(" in fh.read()
    assert "arreau_structure_match" in _hip.EXPORTS
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_structure_match")
