"""Symmetrization on the device (arreau_crystal_symmetrize, csrc/symmetrize.hip) against the float64 restatement on the guarded
batch of tests/symmetrize_cases.py, one ragged launch: flags, partners, orbits, sizes and site orders equal; positions and refined
translations (modulo 1), lengths and angles within the bounds derived in diffusion/symmetrize.py (never from the kernel's
output); displacements within the search's residual bound.  Then the device output under its own refined operations, the copies,
permutation of the batch, repeated runs, sample(symmetrize=...), the two command lines and the argument errors.  Needs an
MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import symmetrize as sz
from arreau_amd.diffusion import symmetry_search as ss
from tests import symmetrize_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("orbit", "orbit_size", "site_order", "partner")
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, batch):
    frac, lattice, counts, types = batch
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return up(dev, frac.reshape(-1, 3)), up(dev, lattice), up(dev, off), up(dev, types)


def launch(dev, batch, params=cases.PARAMS):
    return sz.result_to_numpy(sz.symmetrize(*device_batch(dev, batch), params))


def batch_run(dev):
    """Every case in ONE ragged launch (cached)."""
    if "all" not in _RUN:
        _RUN["all"] = launch(dev, cases.batch())
    return _RUN["all"]


def rows(b):
    first = cases.first_atoms()
    return slice(int(first[b]), int(first[b + 1]))


def mod1(d):
    return np.abs(d - np.rint(d))


def bits(a):
    """The words of an array; every NaN as one word (a NaN's payload is not part of any rule)."""
    a = np.ascontiguousarray(a)
    return np.where(np.isnan(a), np.int32(0x7fc00000), a.view(np.int32)) if a.dtype == np.float32 else a


def test_kernel_matches_the_f64_restatement(dev):
    got, ref, found = batch_run(dev), cases.reference(), cases.search_reference()
    assert np.array_equal(got["found"]["n_ops"], found.n_ops) and np.array_equal(got["found"]["flags"], found.flags)
    assert np.array_equal(got["flags"], ref.flags) and np.array_equal(got["n_orbits"], ref.n_orbits)
    for k in INT_KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), k
    worst = {}
    for b, case in enumerate(cases.cases()):
        L = case.lattice.astype(np.float64)
        if case.flags & sz.NONFINITE:
            continue
        K = int(found.n_ops[b]) if not case.flags else 0
        bound = {"position": sz.position_bound(case.n, max(K, 1), float(ref.D[b])), "length": sz.length_bound(L, cases.SYMPREC),
                 "angle": sz.angle_bound(L, cases.SYMPREC, ref.angles[b]), "displacement": ss.residual_bound(L)}
        err = {"position": max(float(mod1(got["frac_out"][rows(b)] - ref.frac_out[rows(b)]).max()) if case.n else 0.0,
                               float(mod1(got["ops_translation"][b] - ref.ops_translation[b]).max())),
               "length": float(np.abs(got["lengths"][b] - ref.lengths[b]).max()),
               "angle": float(np.abs(got["angles"][b] - ref.angles[b]).max()),
               "displacement": max(abs(float(got["max_displacement"][b]) - ref.max_displacement[b]),
                                   abs(float(got["rms_displacement"][b]) - ref.rms_displacement[b]))}
        print(f"{case.name}: " + ", ".join(f"{k} {err[k]:.3e} (bound {bound[k]:.3e})" for k in err))
        for k in err:
            worst[k] = max(worst.get(k, 0.0), err[k] / bound[k])
            assert err[k] <= bound[k], (case.name, k, err[k], bound[k])
        assert float(np.abs(got["ops_shift"][b] - ref.ops_shift[b]).max()) <= bound["position"], case.name
        # the rebuilt cell: the device's own lengths and angles in the sampler's orientation, within float32 of the float64 form
        want = sz.lattice_from_params_f64(got["lengths"][b].astype(np.float64), got["angles"][b].astype(np.float64))
        # (cosines and sines of the angles, each within 2 u; their quotient, the arc cosine and the products: some 18 u of a length
        # for the angles of this batch, 71 to 120 degrees)
        assert np.abs(got["lattice"][b] - want).max() <= 64 * sz.U * float(got["lengths"][b].max()), case.name
    print("largest deviation / bound:", worst)


def test_device_output_is_symmetric_under_its_own_operations(dev):
    """Residuals under the refined operations within the derived bound, and at least 100 times below the input's under the found
    ones: a kernel that copies its input fails."""
    got, ref, found = batch_run(dev), cases.reference(), cases.search_reference()
    for b, case in enumerate(cases.cases()):
        if case.flags or case.n_ops == 1 or case.n == 1:
            continue
        K = case.n_ops
        stored = [(ss.decode_rotation(int(c)), t.astype(np.float64)) for c, t in zip(got["found"]["ops_rotation"][b, :K], got["found"]["ops_translation"][b, :K])]
        refined = [(W, t.astype(np.float64)) for (W, _), t in zip(stored, got["ops_translation"][b, :K])]
        L = case.lattice.astype(np.float64)
        before = float(ss.operation_residuals(case.frac, L, case.types, stored).max())
        after = float(ss.operation_residuals(got["frac_out"][rows(b)], L, case.types, refined).max())
        # an image W x' + t' carries the position bound on x' (three terms) and on t'; its partner the bound once more; in A
        bound = 5.0 * sz.position_bound(case.n, K, float(ref.D[b])) * float(np.abs(L).sum(axis=0).max())
        print(f"{case.name}: residual before {before:.3e} A, after {after:.3e} A (bound {bound:.3e})")
        assert after <= bound and 100.0 * after <= before, case.name


def test_flagged_and_identity_only_crystals_are_copied_bit_for_bit(dev):
    got = batch_run(dev)
    group = list(enumerate(cases.cases()))
    extra = cases.not_a_permutation()
    alone = launch(dev, (extra[0], extra[1][None], [4], extra[2]))
    assert int(alone["flags"][0]) == sz.NOT_A_PERMUTATION and int(alone["found"]["n_ops"][0]) == 2
    checks = [(got, rows(b), b, c.frac, c.flags, c.name) for b, c in group if c.flags or c.n_ops == 1]
    checks.append((alone, slice(0, 4), 0, extra[0], sz.NOT_A_PERMUTATION, "no permutation"))
    assert len(checks) == 6
    for out, sl, b, frac, flags, name in checks:
        with np.errstate(all="ignore"):
            w = frac - np.floor(frac)
            w[w >= 1] = 0
        assert int(out["flags"][b]) == flags, name
        assert np.array_equal(bits(out["frac_out"][sl]), bits(w)), name
        n = len(frac)
        assert np.array_equal(out["orbit"][sl], np.arange(n)) and int(out["n_orbits"][b]) == n, name
        assert (out["orbit_size"][sl] == 1).all() and (out["site_order"][sl] == 1).all(), name
        assert out["max_displacement"][b] == 0 and out["rms_displacement"][b] == 0, name
        if flags:
            assert not out["ops_translation"][b].any() and not out["ops_shift"][b].any() and (out["partner"][:, sl] == -1).all(), name


def test_permuting_the_batch_permutes_the_results_and_two_runs_agree(dev):
    got = batch_run(dev)
    again = launch(dev, cases.batch())
    for k in sz.RESULT_KEYS:
        assert np.array_equal(bits(got[k]), bits(again[k])), k
    group = list(cases.cases())
    order = [5, 11, 0, 9, 3, 8, 2, 7, 10, 4, 6, 1]
    assert sorted(order) == list(range(len(group)))
    perm = launch(dev, cases.batch_of([group[b] for b in order]))
    first = np.concatenate([[0], np.cumsum([group[b].n for b in order])])
    for at, b in enumerate(order):
        sl = slice(int(first[at]), int(first[at + 1]))
        for k in ("lattice", "lengths", "angles", "n_orbits", "max_displacement", "rms_displacement", "ops_translation", "ops_shift", "flags"):
            assert np.array_equal(bits(perm[k][at]), bits(got[k][b])), (group[b].name, k)
        for k in ("frac_out", "orbit", "orbit_size", "site_order"):
            assert np.array_equal(bits(perm[k][sl]), bits(got[k][rows(b)])), (group[b].name, k)
        assert np.array_equal(perm["partner"][:, sl], got["partner"][:, rows(b)]), group[b].name


def test_sample_with_symmetrize(dev, fused_model):
    m, _ = fused_model
    out = []
    for kw in ({}, dict(symmetrize=True), dict(symmetrize=None), dict(symmetrize=True, find_symmetry=True, screen=True, reduce_cell=True)):
        torch.manual_seed(3)
        np.random.seed(3)
        r = m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)
        out.append((r, torch.random.get_rng_state(), np.random.uniform()))
    plain = out[0][0]
    for r, rng, after in out[1:]:
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and torch.equal(out[0][1], rng) and out[0][2] == after
    a, none, every = out[1][0], out[2][0], out[3][0]
    assert plain.symmetrized is None and none.symmetrized is None and a.symmetry is None and a.reduced is None and a.metrics is None
    sym = a.symmetrized
    assert set(sym) == set(sz.SYMMETRIZED_KEYS) and sym["frac_x"].shape == (12, 3) and sym["ops_translation"].shape == (3, 192, 3)
    assert sym["lattice"].shape == (3, 3, 3) and sym["orbit"].shape == (12,) and sym["n_orbits"].shape == (3,)
    # consistent with the engine-free entry point on the returned arrays
    direct = sz.symmetrize_sample_result(plain, sz.SymmetrizeParams(), dev)
    for k in sz.SYMMETRIZED_KEYS:
        assert np.array_equal(sym[k], every.symmetrized[k], equal_nan=True), k  # the shared search changes nothing
        # (the entry point takes the atomic numbers as species ids, the sampler its class indices: the same partition of the atoms,
        # but a tie between two equally rare species may start the search's translations from another atom)
        if sym[k].dtype.kind == "i":
            assert np.array_equal(sym[k], direct[k]), k
        else:
            d = np.abs(sym[k].astype(np.float64) - direct[k])
            assert np.minimum(d, np.abs(1.0 - d)).max() <= 1e-5 if k in ("frac_x", "ops_translation") else d.max() <= 1e-5, k
    assert every.symmetry is not None and every.reduced is not None and every.metrics is not None
    assert np.array_equal(every.symmetry["n_ops"], direct["found"]["n_ops"])
    assert (sym["site_order"] >= 1).all() and (sym["orbit_size"] >= 1).all() and (sym["n_orbits"] <= [4, 7, 1]).all()


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_round_trip_through_a_file(dev, tmp_path):
    """generate --symmetrize on crystals sampled with P4/mmm symmetry (one general orbit of 16), then screen --symmetrize --out on that
    file and the other instruments on the symmetrized file: each a fresh process."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    ops = tmp_path / "p4mmm.txt"
    ops.write_text("-y,x,z\n-x,y,-z\n-x,-y,-z\n")
    out, out2 = str(tmp_path / "out" / "crystals.npz"), str(tmp_path / "out" / "symmetrized.npz")
    text = _child(["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--batch", "4", "--num_steps", "10", "--symops", str(ops),
                   "--lattice_system", "tetragonal", "--orbits", "1", "--seed", "5", "--symmetrize", "--symprec", "0.001", "--out", out], 300)
    assert re.search(r"symmetrize rank 0: symmetrized \d / attempted 5; orbits ", text) and "symmetrize total: " in text, text
    res = load_sample_results_from_hdf5(out)
    sym = res.symmetrized
    assert set(sym) == set(sz.SYMMETRIZED_KEYS) and sym["frac_x"].shape == res.frac_x.shape and sym["n_orbits"].shape == (5,)
    ok = sym["flags"] == 0
    assert ok.any() and (sym["site_order"].reshape(5, 16)[ok] * sym["orbit_size"].reshape(5, 16)[ok] >= 16).all()
    assert (sym["max_displacement"][ok] < 0.001).all()
    text = _child(["arreau_amd.screen", out, "--symmetrize", "--symprec", "0.001", "--out", out2], 120)
    assert "symmetrize total: symmetrized " in text and "wrote" in text, text
    back = load_sample_results_from_hdf5(out2)
    assert mod1(back.frac_x - sym["frac_x"]).max() <= 1e-5 and np.array_equal(back.num_atoms, res.num_atoms)
    assert np.abs(back.lattice - sym["lattice"]).max() <= 1e-4 and np.array_equal(back.symmetrized["orbit"], sym["orbit"])
    assert np.array_equal(back.atomic_numbers, res.atomic_numbers) and np.array_equal(back.frac_x, back.symmetrized["frac_x"])
    text = _child(["arreau_amd.screen", out2, "--find_symmetry", "--symprec", "0.001"], 120)  # the other instruments run on it
    assert "symmetry total: classified " in text, text


def test_argument_errors_touch_nothing(dev):
    frac, lattice, off, types = device_batch(dev, cases.batch_of(list(cases.cases())[:1]))
    with pytest.raises(ValueError, match="symmetrize: types"):
        sz.symmetrize(frac, lattice, off, types.to(torch.int64))
    found = ss.find_symmetry(frac, lattice, off, types, cases.PARAMS.search())
    out = sz.symmetrize(frac, lattice, off, types, cases.PARAMS, found)
    s = _hip.SymmetryResultC(*[_hip.ptr(found[k]).value for k in ss.SYM_KEYS[:-1]])
    r = _hip.SymmetrizeResultC(*[_hip.ptr(out[k]).value for k in sz.RESULT_KEYS])
    before = {k: out[k].clone() for k in sz.RESULT_KEYS}
    args = (_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(off))
    call = _hip.lib().arreau_crystal_symmetrize
    EINVAL = -1  # ARREAU_EINVAL
    for B, N, fnd, max_ops, res in ((1, 8, None, 384, ctypes.byref(r)), (1, 8, ctypes.byref(s), 384, None), (-1, 8, ctypes.byref(s), 384, ctypes.byref(r)),
                                    (1, -8, ctypes.byref(s), 384, ctypes.byref(r)), (1, 8, ctypes.byref(s), 0, ctypes.byref(r)),
                                    (1, 8, ctypes.byref(s), 4097, ctypes.byref(r)), (1, 8, ctypes.byref(_hip.SymmetryResultC()), 384, ctypes.byref(r)),
                                    (1, 8, ctypes.byref(s), 384, ctypes.byref(_hip.SymmetrizeResultC()))):
        assert call(*args, B, N, fnd, max_ops, res, _hip.stream_ptr(dev)) == EINVAL
        assert b"arreau_crystal_symmetrize" in _hip.lib().arreau_last_error()
    assert call(None, _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(off), 1, 8, ctypes.byref(s), 384, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    torch.cuda.synchronize()
    for k in sz.RESULT_KEYS:
        assert torch.equal(before[k], out[k]), k


def test_the_symbol_is_exported_everywhere():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_symmetrize(" in fh.read()
    assert "arreau_crystal_symmetrize" in _hip.EXPORTS
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_symmetrize")
