"""The conventional-cell launch on the device (arreau_crystal_conventional, csrc/conventional.hip) against the float64 restatement,
on the ragged batch of 67 disguised crystals of tests/conventional_cell_cases.py: the chain reduce -> search -> conventional runs
on the device; the restatement restates the last two launches on the reduced batch the device's reduction handed on (which of
several equally short vectors a reduction picks is decided by float32 rounding, so the restatement of the reduction cannot be asked
to pick alike: cell_reduction.py).  Transform, centring, Bravais lattice, counts, sources, species and flags equal on every guarded
crystal; cells, lengths, angles and positions within the bounds derived in diffusion/conventional_cell.py (never from the kernel's
output).  Then batch order and size, repeated runs, the copies, sample(conventional_cell=...), the two command lines, the argument
errors and the export.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import conventional_cell as cc
from arreau_amd.diffusion import symmetry_search as ss
from tests import conventional_cell_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("transform", "centring", "bravais", "n_points", "num_atoms", "flags")
BIT_KEYS = ("lattice", "lengths", "angles") + INT_KEYS
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, batch):
    frac, lattice, counts, types = batch
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return up(dev, frac.reshape(-1, 3)), up(dev, lattice), up(dev, off), up(dev, types.astype(np.int32))


def launch(dev, batch, params=cases.PARAMS):
    """The chain on the device: (the numpy dict of the conventional launch, the reduced batch it read as numpy arrays, the numpy
    dict of the search on that batch)."""
    out = cc.conventional_cell(*device_batch(dev, batch), params)
    f, L, off, t = cc.reduced_batch(out["reduced"])
    red = (f.cpu().numpy(), L.cpu().numpy(), np.diff(off.cpu().numpy()).tolist(), t.cpu().numpy().astype(np.int64))
    return cc.result_to_numpy(out), red, ss.result_to_numpy(out["found"])


def batch_run(dev):
    """The 67 crystals in ONE ragged chain of launches, and the restatement of the search and the conventional stage on the reduced
    batch the device produced (cached)."""
    if "all" not in _RUN:
        names, items, batch = cases.gpu_batch()
        got, red, found = launch(dev, batch)
        ref_found = ss.symmetry_reference_f64(*red, cases.PARAMS.search(), details=True)
        _RUN["all"] = (got, red, found, ref_found, cc.conventional_stage_f64(*red, ref_found))
    return _RUN["all"]


def mod1(d):
    return np.abs(d - np.rint(d))


def bits(a):
    a = np.ascontiguousarray(a)
    return np.where(np.isnan(a), np.int32(0x7fc00000), a.view(np.int32)) if a.dtype == np.float32 else a


def atom_rows(num_atoms, b):
    first = np.concatenate([[0], np.cumsum(num_atoms)])
    return slice(int(first[b]), int(first[b + 1]))


def test_the_batch_is_what_the_issue_asks_for():
    names, items, batch = cases.gpu_batch()
    counts = batch[2]
    assert len(names) == 67 and 1 in counts and max(counts) >= 48 and len(set(counts)) > 3
    assert {n for n, _, _ in names} == {c.name for c in cases.CASES}


def test_kernel_matches_the_f64_restatement(dev):
    names, items, _ = cases.gpu_batch()
    got, red, found, ref_found, ref = batch_run(dev)
    guarded = [b for b in range(67) if cc.guarded(ref, b) and cc.search_guarded(ref_found, b, cases.SYMPREC)]
    print(f"guarded {len(guarded)} / 67")
    assert 10 * (67 - len(guarded)) <= 67  # at most one in ten is left out as unguarded
    worst = {}
    for b in guarded:
        name = names[b][0]
        assert int(found["n_ops"][b]) == int(ref_found.n_ops[b]) and int(found["point_group"][b]) == int(ref_found.point_group[b]), name
        for k in INT_KEYS:
            assert np.array_equal(got[k][b], getattr(ref, k)[b]), (name, k, got[k][b], getattr(ref, k)[b])
        sl = atom_rows(ref.num_atoms, b)
        assert np.array_equal(got["source"][sl], ref.source[sl]) and np.array_equal(got["types"][sl], ref.types[sl]), name
        case = cases.BY_NAME[name]
        if not int(got["reduce_flags"][b]):  # (a disguise the reduction flags hands on the cell as given: cell_reduction.py)
            assert cc.pearson_symbol(got["bravais"][b], got["num_atoms"][b]) == case.pearson, (name, names[b])
            assert cc.CENTRING_NAMES[got["centring"][b]] == (case.expect_centring or case.centring), name
        P, L = ref.transform[b].astype(np.int64), red[1][b].astype(np.float64)
        bound = {"lattice": cc.lattice_bound(P, L), "length": cc.length_bound(P, L), "angle": cc.angle_bound(P, L, ref.angles[b]),
                 "position": cc.position_bound(P)}
        err = {"lattice": float(np.abs(got["lattice"][b] - ref.lattice[b]).max()), "length": float(np.abs(got["lengths"][b] - ref.lengths[b]).max()),
               "angle": float(np.abs(got["angles"][b] - ref.angles[b]).max()),
               "position": float(mod1(got["frac_x"][sl] - ref.frac_x[sl]).max())}
        print(f"{name}: " + ", ".join(f"{k} {err[k]:.3e} (bound {bound[k]:.3e})" for k in err))
        for k in err:
            worst[k] = max(worst.get(k, 0.0), err[k] / bound[k])
            assert err[k] <= bound[k], (name, k, err[k], bound[k])
    print("largest deviation / bound:", worst)
    # the unused slots of the wide per-atom arrays
    wide = 4 * np.concatenate([[0], np.cumsum(red[2])])
    raw = cc.conventional_stage(*device_batch(dev, (red[0], red[1], red[2], red[3])),
                                ss.find_symmetry(*device_batch(dev, (red[0], red[1], red[2], red[3])), cases.PARAMS.search()))
    src, typ, frc = raw["source"].cpu().numpy(), raw["types_out"].cpu().numpy(), raw["frac_out"].cpu().numpy()
    for b in range(67):
        tail = slice(int(wide[b]) + int(got["num_atoms"][b]), int(wide[b + 1]))
        assert (src[tail] == -1).all() and (typ[tail] == -1).all() and not frc[tail].any(), names[b]


def test_results_do_not_depend_on_batch_order_or_size_and_two_runs_agree(dev):
    names, items, batch = cases.gpu_batch()
    got = batch_run(dev)[0]
    again = launch(dev, batch)[0]
    for k in BIT_KEYS + ("frac_x", "types", "source"):
        assert np.array_equal(bits(got[k]), bits(again[k])), k
    order = list(range(66, -1, -1))
    perm = launch(dev, cases.ragged([items[b] for b in order]))[0]
    for at, b in enumerate(order):
        for k in BIT_KEYS:
            assert np.array_equal(bits(perm[k][at]), bits(got[k][b])), (names[b], k)
        for k in ("frac_x", "types", "source"):
            assert np.array_equal(bits(perm[k][atom_rows(perm["num_atoms"], at)]), bits(got[k][atom_rows(got["num_atoms"], b)])), (names[b], k)
    largest = [n for n, _, _ in names].index(cases.LARGEST)
    one_atom = batch[2].index(1)
    for b in (largest, one_atom, 12):  # one crystal alone
        alone = launch(dev, cases.ragged([items[b]]))[0]
        for k in BIT_KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(got[k][b])), (names[b], k)
        for k in ("frac_x", "types", "source"):
            assert np.array_equal(bits(alone[k]), bits(got[k][atom_rows(got["num_atoms"], b)])), (names[b], k)
    assert int(got["num_atoms"][largest]) == 192 and cc.pearson_symbol(got["bravais"][largest], 192) == "cF192"


def test_flagged_crystals_are_copied_through(dev):
    for name, (f, L, t), params, flag in cases.flagged_items():
        got, red, found = launch(dev, (f, L[None], [len(f)], t), params)
        assert int(got["flags"][0]) == flag, (name, cc.describe(got["flags"][0]))
        assert np.array_equal(got["transform"][0], np.eye(3)) and int(got["bravais"][0]) == -1 and int(got["n_points"][0]) == 1, name
        assert int(got["num_atoms"][0]) == len(f) and np.array_equal(got["source"], np.arange(len(f))), name
        assert np.array_equal(bits(got["frac_x"]), bits(red[0])) and np.array_equal(bits(got["lattice"][0]), bits(red[1][0])), name
        assert np.array_equal(got["types"], t), name
        if flag != cc.NO_GROUP:
            assert np.array_equal(bits(red[0]), bits(f)) and np.array_equal(bits(red[1][0]), bits(L)), name


def test_sample_with_conventional_cell(dev, fused_model):
    m, _ = fused_model
    out = []
    for kw in ({}, dict(conventional_cell=True), dict(conventional_cell=None),
               dict(conventional_cell=True, find_symmetry=True, screen=True, reduce_cell=True, symmetrize=True),
               dict(find_symmetry=True, screen=True, reduce_cell=True, symmetrize=True)):
        torch.manual_seed(3)
        np.random.seed(3)
        r = m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)
        out.append((r, torch.random.get_rng_state(), np.random.uniform()))
    plain = out[0][0]
    for r, rng, after in out[1:]:
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and torch.equal(out[0][1], rng) and out[0][2] == after
    a, none, every, others = out[1][0], out[2][0], out[3][0], out[4][0]
    assert plain.conventional is None and none.conventional is None and others.conventional is None
    assert a.symmetry is None and a.reduced is None and a.metrics is None and a.symmetrized is None
    conv = a.conventional
    assert set(conv) == set(cc.CONVENTIONAL_KEYS) and conv["transform"].shape == (3, 3, 3) and conv["lattice"].shape == (3, 3, 3)
    n_conv = int(conv["num_atoms"].sum())
    assert conv["frac_x"].shape == (n_conv, 3) and conv["atomic_numbers"].shape == (n_conv,) and conv["source"].shape == (n_conv,)
    assert (conv["num_atoms"] == conv["n_points"] * every.reduced["num_atoms"]).all()
    for k in cc.CONVENTIONAL_KEYS:  # alone against together with reduce_cell / find_symmetry / symmetrize: the shared launch changes nothing
        assert np.array_equal(bits(conv[k]), bits(every.conventional[k])), k
    for field in ("metrics", "symmetry", "reduced", "symmetrized"):  # every other instrument's arrays: as without the keyword
        x, y = getattr(every, field), getattr(others, field)
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))), (field, k)
    # the atoms of a conventional cell carry the atomic numbers of their reduced-cell sources
    first = np.concatenate([[0], np.cumsum(conv["num_atoms"])])
    rfirst = np.concatenate([[0], np.cumsum(every.reduced["num_atoms"])])
    for b in range(3):
        z = every.reduced["atomic_numbers"][rfirst[b]:rfirst[b + 1]]
        assert np.array_equal(conv["atomic_numbers"][first[b]:first[b + 1]], z[conv["source"][first[b]:first[b + 1]]])


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_round_trip_through_a_file(dev, tmp_path):
    """generate --conventional_cell on crystals sampled with P4/mmm symmetry, then screen --conventional_cell --out on a file of the
    disguised rock salt, fcc and rhombohedral cases: each a fresh process."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    ops = tmp_path / "p4mmm.txt"
    ops.write_text("-y,x,z\n-x,y,-z\n-x,-y,-z\n")
    out = str(tmp_path / "out" / "crystals.npz")
    text = _child(["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--batch", "4", "--num_steps", "10", "--symops", str(ops),
                   "--lattice_system", "tetragonal", "--orbits", "1", "--seed", "5", "--conventional_cell", "--symprec", "0.001", "--out", out], 300)
    assert re.search(r"conventional cell rank 0: classified \d / attempted 5; ", text) and "conventional cell total: " in text, text
    assert "symmetrize" not in text and "cell reduction" not in text, text  # the other instruments print nothing unasked
    res = load_sample_results_from_hdf5(out)
    conv = res.conventional
    assert set(conv) == set(cc.CONVENTIONAL_KEYS) and conv["bravais"].shape == (5,) and res.reduced is None and res.symmetrized is None
    ok = conv["flags"] == 0
    assert ok.any() and set(cc.BRAVAIS_NAMES[k] for k in conv["bravais"][ok]) <= {"tP", "tI", "cP", "cI", "cF"}
    # a file of known crystals
    picks = [cases.BY_NAME[n] for n in ("rocksalt", "fcc", "rhombohedral-35", "mono-C")]
    frac, lattice, counts, types = cases.ragged([cases.build(c, seed=0) for c in picks])
    num = np.array(counts, dtype=np.int64)
    known, out2 = str(tmp_path / "known.npz"), str(tmp_path / "conventional.npz")
    save_sample_results_to_hdf5(SampleResult(frac_x=frac.astype(np.float64), atomic_numbers=types.astype(np.float64), lattice=lattice.astype(np.float64),
                                             num_atoms=num, idx_start=np.cumsum(num) - num), known)
    text = _child(["arreau_amd.screen", known, "--conventional_cell", "--out", out2], 120)
    assert "conventional cell total: classified 4 / attempted 4; mS 1, hR 1, cF 2; flags none" in text and "wrote" in text, text
    back = load_sample_results_from_hdf5(out2)
    assert back.num_atoms.tolist() == [8, 4, 3, 6] and np.array_equal(back.frac_x, back.conventional["frac_x"].astype(np.float64))
    assert [cc.pearson_symbol(b, n) for b, n in zip(back.conventional["bravais"], back.num_atoms)] == ["cF8", "cF4", "hR3", "mS6"]
    assert np.abs(np.linalg.norm(back.lattice[0], axis=1) - 5.64).max() < 1e-4
    assert sorted(back.atomic_numbers[:8].tolist()) == [11] * 4 + [17] * 4


def test_argument_errors_touch_nothing(dev):
    got, red, _, _, _ = batch_run(dev)
    frac, lattice, off, types = device_batch(dev, (red[0][:1], red[1][:1], red[2][:1], red[3][:1]))
    with pytest.raises(ValueError, match="conventional_cell: types"):
        cc.conventional_cell(frac, lattice, off, types.to(torch.int64))
    found = ss.find_symmetry(frac, lattice, off, types, cases.PARAMS.search())
    out = cc.conventional_stage(frac, lattice, off, types, found)
    s = _hip.SymmetryResultC(*[_hip.ptr(found[k]).value for k in ss.SYM_KEYS[:-1]])
    r = _hip.ConventionalResultC(*[_hip.ptr(out[k]).value for k in cc.RESULT_KEYS])
    before = {k: out[k].clone() for k in cc.RESULT_KEYS}
    args = (_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(off))
    call = _hip.lib().arreau_crystal_conventional
    EINVAL = -1  # ARREAU_EINVAL
    for B, N, fnd, max_ops, res in ((1, 1, None, 192, ctypes.byref(r)), (1, 1, ctypes.byref(s), 192, None), (-1, 1, ctypes.byref(s), 192, ctypes.byref(r)),
                                    (1, -1, ctypes.byref(s), 192, ctypes.byref(r)), (1, 1, ctypes.byref(s), 0, ctypes.byref(r)),
                                    (1, 1, ctypes.byref(s), 4097, ctypes.byref(r)), (1, 1, ctypes.byref(_hip.SymmetryResultC()), 192, ctypes.byref(r)),
                                    (1, 1, ctypes.byref(s), 192, ctypes.byref(_hip.ConventionalResultC()))):
        assert call(*args, B, N, fnd, max_ops, res, _hip.stream_ptr(dev)) == EINVAL
        assert b"arreau_crystal_conventional" in _hip.lib().arreau_last_error()
    assert call(None, _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(off), 1, 1, ctypes.byref(s), 192, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    torch.cuda.synchronize()
    for k in cc.RESULT_KEYS:
        assert torch.equal(before[k], out[k]), k


def test_sample_takes_the_keyword_and_the_symbol_is_exported_everywhere(fused_model):
    """What fails without the feature: sample(conventional_cell=...) is a TypeError and the entry point is not in the library."""
    import inspect
    m, _ = fused_model
    assert "conventional_cell" in inspect.signature(m.sample).parameters
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_conventional(" in fh.read()
    assert "arreau_crystal_conventional" in _hip.EXPORTS
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_conventional")
