"""The symmetry search on the device (arreau_crystal_symmetry, csrc/symfind.hip) against the float64 restatement on every
guarded case of tests/symmetry_search_cases.py: every integer output and flag equal, the stored operations equal element by
element in order, translations within symmetry_search.TRANSLATION_BOUND (modulo 1) and residuals within
symmetry_search.residual_bound of the cell -- both derived from float32 rounding in diffusion/symmetry_search.py, never from the
kernel's output.  Then the shapes where it can go wrong (1, 2, 63, 64, 65 and 257 atoms, a ragged batch and each crystal
alone, an empty crystal among full ones, NONFINITE / CELL / AMBIGUOUS, OVERFLOW, max_ops = 1), argument errors,
sample(symmetry=spec, find_symmetry=...) end to end, find_symmetry=None without a side effect, determinism.
Needs an MI355X: `-m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import symmetry as sy
from arreau_amd.diffusion import symmetry_search as ss
from tests import symmetry_search_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401
from tests.symmetry_cases import GENS, ROCK_SALT

pytestmark = pytest.mark.gpu
INT_KEYS = ("n_lattice", "n_ops", "n_translations", "point_group", "flags")
ALL = list(cases.base_cases()) + list(cases.shape_cases().values())[2:] + [cases.overflow_case()]
_RUNS = {}


def launch(dev, batch, params, numpy=True):
    frac, lattice, counts, types = batch
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    out = ss.find_symmetry(up(frac.reshape(-1, 3)), up(lattice), up(off), up(types), params)
    return ss.result_to_numpy(out) if numpy else out


def batch_run(dev, params):
    """Every case with these parameters in ONE ragged launch (cached): (cases, result)."""
    if params not in _RUNS:
        group = [c for c in ALL if c.params == params]
        _RUNS[params] = (group, launch(dev, cases.batch_of(group), params))
    return _RUNS[params]


def assert_matches_reference(got, b, case, ref):
    for k in INT_KEYS:
        assert int(got[k][b]) == int(getattr(ref, k)[0]), (case.name, k)
    assert np.array_equal(got["ops_rotation"][b], ref.ops_rotation[0]), case.name
    stored = min(int(ref.n_ops[0]), case.params.max_ops)
    d = got["ops_translation"][b].astype(np.float64) - ref.ops_translation[0]
    dt = np.abs(d - np.rint(d)).max() if stored else 0.0
    bound = ss.residual_bound(case.lattice)
    dr = np.abs(got["ops_residual"][b].astype(np.float64) - ref.ops_residual[0]).max()
    dw = abs(float(got["residual"][b]) - float(ref.residual[0]))
    print(f"{case.name}: translation deviation {dt:.3g} (bound {ss.TRANSLATION_BOUND:.3g}), residual deviation {max(dr, dw):.3g} (bound {bound:.3g})")
    assert dt <= ss.TRANSLATION_BOUND, case.name
    assert dr <= bound and dw <= bound, case.name
    assert (got["ops_translation"][b][stored:] == 0).all() and (got["ops_residual"][b][stored:] == 0).all()


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_kernel_against_the_restatement(dev, case):
    group, got = batch_run(dev, case.params)
    b = [c.name for c in group].index(case.name)
    assert_matches_reference(got, b, case, cases.reference(case))
    assert (int(got["n_ops"][b]), int(got["n_translations"][b]), ss.point_group_name(got["point_group"][b]), int(got["flags"][b])) == \
        (case.n_ops, case.n_translations, case.point_group, case.flags)


@pytest.mark.parametrize("name", ["n1", "n2", "n63", "n64", "n65", "n257"])
def test_a_crystal_alone_is_its_row_of_the_ragged_batch(dev, name):
    case = cases.shape_cases()[name]
    group, got = batch_run(dev, case.params)
    b = [c.name for c in group].index(case.name)
    alone = launch(dev, cases.batch_of([case]), case.params)
    for k in ss.SYM_KEYS:
        assert np.array_equal(alone[k][0], got[k][b], equal_nan=True), (name, k)
    assert int(alone["n_ops"][0]) == case.n_ops and ss.point_group_name(alone["point_group"][0]) == case.point_group


def test_overflow_stores_the_first_operations(dev):
    case, full = cases.overflow_case(), cases.shape_cases()["n64"]
    (_, small), (_, big) = batch_run(dev, case.params), batch_run(dev, full.params)
    b = [c.name for c in batch_run(dev, case.params)[0]].index(case.name)
    f = [c.name for c in batch_run(dev, full.params)[0]].index(full.name)
    assert int(small["n_ops"][b]) == 1536 and int(small["flags"][b]) == ss.OVERFLOW and int(big["flags"][f]) == 0
    for k in ("ops_rotation", "ops_translation", "ops_residual"):
        assert np.array_equal(small[k][b], big[k][f][:192]), k
    assert small["residual"][b] == big["residual"][f] and small["point_group"][b] == big["point_group"][f] == 31


def test_max_ops_one(dev):
    by = {c.name: c for c in cases.base_cases()}
    picks = [by["triclinic"], by["NaCl displaced"], by["hcp"]]
    p = ss.SymmetrySearchParams(symprec=cases.SYMPREC, max_ops=1)
    got = launch(dev, cases.batch_of(picks), p)
    assert got["ops_rotation"].shape == (3, 1) and got["ops_translation"].shape == (3, 1, 3)
    assert got["n_ops"].tolist() == [1, 192, 24] and got["flags"].tolist() == [0, ss.OVERFLOW, ss.OVERFLOW]
    assert got["point_group"].tolist() == [0, 31, 26]
    full = batch_run(dev, cases.PARAMS)
    for b, c in enumerate(picks):
        f = [x.name for x in full[0]].index(c.name)
        assert got["ops_rotation"][b, 0] == full[1]["ops_rotation"][f, 0] and got["residual"][b] == full[1]["residual"][f]


def test_flagged_crystals_among_full_ones(dev):
    by = {c.name: c for c in cases.base_cases()}
    cs, one = by["CsCl"], by["one atom, cubic"]
    frac = np.concatenate([cs.frac, cs.frac, cs.frac, cs.frac, cs.frac]).astype(np.float32)
    frac[2, 1] = np.nan                       # crystal 1
    lattice = np.stack([cs.lattice] * 7).astype(np.float32)
    lattice[2] = 0.0                          # crystal 2: no volume
    lattice[5, 1, 1] = np.inf                 # crystal 5
    counts = [2, 2, 2, 0, 2, 2, 0]            # crystals 3 and 6 are empty, 6 is the last
    types = np.tile(cs.types, 5).astype(np.int32)
    got = launch(dev, (frac, lattice, counts, types), cases.PARAMS)
    ref = ss.symmetry_reference_f64(frac, lattice, counts, types, cases.PARAMS)
    assert got["flags"].tolist() == ref.flags.tolist() == [0, ss.NONFINITE, ss.CELL, ss.EMPTY, 0, ss.NONFINITE, ss.EMPTY]
    for k in INT_KEYS:
        assert got[k].tolist() == getattr(ref, k).tolist(), k
    assert np.array_equal(got["ops_rotation"], ref.ops_rotation) and got["n_ops"].tolist() == [48, 0, 0, 0, 48, 0, 0]
    assert np.isnan(got["residual"][[1, 2, 3, 5, 6]]).all() and (got["ops_translation"][[1, 2, 3, 5, 6]] == 0).all()
    # AMBIGUOUS: a 3 A cubic cell with symprec 4 A -- the deviations are 0, 1.24, 2.2 and 3 A (pass), 6 and 9 A (fail)
    loose = ss.SymmetrySearchParams(symprec=4.0)
    got = launch(dev, cases.batch_of([one, one]), loose)
    ref = ss.symmetry_reference_f64(one.frac, one.lattice[None], [1], one.types, loose)
    assert got["flags"].tolist() == [ss.AMBIGUOUS] * 2 and int(ref.flags[0]) == ss.AMBIGUOUS
    assert got["n_lattice"].tolist() == [int(ref.n_lattice[0])] * 2 and ref.n_lattice[0] > 48
    assert got["n_ops"].tolist() == [0, 0] and got["point_group"].tolist() == [-1, -1] and (got["ops_rotation"] == -1).all()
    # no crystal at all, and no atom at all
    empty = launch(dev, (np.zeros((0, 3), np.float32), np.zeros((0, 3, 3), np.float32), [], np.zeros(0, np.int32)), cases.PARAMS)
    assert empty["flags"].shape == (0,) and empty["ops_rotation"].shape == (0, 192)
    none = launch(dev, (np.zeros((0, 3), np.float32), cs.lattice[None], [0], np.zeros(0, np.int32)), cases.PARAMS)
    assert none["flags"].tolist() == [ss.EMPTY]


def test_bad_arguments_launch_nothing(dev):
    case = {c.name: c for c in cases.base_cases()}["CsCl"]
    frac, lattice, counts, types = cases.batch_of([case])
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    frac, lattice, types, off = up(frac), up(lattice), up(types), up(np.array([0, 2], np.int32))
    M = 4
    arrays = {"n_lattice": (1,), "n_ops": (1,), "n_translations": (1,), "ops_rotation": (1, M), "ops_translation": (1, M, 3),
              "ops_residual": (1, M), "residual": (1,), "point_group": (1,), "flags": (1,)}
    out = {k: torch.full(shape, -7, device=dev, dtype=torch.float32 if k in ("ops_translation", "ops_residual", "residual") else torch.int32)
           for k, shape in arrays.items()}
    lib = _hip.lib()

    def call(symprec=0.01, max_ops=M, params=True, result=True, B=1, N=2, lat=lattice, null_array=None, ty=types):
        p = _hip.SymmetryParamsC(symprec, max_ops)
        r = _hip.SymmetryResultC(*[None if k == null_array else _hip.ptr(out[k]).value for k in arrays])
        return lib.arreau_crystal_symmetry(_hip.ptr(frac), _hip.ptr(ty), _hip.ptr(lat), _hip.ptr(off), B, N,
                                           ctypes.byref(p) if params else None, ctypes.byref(r) if result else None, _hip.stream_ptr(dev))

    bad = [dict(symprec=0.0), dict(symprec=-0.1), dict(symprec=float("nan")), dict(symprec=float("inf")), dict(max_ops=0),
           dict(max_ops=ss.MAX_OPS_CAP + 1), dict(params=False), dict(result=False), dict(B=-1), dict(N=-1), dict(lat=None),
           dict(ty=None), dict(null_array="ops_residual"), dict(null_array="flags")]
    for kw in bad:
        assert call(**kw) == -1, kw  # ARREAU_EINVAL
        assert "arreau_crystal_symmetry" in lib.arreau_last_error().decode()
    torch.cuda.synchronize(dev)
    for k, v in out.items():
        assert bool((v == -7).all()), k  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert int(out["n_ops"][0]) == 48 and int(out["flags"][0]) == ss.OVERFLOW
    with pytest.raises(ValueError, match="find_symmetry: types"):
        ss.find_symmetry(frac, lattice, off, types.to(torch.int64))
    with pytest.raises(ValueError, match="find_symmetry: lattice"):
        ss.find_symmetry(frac, lattice.cpu(), off, types)


def test_two_launches_are_bitwise_equal(dev):
    group = [c for c in ALL if c.params == cases.PARAMS]
    first = batch_run(dev, cases.PARAMS)[1]
    again = launch(dev, cases.batch_of(group), cases.PARAMS)
    for k in ss.SYM_KEYS:
        assert np.array_equal(first[k], again[k], equal_nan=True), k


def test_engine_entry_points(dev, fused_model):
    from arreau_amd import engine
    m, _ = fused_model
    case = {c.name: c for c in cases.base_cases()}["hcp"]
    frac, lattice, counts, types = cases.batch_of([case])
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    args = (up(frac), up(lattice), up(np.array([0, 2], np.int32)), up(types), cases.PARAMS)
    a, b = engine.find_symmetry(*args), m.engine().find_symmetry(*args)
    assert int(a["n_ops"][0]) == int(b["n_ops"][0]) == 24 and torch.equal(a["ops_rotation"], b["ops_rotation"])


# ------------------------------------------------------------------------------------------------------------ end to end
def _spec(name):
    if name == "P4/mmm general positions":
        return sy.SymmetrySpec.general_positions(("-y,x,z", "-x,y,-z", "-x,-y,-z"), 1, "tetragonal")
    return sy.SymmetrySpec.from_template(ROCK_SALT, GENS["Fm-3m"], "cubic")


@pytest.mark.parametrize("name", ["P4/mmm general positions", "rock salt template"])
def test_the_symmetric_sampler_delivers_its_group(dev, fused_model, name):
    """sample(symmetry=spec) seen the way a user sees it: the finished crystals contain the spec's group, and every operation of
    the group has a residual within the float32 bound of zero."""
    m, _ = fused_model
    spec = _spec(name)
    # symprec: far above the float32 bound of the residuals (1e-5 A and less) and far below the cells of the synthetic model after
    # six steps (some are 0.02 A wide); max_ops: room for a crystal that has more than its spec asks
    params = ss.SymmetrySearchParams(symprec=1.0e-3, max_ops=ss.MAX_OPS_CAP)
    res = m.sample(spec.n_atoms, 3, symmetry=spec, seed=31, max_steps=6, find_symmetry=params)
    found = res.symmetry
    assert found is not None and found["n_ops"].shape == (3,) and found["ops_rotation"].shape == (3, ss.MAX_OPS_CAP)
    assert np.array_equal(found["lattice"], res.lattice.astype(np.float32))
    off = np.concatenate([[0], np.cumsum(res.num_atoms)])
    for b in range(3):
        assert not int(found["flags"][b]) & ss.NO_RESULT_MASK, ss.describe(found["flags"][b])
        bound = ss.residual_bound(found["lattice"][b])
        sl = slice(off[b], off[b + 1])
        exact = ss.operation_residuals(res.frac_x[sl], found["lattice"][b], res.atomic_numbers[sl], spec.ops)
        codes = found["ops_rotation"][b][:int(found["n_ops"][b])]
        mine = np.isin(codes, [ss.encode_rotation(R) for R, _ in spec.ops])
        print(f"{name} crystal {b}: n_ops {int(found['n_ops'][b])}, point group {ss.point_group_name(found['point_group'][b])}, "
              f"float64 residuals of the spec's group max {exact.max():.3g}, kernel's max {found['ops_residual'][b][:len(codes)][mine].max():.3g} "
              f"(bound {bound:.3g})")
        assert ss.contains(found, b, spec), (name, b)
        assert exact.max() <= bound, (name, b)
        assert int(found["n_ops"][b]) >= spec.order


def test_none_adds_nothing(dev, fused_model):
    m, _ = fused_model
    out = []
    for kw in ({}, dict(find_symmetry=None), dict(find_symmetry=True)):
        torch.manual_seed(3)
        np.random.seed(3)
        r = m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)
        out.append((r, torch.random.get_rng_state(), np.random.uniform()))
    a = out[0][0]
    for r, rng, after in out[1:]:
        assert np.array_equal(a.frac_x, r.frac_x) and np.array_equal(a.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(a.lattice, r.lattice) and torch.equal(out[0][1], rng) and out[0][2] == after
    assert out[0][0].symmetry is None and out[1][0].symmetry is None and a.metrics is None and a.uniqueness is None
    found = out[2][0].symmetry
    assert found["n_ops"].shape == (3,) and found["ops_rotation"].shape == (3, 192) and float(found["symprec"][0]) == np.float32(0.1)
    assert (((found["flags"] & ss.NO_RESULT_MASK) != 0) | (found["n_ops"] >= 1)).all()  # the identity at least


# ---------------------------------------------------------------------------------------------------------- command lines
def test_screen_command_line(dev, tmp_path, capsys):
    from arreau_amd import screen
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    by = {c.name: c for c in cases.base_cases()}
    picks = [by["triclinic"], by["NaCl"], by["hcp displaced"]]
    frac, lattice, counts, types = cases.batch_of(picks)
    counts = np.array(counts)
    src = save_sample_results_to_hdf5(SampleResult(frac_x=frac.astype(np.float64), atomic_numbers=types.astype(np.float64) + 1.0,
                                                   lattice=lattice.astype(np.float64), num_atoms=counts, idx_start=np.cumsum(counts) - counts),
                                      str(tmp_path / "in.npz"))
    out = str(tmp_path / "out.npz")
    screen.main([src, "--find_symmetry", "--symprec", str(cases.SYMPREC), "--out", out])
    text = capsys.readouterr().out
    assert "symmetry total: classified 3 / attempted 3; triclinic 1, hexagonal 1, cubic 1; point groups 1: 1, 6/mmm: 1, m-3m: 1; flags none" in text
    back = load_sample_results_from_hdf5(out)
    assert back.symmetry["n_ops"].tolist() == [1, 192, 24] and back.symmetry["point_group"].tolist() == [0, 31, 26]
    assert ss.contains(back.symmetry, 1, cases.FM3M) and back.metrics is not None


def test_generate_command_line(dev, tmp_path):
    import os
    import re
    import subprocess
    import sys
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    ops = tmp_path / "p4mmm.txt"
    ops.write_text("-y,x,z\n-x,y,-z\n-x,-y,-z\n")
    out = str(tmp_path / "out" / "crystals.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = root
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5",
                        "--batch", "4", "--num_steps", "10", "--symops", str(ops), "--lattice_system", "tetragonal", "--orbits", "1",
                        "--seed", "5", "--find_symmetry", "--symprec", "0.001", "--out", out], env=env, cwd=root, capture_output=True,
                       text=True, timeout=330)
    assert p.returncode == 0, p.stderr[-3000:]
    assert re.search(r"symmetry rank 0: classified \d / attempted 5; ", p.stdout) and "symmetry total: " in p.stdout, p.stdout
    assert "symmetry: 5 / 5 crystals contain the requested group (|G| = 16)" in p.stdout, p.stdout
    res = load_sample_results_from_hdf5(out)
    assert res.symmetry["n_ops"].shape == (5,) and res.symmetry["ops_rotation"].shape == (5, 192) and (res.symmetry["n_ops"] >= 16).all()
