"""Cell reduction on the device (arreau_crystal_reduce, csrc/reduce.hip) against the float64 restatement on every guarded case of
tests/cell_reduction_cases.py in one ragged batch: flags, multiplicity, n_out, keep and selling_steps equal, lattice and positions
within twice the bounds derived in diffusion/cell_reduction.py (never from the kernel's output).  The same assertions on
`size_cases()` and `size_flag_cases()` in a second ragged launch of 18 crystals and 2,264 atoms: 63 / 64 / 65 atoms (a second
block of 64 lanes in the candidate loop), 80 atoms of which only the first 64, or only the last 16, reject a candidate, 257 to
264 atoms (the unstaged path, two rounds of 256, counters carried between them, a class representative at 256, copy_through past
256), 27 and 64 translations (the closure and triple loops past 256 threads, K = 66), 65 translations, face and rhombohedral
centring, an open closure; their bits alone in a launch and in a repeated launch; the fingerprint of each against its reduced
form.  Then the other instruments, unchanged, on its results: the fingerprint of a crystal and of its reduced form, the symmetry search on a skewed rock salt and on
its reduced cell; the flags; sample(reduce_cell=...); the export.  Needs an MI355X: `-m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import cell_reduction as cr
from arreau_amd.diffusion import symmetry_search as ss
from arreau_amd.diffusion import uniqueness as uq
from tests import cell_reduction_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
INT_KEYS = ("multiplicity", "n_translations", "n_out", "flags", "selling_steps")
_RUN = {}
# The fingerprint enumerates at most 8 images per axis (its CELL rule): r_cut = r_max + 5 sigma <= 8 x the narrowest plane spacing of
# a cell.  The most skewed input here ("P1 skew 2") has planes 0.58 A apart, so r_max = 4 A (r_cut 4.5 A, 7.8 images) keeps every
# input inside the fingerprint's own domain; the default 6 A would flag that input CELL, and a flagged crystal matches nothing.
FP_PARAMS = uq.FingerprintParams(r_max=4.0)


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, batch):
    frac, lattice, counts, types = batch
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return up(dev, frac.reshape(-1, 3)), up(dev, lattice), up(dev, off), up(dev, types)


def launch(dev, batch, params=cases.PARAMS):
    return cr.result_to_numpy(cr.reduce_cells(*device_batch(dev, batch), params))


def batch_run(dev):
    """Every guarded case in ONE ragged launch (cached): (cases, batch, result)."""
    if "all" not in _RUN:
        group = list(cases.cases().values())
        batch = cases.batch_of(group)
        _RUN["all"] = (group, batch, launch(dev, batch))
    return _RUN["all"]


def test_kernel_matches_the_f64_restatement(dev):
    group, batch, got = batch_run(dev)
    first = np.concatenate([[0], np.cumsum(batch[2])])
    worst = {"lattice": 0.0, "position": 0.0}
    for b, case in enumerate(group):
        ref = cases.reference(case)
        for k in INT_KEYS:
            assert int(got[k][b]) == int(getattr(ref, k)[0]), (case.name, k)
        assert int(got["multiplicity"][b]) == case.multiplicity and int(got["flags"][b]) == 0, case.name
        sl = slice(first[b], first[b + 1])
        assert np.array_equal(got["keep"][sl], ref.keep), case.name
        assert np.array_equal(got["types_out"][sl], ref.types_out), case.name
        L = case.lattice.astype(np.float64)
        lat_bound, pos_bound = 2.0 * cr.lattice_bound(ref.transform[0], L), 2.0 * cr.position_bound(ref.inverse[0])
        assert np.array_equal(got["transform"][b].astype(np.float64), (ref.transform[0]).astype(np.float32).astype(np.float64)), case.name
        d_lat = float(np.abs(got["lattice_out"][b].astype(np.float64) - ref.lattice_out[0]).max())
        n_out = int(ref.n_out[0])
        d = got["frac_out"][sl][:n_out].astype(np.float64) - ref.frac_out[:n_out]
        d_pos = float(np.abs(d - np.rint(d)).max())
        print(f"{case.name}: m {case.multiplicity} steps {int(got['selling_steps'][b])} |lattice - f64| {d_lat:.3e} (bound {lat_bound:.3e}) "
              f"|x - f64| {d_pos:.3e} (bound {pos_bound:.3e})")
        worst["lattice"], worst["position"] = max(worst["lattice"], d_lat / lat_bound), max(worst["position"], d_pos / pos_bound)
        assert d_lat <= lat_bound and d_pos <= pos_bound, case.name
        assert (got["frac_out"][sl][n_out:] == 0).all() and (got["keep"][sl][n_out:] == -1).all()
    print("largest deviation / tolerance:", worst)


def test_repeated_and_eager_runs_give_the_same_bits(dev):
    group, batch, got = batch_run(dev)
    again = launch(dev, batch)
    for k in cr.RED_KEYS:
        assert np.array_equal(got[k], again[k]), k
    alone = launch(dev, cases.batch_of(group[2:3]))  # a crystal's rows do not depend on its place in the batch
    assert np.array_equal(alone["lattice_out"][0], got["lattice_out"][2]) and int(alone["multiplicity"][0]) == 8
    assert np.array_equal(alone["frac_out"][:2], got["frac_x"][int(got["num_atoms"][:2].sum()):][:2])


def test_fingerprint_of_the_reduced_form_matches_the_input(dev):
    """uniqueness claims invariance under a change of basis and supercells: arreau_fingerprint_match between every input crystal
    and its reduced form, within the uniqueness test's float32 bound."""
    group, batch, got = batch_run(dev)
    fx = uq.fingerprint(*device_batch(dev, batch), FP_PARAMS)
    red = (got["frac_x"], got["lattice"], [int(v) for v in got["num_atoms"]], got["types"])
    fy = uq.fingerprint(*device_batch(dev, red), FP_PARAMS)
    assert not fx["flags"].any().item() and not fy["flags"].any().item(), (fx["flags"], fy["flags"])
    row = lambda f, b: {k: v[b:b + 1].contiguous() for k, v in f.items()}
    for b, case in enumerate(group):
        m = uq.match(row(fx, b), row(fy, b), 0.01)
        d = float(m["nearest_distance"].cpu()[0])
        print(f"{case.name}: fingerprint distance input / reduced {d:.3e} (bound {uq.D_BOUND:.3e})")
        assert int(m["nearest"].cpu()[0]) == 0 and abs(d) <= uq.D_BOUND, case.name


def test_symmetry_search_finds_the_full_group_only_on_the_reduced_cell(dev):
    """Rock salt 2x1x1 in a skewed basis: the search (entries of W in {-1, 0, 1}) misses operations there -- shown first with its
    float64 restatement on the host -- and finds all 48 x 1 on the reduced cell."""
    case = cases.skewed_rock_salt(0, (2, 1, 1))
    params = ss.SymmetrySearchParams(symprec=cases.SYMPREC, max_ops=192)
    full = 48 * case.multiplicity
    host = ss.symmetry_reference_f64(case.frac, case.lattice[None], [case.n], case.types, params)
    assert int(host.n_ops[0]) < full, "the skew does not hide an operation from the search"
    batch = cases.batch_of([case])
    on_input = ss.result_to_numpy(ss.find_symmetry(*device_batch(dev, batch), params))
    got = launch(dev, batch)
    assert int(got["flags"][0]) == 0 and int(got["multiplicity"][0]) == 2 and int(got["num_atoms"][0]) == 2
    assert abs(abs(np.linalg.det(got["lattice"][0].astype(np.float64))) - cases.A_NACL ** 3 / 4) < 1e-3
    red = (got["frac_x"], got["lattice"], [2], got["types"])
    on_reduced = ss.result_to_numpy(ss.find_symmetry(*device_batch(dev, red), params))
    print(f"operations found: skewed input {int(on_input['n_ops'][0])} (float64 restatement {int(host.n_ops[0])}) of {full}; "
          f"reduced cell {int(on_reduced['n_ops'][0])} of 48")
    assert int(on_input["n_ops"][0]) == int(host.n_ops[0]) < full
    assert int(on_reduced["n_ops"][0]) == 48 and int(on_reduced["n_translations"][0]) == 1
    assert ss.point_group_name(on_reduced["point_group"][0]) == "m-3m"


def flag_cases():
    f, L, t = cases.rock_salt((2, 1, 1))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    nan = f.copy()
    nan[1, 2] = np.nan
    flat = L.copy()
    flat[2] = 0.0  # (a volume of exactly zero in float32 and float64)
    near = f.copy()  # the second chlorine 1.5 symprec off its translated place: the candidate's residual is 1.5 symprec
    near[3] += np.linalg.solve(L.T, np.array([1.5 * cases.SYMPREC, 0.0, 0.0]))
    # a third chlorine 0.3 symprec beside the first: the translation is still accepted, and 2 does not divide 5
    odd_f = np.concatenate([f, f[1:2] + np.linalg.solve(L.T, np.array([0.3 * cases.SYMPREC, 0.0, 0.0]))[None, :]])
    odd_t = np.concatenate([t, [17]])
    return [("nan", f32(nan), f32(L), t, cr.NONFINITE, 0), ("flat", f32(f), f32(flat), t, cr.CELL, 0),
            ("near", f32(near), f32(L), t, 0, 1), ("odd", f32(odd_f), f32(L), odd_t, cr.AMBIGUOUS, 2)]


def test_flags(dev):
    group = flag_cases()
    batch = (np.concatenate([c[1] for c in group]), np.stack([c[2] for c in group]), [len(c[1]) for c in group],
             np.concatenate([c[3] for c in group]).astype(np.int32))
    got = launch(dev, batch)
    ref = cr.reduce_reference_f64(*batch, cases.PARAMS)
    first = np.concatenate([[0], np.cumsum(batch[2])])
    for b, (name, f, L, t, flags, n_translations) in enumerate(group):
        assert int(got["flags"][b]) == flags == int(ref.flags[b]), (name, cr.describe(got["flags"][b]))
        assert int(got["n_translations"][b]) == n_translations == int(ref.n_translations[b]), name
        assert int(got["multiplicity"][b]) == 1, name
        sl = slice(first[b], first[b + 1])
        if flags & cr.COPIED_MASK:  # copied through, bit for bit
            assert np.array_equal(got["frac_out"][sl].view(np.int32), f.view(np.int32)), name
            assert np.array_equal(got["lattice_out"][b].view(np.int32), L.view(np.int32)), name
            assert np.array_equal(got["types_out"][sl], t) and np.array_equal(got["keep"][sl], np.arange(len(f))), name
            assert np.array_equal(got["transform"][b], np.eye(3, dtype=np.float32)) and int(got["n_out"][b]) == len(f), name
        else:
            assert int(got["n_out"][b]) == len(f) and int(got["flags"][b]) == 0, name


# ------------------------------------------------------------- past 16 atoms: rounds, 64 translations, closure (size_cases)
# the 257-, 260-, 261- and 264-atom crystals between small ones, the flagged crystals among the reduced ones
SIZE_ORDER = ("face-centred", "rounds 260 permuted", "P1 n63", "261 atoms", "R-centred", "P1 n257", "open closure", "2-atom 4x4x4",
              "rounds 264 permuted", "P1 n64", "first block decides", "65 translations", "last block decides", "2-atom 3x2x1", "nan in atom 258", "P1 n65", "rounds 260", "2-atom 3x3x3")


def size_group():
    """[(Case, FlagCase or None)] in SIZE_ORDER: every size case and every flagged one."""
    assert sorted(SIZE_ORDER) == sorted(cases.SIZE_NAMES + cases.SIZE_FLAG_NAMES)
    flagged = cases.size_flag_cases()
    return [(flagged[k].case, flagged[k]) if k in flagged else (cases.size_cases()[k], None) for k in SIZE_ORDER]


def size_run(dev):
    """Every size case and flagged size case in ONE ragged launch (cached): (group, batch, first atom of each crystal, result)."""
    if "size" not in _RUN:
        group = size_group()
        batch = cases.batch_of([c for c, _ in group])
        _RUN["size"] = (group, batch, np.concatenate([[0], np.cumsum(batch[2])]), launch(dev, batch))
    return _RUN["size"]


def test_size_cases_match_the_f64_restatement(dev):
    """test_kernel_matches_the_f64_restatement's assertions on the cases whose loops make a second trip."""
    group, batch, first, got = size_run(dev)
    worst = {"lattice": 0.0, "position": 0.0}
    for b, (case, flagged) in enumerate(group):
        if flagged is not None:
            continue
        ref = cases.reference(case)
        for k in INT_KEYS:
            assert int(got[k][b]) == int(getattr(ref, k)[0]), (case.name, k)
        assert int(got["multiplicity"][b]) == case.multiplicity and int(got["flags"][b]) == 0, case.name
        sl = slice(first[b], first[b + 1])
        assert np.array_equal(got["keep"][sl], ref.keep), case.name
        assert np.array_equal(got["types_out"][sl], ref.types_out), case.name
        L = case.lattice.astype(np.float64)
        lat_bound, pos_bound = 2.0 * cr.lattice_bound(ref.transform[0], L), 2.0 * cr.position_bound(ref.inverse[0])
        assert np.array_equal(got["transform"][b].astype(np.float64), (ref.transform[0]).astype(np.float32).astype(np.float64)), case.name
        d_lat = float(np.abs(got["lattice_out"][b].astype(np.float64) - ref.lattice_out[0]).max())
        n_out = int(ref.n_out[0])
        d = got["frac_out"][sl][:n_out].astype(np.float64) - ref.frac_out[:n_out]
        d_pos = float(np.abs(d - np.rint(d)).max())
        print(f"{case.name}: n {case.n} m {case.multiplicity} steps {int(got['selling_steps'][b])} |lattice - f64| {d_lat:.3e} "
              f"(bound {lat_bound:.3e}, {d_lat / lat_bound:.3f} of it) |x - f64| {d_pos:.3e} (bound {pos_bound:.3e}, {d_pos / pos_bound:.3f} of it)")
        worst["lattice"], worst["position"] = max(worst["lattice"], d_lat / lat_bound), max(worst["position"], d_pos / pos_bound)
        assert d_lat <= lat_bound and d_pos <= pos_bound, case.name
        assert (got["frac_out"][sl][n_out:] == 0).all() and (got["keep"][sl][n_out:] == -1).all() and (got["types_out"][sl][n_out:] == -1).all()
    print("largest deviation / tolerance:", worst)


def test_size_flag_cases_are_copied_through(dev):
    """65 translations, the open closure, 261 atoms (copy_through strides twice) and the NaN in the second round of 256."""
    group, batch, first, got = size_run(dev)
    seen = 0
    for b, (case, flagged) in enumerate(group):
        if flagged is None:
            continue
        seen += 1
        ref, name = cases.reference(case), case.name
        assert int(got["flags"][b]) == flagged.flags == int(ref.flags[0]), (name, cr.describe(got["flags"][b]))
        assert int(got["n_translations"][b]) == flagged.n_translations == int(ref.n_translations[0]), name
        assert int(got["multiplicity"][b]) == 1 and int(got["n_out"][b]) == case.n and int(got["selling_steps"][b]) == 0, name
        sl = slice(first[b], first[b + 1])
        assert np.array_equal(got["frac_out"][sl].view(np.int32), case.frac.view(np.int32)), name
        assert np.array_equal(got["lattice_out"][b].view(np.int32), case.lattice.view(np.int32)), name
        assert np.array_equal(got["types_out"][sl], case.types) and np.array_equal(got["keep"][sl], np.arange(case.n)), name
        assert np.array_equal(got["transform"][b], np.eye(3, dtype=np.float32)), name
    assert seen == len(cases.SIZE_FLAG_NAMES) == 4


def test_size_cases_do_not_depend_on_their_place_or_the_launch(dev):
    group, batch, first, got = size_run(dev)
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a  # (a NaN that was copied through equals itself)
    again = launch(dev, batch)
    for k in cr.RED_KEYS:
        assert np.array_equal(bits(got[k]), bits(again[k])), k
    for name in ("2-atom 4x4x4", "rounds 260 permuted"):
        b = SIZE_ORDER.index(name)
        alone = launch(dev, cases.batch_of([group[b][0]]))
        for k in cr.CRYSTAL_KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(got[k][b])), (name, k)
        for k in cr.ATOM_KEYS:
            assert np.array_equal(bits(alone[k]), bits(got[k][first[b]:first[b + 1]])), (name, k)


def test_fingerprint_of_the_reduced_size_cases_matches_the_input(dev):
    """test_fingerprint_of_the_reduced_form_matches_the_input on every unflagged size case, none left out."""
    group, batch, first, got = size_run(dev)
    rows = [b for b, (_, flagged) in enumerate(group) if flagged is None]
    assert len(rows) == len(cases.SIZE_NAMES)
    fx = uq.fingerprint(*device_batch(dev, cases.batch_of([group[b][0] for b in rows])), FP_PARAMS)
    red = (np.concatenate([got["frac_out"][first[b]:first[b] + int(got["n_out"][b])] for b in rows]), got["lattice_out"][rows],
           [int(got["n_out"][b]) for b in rows], np.concatenate([got["types_out"][first[b]:first[b] + int(got["n_out"][b])] for b in rows]))
    fy = uq.fingerprint(*device_batch(dev, red), FP_PARAMS)
    assert not fx["flags"].any().item() and not fy["flags"].any().item(), (fx["flags"], fy["flags"])
    row = lambda f, r: {k: v[r:r + 1].contiguous() for k, v in f.items()}
    for r, b in enumerate(rows):
        m = uq.match(row(fx, r), row(fy, r), 0.01)
        d = float(m["nearest_distance"].cpu()[0])
        print(f"{group[b][0].name}: fingerprint distance input / reduced {d:.3e} (bound {uq.D_BOUND:.3e})")
        assert int(m["nearest"].cpu()[0]) == 0 and abs(d) <= uq.D_BOUND, group[b][0].name


def test_argument_errors_touch_nothing(dev):
    frac, lattice, off, types = device_batch(dev, cases.batch_of(list(cases.cases().values())[:1]))
    with pytest.raises(ValueError, match="reduce_cells: types"):
        cr.reduce_cells(frac, lattice, off, types.to(torch.int64))
    c, r = _hip.ReduceParamsC(float("nan")), _hip.ReduceResultC()
    rc = _hip.lib().arreau_crystal_reduce(_hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(off), 1, 2, ctypes.byref(c),
                                          ctypes.byref(r), _hip.stream_ptr(dev))
    assert rc != 0 and b"symprec" in _hip.lib().arreau_last_error()


def test_engine_entry_points(dev, fused_model):
    from arreau_amd import engine
    m, _ = fused_model
    args = device_batch(dev, cases.batch_of([cases.cases()["body-centred"]])) + (cases.PARAMS,)
    a, b = engine.reduce_cells(*args), m.engine().reduce_cells(*args)
    assert int(a["multiplicity"][0]) == int(b["multiplicity"][0]) == 2 and torch.equal(a["frac_out"], b["frac_out"])


def test_sample_with_reduce_cell(dev, fused_model):
    m, _ = fused_model
    out = []
    for kw in ({}, dict(reduce_cell=True), dict(reduce_cell=True), dict(reduce_cell=None)):
        torch.manual_seed(3)
        np.random.seed(3)
        out.append(m.sample(8, 4, seed=777, max_steps=6, **kw))
    plain, a, b, none = out
    for r in (a, b, none):
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and np.array_equal(plain.num_atoms, r.num_atoms)
        assert r.metrics is None and r.uniqueness is None and r.symmetry is None
    assert plain.reduced is None and none.reduced is None
    red = a.reduced
    assert set(red) == set(cr.REDUCED_KEYS)
    n_red = int(red["num_atoms"].sum())
    assert red["multiplicity"].shape == (4,) and red["lattice"].shape == (4, 3, 3) and red["transform"].shape == (4, 3, 3)
    assert red["frac_x"].shape == (n_red, 3) and red["atomic_numbers"].shape == (n_red,) and red["keep"].shape == (n_red,)
    assert (red["num_atoms"] * red["multiplicity"] == 8).all() and float(red["symprec"][0]) == np.float32(0.1)
    first = np.concatenate([[0], np.cumsum(red["num_atoms"])])
    for c in range(4):
        assert np.array_equal(red["atomic_numbers"][first[c]:first[c + 1]], plain.atomic_numbers[8 * c + red["keep"][first[c]:first[c + 1]]])
    for k in cr.REDUCED_KEYS:
        assert np.array_equal(red[k], b.reduced[k], equal_nan=True), k


def test_screen_command_line_writes_the_reduced_crystals(dev, tmp_path, capsys):
    from arreau_amd import screen
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    group = [cases.cases()[k] for k in ("rock salt 2x2x2", "P1", "body-centred")]
    frac, lattice, counts, types = cases.batch_of(group)
    num = np.array(counts, dtype=np.int64)
    src, out = str(tmp_path / "crystals.npz"), str(tmp_path / "reduced.npz")
    save_sample_results_to_hdf5(SampleResult(frac_x=frac.astype(np.float64), atomic_numbers=types.astype(np.float64),
                                             lattice=lattice.astype(np.float64), num_atoms=num, idx_start=np.cumsum(num) - num), src)
    screen.main([src, "--reduce_cell", "--symprec", str(cases.SYMPREC), "--out", out])
    printed = capsys.readouterr().out
    assert "cell reduction total: reduced 3 / attempted 3; multiplicity 1: 1, 2: 1, 8: 1; flags none" in printed
    red = load_sample_results_from_hdf5(out)
    assert red.num_atoms.tolist() == [2, 7, 2] and red.frac_x.shape == (11, 3)
    assert red.reduced is not None and red.reduced["multiplicity"].tolist() == [8, 1, 2]
    screen.main([out, "--find_symmetry", "--symprec", str(cases.SYMPREC)])  # the other instruments run on the reduced file
    assert "m-3m: 1" in capsys.readouterr().out


def test_the_symbol_is_exported_everywhere():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_reduce(" in fh.read()
    assert "arreau_crystal_reduce" in _hip.EXPORTS
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_reduce")
