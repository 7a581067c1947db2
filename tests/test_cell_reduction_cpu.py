"""The cell reduction without a GPU: the float64 restatement (diffusion/cell_reduction.py) on the constructed crystals of
tests/cell_reduction_cases.py -- known multiplicities and cells, det(transform) = 1 / m, equal volumes, the reduced atoms expanded
by the translations reproduce the input, reducing a reduced crystal is the identity, skewed bases reduce to the same lengths and
angles -- every case under its own guard; the same invariants on `size_cases()` (63 to 264 atoms, face- and R-centred cells, 27
and 64 translations, two rounds of 256 atoms), each supercell's reduced cell against that of its own primitive crystal, the
flagged crystals (65 translations, an open closure, 261 atoms, a NaN) and a test of what those cases reach; the argument errors of CellReductionParams, resolve and sample(reduce_cell=...); the
command-line parsers and the loud failure of the device path without a GPU."""
import numpy as np
import pytest

from arreau_amd.diffusion import cell_reduction as cr
from arreau_amd.diffusion import crystal_batch as cb
from tests import cell_reduction_cases as cases

NAMES = list(cases.cases())


def test_every_family_is_there_and_guarded():
    assert len(NAMES) == 10 and sum(n.startswith("P1 skew") for n in NAMES) == len(cases.SKEWS)
    for name in NAMES:
        case = cases.cases()[name]
        mg = cases.reference(case).margins[0]
        assert sum(len(v) for v in mg.values()) > 0
        ratio = cr.guard_ratio(mg)
        print(f"{name}: smallest margin / bound {ratio:.3g}")
        assert ratio > cr.GUARD and cr.guarded(mg), name  # no case is skipped


def check_invariants(case):
    name = case.name
    ref = cases.reference(case)
    m, n_out = int(ref.multiplicity[0]), int(ref.n_out[0])
    assert int(ref.flags[0]) == 0 and m == case.multiplicity == int(ref.n_translations[0]) and n_out * m == case.n
    L, T, Lr = case.lattice.astype(np.float64), ref.transform[0], ref.lattice_out[0]
    assert abs(np.linalg.det(T) - 1.0 / m) < 1e-12 and np.allclose(T * m, np.rint(T * m), atol=1e-12)
    assert np.linalg.det(Lr) > 0 and abs(np.linalg.det(Lr) - abs(np.linalg.det(L)) / m) < 1e-9 * abs(np.linalg.det(L))
    assert np.array_equal(np.rint(T @ ref.inverse[0]), np.eye(3))
    ln = np.linalg.norm(Lr, axis=1)
    assert (np.diff(ln) >= -1e-12).all()  # the shortest first
    # the reduced atoms, expanded by the lattice of the reduced cell, reproduce every input atom within symprec
    xr, tr = ref.frac_out[:n_out], ref.types_out[:n_out]
    w = case.frac.astype(np.float64)
    for i in range(case.n):
        d = cr.min_image_distance((w[i] @ ref.inverse[0].astype(np.float64))[None, :] - xr[tr == case.types[i]], Lr)
        assert d.min() <= case.params.symprec, (name, i)
    assert sorted(ref.keep[:n_out]) == list(ref.keep[:n_out]) and (ref.keep[n_out:] == -1).all()
    # reducing the reduced crystal is the identity, up to the bounds
    again = cr.reduce_reference_f64(xr.astype(np.float32), Lr[None].astype(np.float32), [n_out], tr, case.params)
    assert cr.guarded(again.margins[0]), name
    assert int(again.multiplicity[0]) == 1 and int(again.flags[0]) == 0 and np.array_equal(again.transform[0], np.eye(3))
    assert np.array_equal(again.keep[:n_out], np.arange(n_out))
    assert np.abs(again.lattice_out[0] - Lr).max() <= 2.0 * cr.lattice_bound(T, L)
    d = again.frac_out - xr
    assert np.abs(d - np.rint(d)).max() <= 2.0 * cr.position_bound(ref.inverse[0])


@pytest.mark.parametrize("name", NAMES)
def test_invariants(name):
    check_invariants(cases.cases()[name])


def test_rock_salt_reduces_to_the_primitive_fcc_cell():
    for reps in ((1, 1, 1), (2, 1, 1), (2, 2, 2)):
        ref = cases.reference(cases.cases()["rock salt %dx%dx%d" % reps])
        assert int(ref.n_out[0]) == 2 and sorted(ref.types_out[:2]) == [11, 17]
        assert abs(np.linalg.det(ref.lattice_out[0]) - cases.A_NACL ** 3 / 4) < 1e-4
        assert np.allclose(np.linalg.norm(ref.lattice_out[0], axis=1), cases.A_NACL / np.sqrt(2), atol=1e-5)
        d = cr.min_image_distance((ref.frac_out[1] - ref.frac_out[0])[None, :], ref.lattice_out[0])
        assert abs(float(d[0]) - cases.A_NACL / 2) < 1e-5  # sodium to chlorine


def test_skewed_bases_reduce_to_the_cell_of_the_unskewed_crystal():
    want_len, want_cos = cases.lengths_angles(cases.reference(cases.cases()["P1"]).lattice_out[0])
    assert np.allclose(want_len, [4.1, 5.3, 6.2], atol=1e-5)
    for k in range(len(cases.SKEWS)):
        ref = cases.reference(cases.cases()[f"P1 skew {k}"])
        got_len, got_cos = cases.lengths_angles(ref.lattice_out[0])
        assert np.allclose(got_len, want_len, atol=1e-4) and np.allclose(got_cos, want_cos, atol=1e-5), k
        assert int(ref.selling_steps[0]) > 3 and np.abs(ref.transform[0]).max() > 1


def test_centred_cells():
    for name, t in (("body-centred", (0.5, 0.5, 0.5)), ("base-centred", (0.5, 0.5, 0.0))):
        case = cases.cases()[name]
        ref = cases.reference(case)
        L = case.lattice.astype(np.float64)
        # the centring vector is a lattice vector of the reduced cell
        x = np.linalg.solve(ref.lattice_out[0].T, np.array(t) @ L)
        assert np.allclose(x, np.rint(x), atol=1e-6) and int(ref.multiplicity[0]) == 2 and ref.keep[:2].tolist() == [0, 1]


# ------------------------------------------------------------- past 16 atoms: rounds, 64 translations, closure (size_cases)
def test_every_size_case_is_there_and_guarded():
    assert tuple(cases.size_cases()) == cases.SIZE_NAMES and tuple(cases.size_flag_cases()) == cases.SIZE_FLAG_NAMES
    for name, case in cases.size_cases().items():
        mg = cases.reference(case).margins[0]
        assert sum(len(v) for v in mg.values()) > 0
        ratio = cr.guard_ratio(mg)
        print(f"{name}: n {case.n} smallest margin / bound {ratio:.3g}")
        assert ratio > cr.GUARD and cr.guarded(mg), name  # no case is skipped


@pytest.mark.parametrize("name", cases.SIZE_NAMES)
def test_invariants_of_the_size_cases(name):
    case = cases.size_cases()[name]
    check_invariants(case)
    if case.multiplicity == 1:
        assert np.array_equal(cases.reference(case).keep, np.arange(case.n))


def test_supercells_reduce_to_the_cell_of_their_primitive_crystal():
    """No restatement of the supercell enters the expectation: the reduced cell of a supercell against the reduced cell of the
    crystal it was built from.  Both are float64 results from float32-rounded cells, and the two roundings differ: a component of
    a reduced vector moves by at most sum_k |T_rk| u / 2 |L_kd|, a sixteenth of lattice_bound, and a length by no more than
    sqrt(3) times that, so lengths agree within twice the two crystals' lattice bounds; a cosine moves by at most the two
    vectors' relative changes, 2 x that tolerance / the shortest length, and is given twice that."""
    for name, prim in cases.size_primitives().items():
        case = cases.size_cases()[name]
        ref, want = cases.reference(case), cases.reference(prim)
        assert int(want.multiplicity[0]) == 1 and int(want.flags[0]) == 0 and int(ref.flags[0]) == 0, name
        tol = 2.0 * (cr.lattice_bound(ref.transform[0], case.lattice.astype(np.float64)) +
                     cr.lattice_bound(want.transform[0], prim.lattice.astype(np.float64)))
        got_len, got_cos = cases.lengths_angles(ref.lattice_out[0])
        want_len, want_cos = cases.lengths_angles(want.lattice_out[0])
        d_len, d_cos = float(np.abs(got_len - want_len).max()), float(np.abs(got_cos - want_cos).max())
        print(f"{name}: |length - primitive's| {d_len:.3e} (tolerance {tol:.3e}) |cos - primitive's| {d_cos:.3e} "
              f"(tolerance {4.0 * tol / want_len[0]:.3e})")
        assert d_len <= tol and d_cos <= 4.0 * tol / want_len[0], name
        n_out = int(ref.n_out[0])
        assert n_out == prim.n and int(ref.multiplicity[0]) * prim.n == case.n, name
        assert sorted(ref.types_out[:n_out]) == sorted(prim.types), name
    for name, m in (("face-centred", 4), ("R-centred", 3)):
        ref = cases.reference(cases.size_cases()[name])
        assert int(ref.multiplicity[0]) == m and int(ref.n_out[0]) == 2, name


def test_size_flag_cases_on_the_restatement():
    for name, fc in cases.size_flag_cases().items():
        case, ref = fc.case, cases.reference(fc.case)
        assert int(ref.flags[0]) == fc.flags and int(ref.n_translations[0]) == fc.n_translations, (name, cr.describe(ref.flags[0]))
        assert int(ref.multiplicity[0]) == 1 and int(ref.n_out[0]) == case.n and np.array_equal(ref.transform[0], np.eye(3)), name
        assert np.array_equal(ref.keep, np.arange(case.n)) and np.array_equal(ref.types_out, case.types), name
        assert np.array_equal(ref.frac_out, case.frac.astype(np.float64), equal_nan=True), name
        assert np.array_equal(ref.lattice_out[0], case.lattice.astype(np.float64)), name
    want = {"65 translations": (cr.AMBIGUOUS, 65), "open closure": (cr.AMBIGUOUS, 3), "261 atoms": (cr.AMBIGUOUS, 4),
            "nan in atom 258": (cr.NONFINITE, 0)}
    assert {k: (v.flags, v.n_translations) for k, v in cases.size_flag_cases().items()} == want


def test_the_size_cases_reach_what_they_are_for():
    """Computed from the restatement's results, so that the cases cannot decay into ones the kernel's second trips never see."""
    rows = []
    for case in list(cases.size_cases().values()) + [fc.case for fc in cases.size_flag_cases().values()]:
        ref = cases.reference(case)
        finite = bool(np.isfinite(case.frac).all())
        species, cnt = np.unique(case.types, return_counts=True)
        rare = np.nonzero(case.types == species[int(np.argmin(cnt))])[0] if finite else np.empty(0, np.int64)
        flags, n_out = int(ref.flags[0]), int(ref.n_out[0])
        rows.append(dict(name=case.name, n=case.n, m=int(ref.multiplicity[0]), nt=int(ref.n_translations[0]), flags=flags,
                         rare_n=int(rare.size), rare_max=int(rare.max()) if rare.size else -1, rare_min=int(rare.min()) if rare.size else -1,
                         last_kept=int(ref.keep[n_out - 1]) if flags == 0 else -1))
    reach = {
        "n of 63, 64, 65 and at least 257": {63, 64, 65} <= {r["n"] for r in rows} and any(r["n"] >= 257 and not r["flags"] for r in rows),
        # (that only the first block of 64 atoms rejects some of them in one crystal, only the last block in another, is
        # asserted where those cases are built)
        "candidates rejected among more than 64 atoms, none accepted": sum(r["n"] > 64 and r["rare_n"] > 8 and r["nt"] == 1 and not r["flags"]
                                                                           for r in rows) >= 2,
        "an m of 64":any(r["m"] == 64 == cr.MAX_TRANSLATIONS and not r["flags"] for r in rows),
        "65 translations flagged AMBIGUOUS": any(r["nt"] == 65 and r["flags"] == cr.AMBIGUOUS for r in rows),
        "a rarest-species index of 256 or more": any(r["rare_max"] >= 256 and not r["flags"] for r in rows),
        "the rarest species in both rounds, m > 1": any(r["rare_min"] < 256 <= r["rare_max"] and r["m"] > 1 for r in rows),
        "keep[n_out - 1] >= 256": any(r["last_kept"] >= 256 and r["m"] > 1 for r in rows),
        "an odd m": any(r["m"] % 2 == 1 and r["m"] > 1 for r in rows),
        "a flagged crystal of more than 256 atoms": any(r["flags"] and r["n"] > 256 for r in rows),
        "AMBIGUOUS with n % n_translations == 0": any(r["flags"] == cr.AMBIGUOUS and 0 < r["nt"] <= cr.MAX_TRANSLATIONS and r["n"] % r["nt"] == 0
                                                      for r in rows),
    }
    for what, there in reach.items():
        print(f"{what}: {'yes' if there else 'NO'}")
    assert all(reach.values()), [k for k, v in reach.items() if not v]


def test_flags_of_the_restatement():
    f, L, t = cases.rock_salt((1, 1, 1))
    bad = f.copy()
    bad[0, 0] = np.inf
    ref = cr.reduce_reference_f64(np.concatenate([bad, f]), np.stack([L, np.zeros((3, 3))]), [2, 2], np.concatenate([t, t]))
    assert ref.flags.tolist() == [cr.NONFINITE, cr.CELL] and ref.multiplicity.tolist() == [1, 1] and ref.keep.tolist() == [0, 1, 0, 1]
    assert cr.describe(cr.NONFINITE | cr.AMBIGUOUS) == "NONFINITE|AMBIGUOUS" and cr.describe(0) == "ok"
    ref = cr.reduce_reference_f64(np.empty((0, 3)), L[None], [0], np.empty(0))
    assert ref.flags.tolist() == [cr.EMPTY]


def test_header_constants_agree():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "arreau_hip.h")) as fh:
        defs = dict(re.findall(r"#define ARREAU_RED_(\w+) (\d+)", fh.read()))
    assert {k: int(v) for k, v in defs.items()} == dict(NONFINITE=cr.NONFINITE, CELL=cr.CELL, EMPTY=cr.EMPTY, AMBIGUOUS=cr.AMBIGUOUS,
                                                        NOT_CONVERGED=cr.NOT_CONVERGED, MAX_TRANSLATIONS=cr.MAX_TRANSLATIONS,
                                                        MAX_STEPS=cr.MAX_STEPS)


def test_compact_ragged_and_statistics():
    off, (a,) = cb.compact_ragged([0, 3, 5], [1, 2], np.arange(5) * 10)
    assert off.tolist() == [0, 1, 3] and a.tolist() == [0, 30, 40]
    st = [cr.stats_of({"multiplicity": [1, 2, 1], "flags": [0, 0, cr.AMBIGUOUS]}, 1), cr.stats_of({"multiplicity": [4], "flags": [0]}, 0)]
    lines = cr.summary_lines(st)
    assert lines[0] == "cell reduction rank 0: reduced 1 / attempted 1; multiplicity 4: 1; flags none"
    assert lines[2] == "cell reduction total: reduced 3 / attempted 4; multiplicity 1: 2, 2: 1, 4: 1; flags AMBIGUOUS 1"


# --------------------------------------------------------------------------------------------------- argument validation
def test_params_and_resolve():
    assert cr.resolve(None) is None and cr.resolve(False) is None and cr.resolve(True) == cr.CellReductionParams()
    p = cr.CellReductionParams(symprec=0.05)
    assert cr.resolve(p) is p and cr.CellReductionParams().symprec == 0.1
    for bad in (0, float("nan"), "a", -1.0, True, float("inf")):
        with pytest.raises(ValueError, match="symprec"):
            cr.CellReductionParams(symprec=bad)
    for bad in (5, "yes", 0.1):
        with pytest.raises(ValueError, match="reduce_cell must be None, True or a CellReductionParams"):
            cr.resolve(bad)


def test_sample_rejects_a_bad_reduce_cell_before_any_engine():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss, SampleResult
    loss = object.__new__(DiffusionLoss)
    with pytest.raises(ValueError, match="reduce_cell must be None, True or a CellReductionParams"):
        DiffusionLoss.sample(loss, model=None, z_table=None, num_atoms_per_sample=4, num_samples_in_batch=2, reduce_cell=5)
    assert SampleResult().reduced is None


def test_command_line_parsers():
    from arreau_amd import generate, screen
    for parser in (generate.build_parser(), screen.build_parser()):
        flags = {s for a in parser._actions for s in a.option_strings}
        assert {"--reduce_cell", "--symprec"} <= flags
    args = screen.build_parser().parse_args(["f.npz", "--reduce_cell", "--symprec", "0.05"])
    assert args.reduce_cell and generate.instrument_params("reduce_cell", args, None) == cr.CellReductionParams(symprec=0.05)
    args = generate.build_parser().parse_args(["--model_path", "m.ckpt", "--reduce_cell"]) if False else args
    errors = []
    args.symprec = -1.0
    generate.instrument_params("reduce_cell", args, errors.append)
    assert errors and "cell reduction" in errors[0]


def test_the_device_path_fails_loudly_without_a_gpu(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (on a machine with a GPU too: the product's own check)
    from arreau_amd import _hip, screen
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import save_sample_results_to_hdf5
    case = cases.cases()["body-centred"]
    num = np.array([case.n], dtype=np.int64)
    src = str(tmp_path / "crystals.npz")
    save_sample_results_to_hdf5(SampleResult(frac_x=case.frac.astype(np.float64), atomic_numbers=case.types.astype(np.float64),
                                             lattice=case.lattice[None].astype(np.float64), num_atoms=num, idx_start=num * 0), src)
    with pytest.raises((_hip.ArreauHipError, RuntimeError, AssertionError)):
        screen.main([src, "--reduce_cell", "--out", str(tmp_path / "reduced.npz")])
    assert not (tmp_path / "reduced.npz").exists()
    with pytest.raises(_hip.ArreauHipError, match="no CPU fallback"):
        cr.reduce_cells(torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_hip.ArreauHipError, match="no CPU fallback"):
        cr.reduce_sample_result(SampleResult(frac_x=case.frac, atomic_numbers=case.types, lattice=case.lattice[None], num_atoms=num), device="cpu")
