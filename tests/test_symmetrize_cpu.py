"""The symmetrization without a GPU: the float64 restatement of rules 1-7 (diffusion/symmetrize.py) on the noisy crystals of
tests/symmetrize_cases.py -- exactness under the refined operations, idempotence, the known orbits, SymmetrySpec.from_template on
the noisy and on the symmetrized crystal, the copy of flagged crystals --, then argument validation, the statistics lines, the
file round trip, the parsers, the header, and the argument errors of sample(symmetrize=...)."""
import os
import re

import numpy as np
import pytest

from arreau_amd.diffusion import symmetrize as sz
from arreau_amd.diffusion import symmetry_search as ss
from arreau_amd.diffusion.diffusion_loss import SampleResult
from arreau_amd.diffusion.symmetry import SymmetrySpec
from tests import symmetrize_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(enumerate(cases.cases()))
CLEAN = [(b, c) for b, c in CASES if not c.flags]
ids = lambda bc: bc[1].name


def rows(b):
    first = cases.first_atoms()
    return slice(int(first[b]), int(first[b + 1]))


def mod1(d):
    return np.abs(d - np.rint(d))


@pytest.mark.parametrize("bc", CLEAN, ids=ids)
def test_output_is_exactly_symmetric_in_float64(bc):
    b, case = bc
    ref, found = cases.reference(), cases.search_reference()
    assert int(ref.flags[b]) == 0 and int(found.n_ops[b]) == case.n_ops
    ops = sz.refined_operations(ref, b)
    assert len(ops) == case.n_ops
    stored = [(ss.decode_rotation(int(c)), t) for c, t in zip(found.ops_rotation[b, :case.n_ops], found.ops_translation[b, :case.n_ops])]
    L_in, L_out = case.lattice.astype(np.float64), ref.lattice[b]
    before = ss.operation_residuals(case.frac, L_in, case.types, stored).max()
    after = max(ss.operation_residuals(ref.frac_out[rows(b)], L, case.types, ops).max() for L in (L_in, L_out))
    print(f"{case.name}: residual {before:.3e} A under the found operations, {after:.3e} A after, under the refined ones")
    assert after < 1e-10
    if case.n_ops > 1 and case.n > 1:
        assert 1e-4 < before <= cases.SYMPREC / 2  # the noise level
    G = L_out @ L_out.T
    for W, _ in ops:
        assert np.abs(W.T @ G @ W - G).max() < 1e-10 * G.max()
    # the rebuilt cell holds the lengths and angles it was rebuilt from, in the sampler's orientation (c along z, a in the xz plane)
    ln, ang = sz.params_of_metric(G)
    assert np.allclose(ln, ref.lengths[b], rtol=1e-12) and np.allclose(ang, ref.angles[b], atol=1e-12)
    assert L_out[0, 1] == 0.0 and L_out[2, 0] == 0.0 and L_out[2, 1] == 0.0


@pytest.mark.parametrize("bc", CLEAN, ids=ids)
def test_known_orbits(bc):
    b, case = bc
    ref = cases.reference()
    orbit, size, order = ref.orbit[rows(b)], ref.orbit_size[rows(b)], ref.site_order[rows(b)]
    leaders = np.nonzero(orbit == np.arange(case.n))[0]
    assert int(ref.n_orbits[b]) == len(leaders) == len(case.orbit_sizes)
    assert tuple(sorted(size[leaders].tolist())) == case.orbit_sizes
    assert (size * order == case.n_ops).all() and (orbit <= np.arange(case.n)).all()
    for l in leaders:  # an orbit holds one species, and as many atoms as its size says
        members = np.nonzero(orbit == l)[0]
        assert len(members) == size[l] and (size[members] == size[l]).all() and len(set(case.types[members].tolist())) == 1
    part = ref.partner[:case.n_ops, rows(b)]
    assert (np.sort(part, axis=1) == np.arange(case.n)[None, :]).all() and (ref.partner[case.n_ops:, rows(b)] == -1).all()
    assert float(ref.max_displacement[b]) >= float(ref.rms_displacement[b]) >= 0.0
    if case.n_ops > 1 and case.n > 1:
        assert 1e-4 < float(ref.max_displacement[b]) < cases.SYMPREC


def test_expected_values_of_the_table():
    by = {c.name: (b, c) for b, c in CASES}
    ref = cases.reference()
    b, c = by["rock salt"]
    assert (c.n, c.n_ops, c.orbit_sizes) == (8, 192, (4, 4)) and set(ref.site_order[rows(b)].tolist()) == {48}
    b, c = by["Fm-3m general position"]
    assert (c.n, c.orbit_sizes) == (192, (192,)) and set(ref.site_order[rows(b)].tolist()) == {1}
    b, c = by["P2_1/c, 65 orbits"]
    assert c.n == 260 > ss.STAGED_ATOMS and int(ref.n_orbits[b]) == 65
    b, c = by["Pnma 4c + 8d"]
    assert sorted(set(zip(ref.orbit_size[rows(b)].tolist(), ref.site_order[rows(b)].tolist()))) == [(4, 2), (8, 1)]
    b, c = by["R-3m, hexagonal cell"]
    assert sorted(set(zip(ref.orbit_size[rows(b)].tolist(), ref.site_order[rows(b)].tolist()))) == [(3, 12), (6, 6)]
    b, c = by["rock salt 2x1x1"]
    assert int(cases.search_reference().n_translations[b]) == 8 and set(ref.site_order[rows(b)].tolist()) == {16}
    assert int(cases.search_reference().flags[by["rock salt 2x2x2 (the search overflows)"][0]]) == ss.OVERFLOW
    assert int(cases.search_reference().flags[by["cell far below symprec (the search is ambiguous)"][0]]) == ss.AMBIGUOUS


@pytest.mark.parametrize("bc", [(b, c) for b, c in CLEAN if c.n <= 16], ids=ids)
def test_idempotence(bc):
    """The symmetrized crystal, rounded to float32 and searched and symmetrized again, stays where it is within that rounding."""
    b, case = bc
    ref = cases.reference()
    again = sz.symmetrize_reference_f64(ref.frac_out[rows(b)].astype(np.float32), ref.lattice[b:b + 1].astype(np.float32), [case.n],
                                        case.types, cases.PARAMS)
    assert int(again.flags[0]) == 0 and np.array_equal(again.orbit, ref.orbit[rows(b)]) and np.array_equal(again.orbit_size, ref.orbit_size[rows(b)])
    assert mod1(again.frac_out - ref.frac_out[rows(b)]).max() < 1e-6 and float(again.max_displacement[0]) < 1e-5
    assert np.abs(again.lengths[0] - ref.lengths[b]).max() < 1e-5 and np.abs(again.angles[0] - ref.angles[b]).max() < 1e-6


@pytest.mark.parametrize("bc", [(b, c) for b, c in CLEAN if c.generators is not None], ids=ids)
def test_from_template_rejects_the_noisy_crystal_and_accepts_the_symmetrized_one(bc):
    b, case = bc
    ref = cases.reference()
    assert np.abs(case.frac - case.ideal).max() > 1e-4
    with pytest.raises(ValueError, match="matches no template atom within"):
        SymmetrySpec.from_template(case.frac.astype(np.float64), case.generators, case.system)
    spec = SymmetrySpec.from_template(ref.frac_out[rows(b)], case.generators, case.system)
    assert spec.order == case.n_ops and tuple(sorted(len(o) for o in spec.orbits)) == case.orbit_sizes
    assert sorted(min(o) for o in spec.orbits) == sorted(set(ref.orbit[rows(b)].tolist()))


@pytest.mark.parametrize("bc", [(b, c) for b, c in CASES if c.flags or c.n_ops == 1], ids=ids)
def test_flagged_and_identity_only_crystals_are_copied_through(bc):
    b, case = bc
    ref = cases.reference()
    assert int(ref.flags[b]) == case.flags
    with np.errstate(all="ignore"):
        w = case.frac - np.floor(case.frac)
        w[w >= 1] = 0
    assert np.array_equal(ref.frac_out[rows(b)].astype(np.float32).view(np.int32), w.view(np.int32))
    assert np.array_equal(ref.orbit[rows(b)], np.arange(case.n)) and int(ref.n_orbits[b]) == case.n
    assert (ref.orbit_size[rows(b)] == 1).all() and (ref.site_order[rows(b)] == 1).all()
    assert ref.max_displacement[b] == 0 and ref.rms_displacement[b] == 0
    if case.flags:
        assert not ref.ops_translation[b].any() and (ref.partner[:, rows(b)] == -1).all()
        ln, ang = sz.params_of_metric(case.lattice.astype(np.float64) @ case.lattice.astype(np.float64).T)
        assert np.array_equal(ref.lengths[b], ln) and np.array_equal(ref.angles[b], ang)


def test_a_partner_map_that_is_no_permutation_is_flagged():
    frac, L, ty = cases.not_a_permutation()
    found = ss.symmetry_reference_f64(frac, L[None], [4], ty, cases.PARAMS.search())
    assert int(found.n_ops[0]) == 2 and int(found.flags[0]) == 0 and ss.point_group_name(found.point_group[0]) == "m"
    ref = sz.symmetrize_reference_f64(frac, L[None], [4], ty, cases.PARAMS, found=found)
    assert int(ref.flags[0]) == sz.NOT_A_PERMUTATION and np.array_equal(ref.orbit, np.arange(4)) and not ref.ops_translation.any()
    assert np.array_equal(ref.frac_out.astype(np.float32), frac) and int(ref.n_orbits[0]) == 4


# --------------------------------------------------------------------------------------------------- argument validation
def test_params_and_resolve():
    assert sz.resolve(None) is None and sz.resolve(False) is None and sz.resolve(True) == sz.SymmetrizeParams()
    p = sz.SymmetrizeParams(symprec=0.05, max_ops=48)
    assert sz.resolve(p) is p and (sz.SymmetrizeParams().symprec, sz.SymmetrizeParams().max_ops) == (0.1, 192)
    assert p.search() == ss.SymmetrySearchParams(symprec=0.05, max_ops=48)
    for bad in (0, float("nan"), "a", -1.0, True, float("inf")):
        with pytest.raises(ValueError, match="symprec"):
            sz.SymmetrizeParams(symprec=bad)
    for bad in (0, 4097, 1.5, True, "9"):
        with pytest.raises(ValueError, match="max_ops"):
            sz.SymmetrizeParams(max_ops=bad)
    for bad in (5, "yes", 0.1, ss.SymmetrySearchParams()):
        with pytest.raises(ValueError, match="symmetrize must be None, True or a SymmetrizeParams"):
            sz.resolve(bad)
    sz.check_shared_search(p, None), sz.check_shared_search(None, ss.SymmetrySearchParams()), sz.check_shared_search(p, p.search())
    with pytest.raises(ValueError, match="share one search"):
        sz.check_shared_search(p, ss.SymmetrySearchParams())
    assert sz.describe(0) == "ok" and sz.describe(sz.NO_GROUP | sz.CELL) == "CELL|NO_GROUP"


class NoEngine:
    def engine(self):
        raise AssertionError("the engine was touched")


def test_sample_rejects_a_bad_symmetrize_before_any_engine():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    loss = object.__new__(DiffusionLoss)
    loss.T = 100
    state = np.random.get_state()
    kw = dict(model=NoEngine(), z_table=None, num_atoms_per_sample=4, num_samples_in_batch=2)
    with pytest.raises(ValueError, match="symmetrize must be None, True or a SymmetrizeParams"):
        DiffusionLoss.sample(loss, symmetrize=5, **kw)
    with pytest.raises(ValueError, match="share one search"):
        DiffusionLoss.sample(loss, symmetrize=sz.SymmetrizeParams(symprec=0.05), find_symmetry=True, **kw)
    with pytest.raises(ValueError, match="share one search"):
        DiffusionLoss.sample(loss, symmetrize=True, find_symmetry=ss.SymmetrySearchParams(max_ops=48), **kw)
    assert np.array_equal(np.random.get_state()[1], state[1])  # nothing drawn
    assert SampleResult().symmetrized is None


def test_command_line_parsers():
    from arreau_amd import generate, screen
    for parser in (generate.build_parser(), screen.build_parser()):
        flags = {s for a in parser._actions for s in a.option_strings}
        assert {"--symmetrize", "--symprec"} <= flags
    args = screen.build_parser().parse_args(["f.npz", "--symmetrize", "--reduce_cell", "--symprec", "0.05", "--out", "s.npz"])
    assert args.symmetrize and args.reduce_cell and generate.instrument_params("symmetrize", args, None) == sz.SymmetrizeParams(symprec=0.05)
    assert not screen.build_parser().parse_args(["f.npz"]).symmetrize
    errors = []
    args.symprec = -1.0
    generate.instrument_params("symmetrize", args, errors.append)
    assert errors and "symmetrize" in errors[0]


def test_header_declares_the_entry_point_and_the_flags():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        text = fh.read()
    assert "int arreau_crystal_symmetrize(const float* d_frac, const int32_t* d_types, const float* d_lattice" in text
    assert "typedef struct arreau_symmetrize_result" in text
    defs = {k: int(v) for k, v in re.findall(r"#define ARREAU_SYMZ_(\w+) (\d+)", text)}
    assert defs == dict(NONFINITE=sz.NONFINITE, CELL=sz.CELL, EMPTY=sz.EMPTY, NO_GROUP=sz.NO_GROUP, NOT_A_PERMUTATION=sz.NOT_A_PERMUTATION)
    fields = re.search(r"typedef struct arreau_symmetrize_result \{(.*?)\} arreau_symmetrize_result;", text, re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == sz.RESULT_KEYS
    from arreau_amd import _hip
    assert tuple(n for n, _ in _hip.SymmetrizeResultC._fields_) == sz.RESULT_KEYS and "arreau_crystal_symmetrize" in _hip.EXPORTS


def _as_sample_arrays(ref):
    out = {k: getattr(ref, k) for k in sz.SYMMETRIZED_KEYS if k != "frac_x"}
    out["frac_x"] = ref.frac_out
    return out


def test_statistics_lines_and_the_file_round_trip(tmp_path):
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results, select_crystals
    sym = _as_sample_arrays(cases.reference())
    lines = sz.summary_lines([sz.stats_of(sym, 0)])
    assert lines[0].startswith("symmetrize rank 0: symmetrized 8 / attempted 12; orbits 1: 2, 2: 4, 5: 1, 65: 1; max displacement 0.0")
    assert lines[0].endswith(" A; flags NONFINITE 1, EMPTY 1, NO_GROUP 2") and lines[1].startswith("symmetrize total: symmetrized 8 / attempted 12")
    frac, lattice, counts, types = cases.batch()
    num = np.array(counts, dtype=np.int64)
    res = SampleResult(frac_x=frac.astype(np.float64), atomic_numbers=types.astype(np.float64), lattice=lattice.astype(np.float64),
                       num_atoms=num, idx_start=np.cumsum(num) - num, symmetrized=sym)
    back = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "s.npz")))
    assert set(back.symmetrized) == set(sz.SYMMETRIZED_KEYS)
    for k in sz.SYMMETRIZED_KEYS:
        assert np.array_equal(back.symmetrized[k], sym[k], equal_nan=True), k
    res.symmetrized = None
    plain = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "p.npz")))
    assert plain.symmetrized is None and not any(k.startswith("symmetrized_") for k in np.load(str(tmp_path / "p.npz")).files)
    res.symmetrized = sym
    keep = np.zeros(len(num), dtype=bool)
    keep[[0, 3]] = True
    some = select_crystals(res, keep)
    assert some.symmetrized["frac_x"].shape == (8 + 12, 3) and some.symmetrized["n_orbits"].tolist() == [2, 2]
    both = concat_results([some, some])
    assert both.symmetrized["orbit"].shape == (40,) and both.symmetrized["flags"].tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="symmetrized"):
        save_sample_results_to_hdf5(SampleResult(frac_x=res.frac_x, atomic_numbers=res.atomic_numbers, lattice=res.lattice, num_atoms=num,
                                                 idx_start=res.idx_start, symmetrized={k: v for k, v in sym.items() if k != "orbit"}),
                                    str(tmp_path / "bad.npz"))


def test_the_device_path_fails_loudly_without_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # (on a machine with a GPU too: the product's own check)
    from arreau_amd import _hip
    with pytest.raises(_hip.ArreauHipError, match="no CPU fallback"):
        sz.symmetrize(torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
