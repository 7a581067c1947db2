"""The symmetry search without a GPU: the float64 restatement of rules 1-6 on crystals with a known answer
(tests/symmetry_search_cases.py), the found operations against the closed groups, the generated point-group table and the header
the kernel includes, invariances, the rotation code, argument validation, `contains`, the statistics lines, the file round trip
and the argument errors of sample(find_symmetry=...)."""
import os

import numpy as np
import pytest

from arreau_amd.diffusion import symmetry_search as ss
from arreau_amd.diffusion.diffusion_loss import SampleResult
from arreau_amd.diffusion.symmetry import SymmetrySpec, close_group
from tests import symmetry_search_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(cases.base_cases()) + list(cases.shape_cases().values())[2:] + [cases.overflow_case()]


def _as_result(case, ref):
    """The restatement's namespace as the dict `contains` and `stats_of` read."""
    out = {k: getattr(ref, k) for k in ss.SYM_KEYS[:-1]}
    out["symprec"] = np.full(1, np.float32(case.params.symprec))
    out["lattice"] = case.lattice[None]
    return out


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_restatement_gives_the_expected_answer(case):
    ref = cases.reference(case)
    pg = int(ref.point_group[0])
    assert (int(ref.n_ops[0]), int(ref.n_translations[0]), ss.point_group_name(pg)) == (case.n_ops, case.n_translations, case.point_group)
    assert ss.crystal_system(pg) == ss.POINT_GROUP_SYSTEMS[ss.POINT_GROUP_NAMES.index(case.point_group)]
    assert int(ref.flags[0]) == case.flags
    stored = min(case.n_ops, case.params.max_ops)
    assert (ref.ops_rotation[0, :stored] >= 0).all() and (ref.ops_rotation[0, stored:] == -1).all()
    assert np.all(np.diff(ref.ops_rotation[0, :stored]) >= 0)  # code order
    assert ref.residual[0] == ref.ops_residual[0, :stored].max() or case.flags & ss.OVERFLOW
    assert ref.residual[0] <= case.params.symprec / 2


@pytest.mark.parametrize("case", [c for c in ALL if c.ops is not None and not c.flags], ids=lambda c: c.name)
def test_found_operations_are_the_closed_group(case):
    ref = cases.reference(case)
    result = _as_result(case, ref)
    assert len(case.ops) == case.n_ops == int(ref.n_ops[0])
    assert ss.contains(result, 0, case.ops)
    # and nothing else: every found operation is one of the group's (equal counts and containment make the sets equal)
    L = case.lattice.astype(np.float64)
    for code, t in zip(ref.ops_rotation[0, :case.n_ops], ref.ops_translation[0, :case.n_ops]):
        W = ss.decode_rotation(int(code))
        near = [np.linalg.norm((lambda d: d - np.rint(d))(t - tg) @ L) for R, tg in case.ops if np.array_equal(R, W)]
        assert near and min(near) <= case.params.symprec


def test_point_group_table_and_header():
    table = ss.point_group_table()
    assert table.shape == (32, 10) and len({tuple(r) for r in table.tolist()}) == 32
    assert table.sum(axis=1).tolist() == [1, 2, 2, 2, 4, 4, 4, 8, 4, 4, 8, 8, 8, 8, 16, 3, 6, 6, 6, 12, 6, 6, 12, 12, 12, 12, 24, 12, 24,
                                          24, 24, 48]
    for k, (name, system, gens) in enumerate(ss.POINT_GROUPS):
        rotations = [R for R, _ in close_group(gens)]
        assert ss.classify(rotations, len(rotations), 1) == (k, 0), name
        assert ss.crystal_system(k) == system and ss.point_group_name(k) == name
    # the header beside the kernel is what the generator prints
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_point_group_table", os.path.join(ROOT, "tools", "gen_point_group_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ROOT, "arreau_amd", "csrc", "symfind_table.h")) as fh:
        assert fh.read() == gen.header_text()


def test_a_set_that_is_not_closed_is_not_a_group():
    m3m = [R for R, _ in close_group(cases.PM3M)]
    assert ss.classify(m3m[:-1], 47, 1) == (-1, ss.NOT_A_GROUP)
    four = [R for R, _ in close_group(["-y,x,z"])]
    assert ss.classify(four[:3], 3, 1) == (-1, ss.NOT_A_GROUP)       # 1, 4, 2 without the second fourfold rotation
    assert ss.classify(four, 5, 1) == (-1, ss.NOT_A_GROUP)           # n_ops != rotations x translations
    assert ss.classify([np.array([[1, 1, 0], [1, 0, 0], [0, 0, 1]])], 1, 1) == (-1, ss.NOT_A_GROUP)  # det -1, trace 2: no type
    assert ss.crystal_system(-1) == "none" and ss.point_group_name(-1) == "none"


def _discrete(ref):
    n = int(ref.n_ops[0])
    return (int(ref.n_lattice[0]), n, int(ref.n_translations[0]), int(ref.point_group[0]), int(ref.flags[0]),
            sorted(ref.ops_rotation[0, :n].tolist()))


@pytest.mark.parametrize("name", ["P2_1/c", "NaCl displaced", "perovskite", "R-3m rhombohedral axes displaced", "hcp"])
def test_invariance_of_the_discrete_outputs(name):
    case = {c.name: c for c in cases.base_cases()}[name]
    want = _discrete(cases.reference(case))
    rng = np.random.default_rng(5)
    perm = rng.permutation(case.n)
    f = case.frac.astype(np.float64)
    variants = {"permutation": (f[perm], case.types[perm]),
                "common translation": (f + rng.uniform(0, 1, 3)[None, :], case.types),
                "lattice translations of single atoms": (f + rng.integers(-2, 3, f.shape), case.types)}
    for what, (frac, types) in variants.items():
        ref = ss.symmetry_reference_f64(frac, case.lattice[None], [case.n], types, case.params)
        assert _discrete(ref) == want, what


def test_rotation_code_round_trip():
    assert ss.encode_rotation(np.eye(3, dtype=int)) == ss.IDENTITY_CODE
    assert ss.decode_rotation(0).tolist() == [[-1] * 3] * 3 and ss.decode_rotation(1)[0, 0] == 0
    for code in (0, 1, 3, 9840, ss.IDENTITY_CODE, ss.N_CODES - 1):
        assert ss.encode_rotation(ss.decode_rotation(code)) == code
    for R, _ in close_group(cases.PM3M):
        assert np.array_equal(ss.decode_rotation(ss.encode_rotation(R)), R)
    for bad in (-1, ss.N_CODES, 1.5, True):
        with pytest.raises(ValueError):
            ss.decode_rotation(bad)
    with pytest.raises(ValueError):
        ss.encode_rotation([[2, 0, 0], [0, 1, 0], [0, 0, 1]])


def test_argument_validation():
    assert ss.resolve(None) is None and ss.resolve(False) is None
    assert ss.resolve(True) == ss.SymmetrySearchParams() == ss.SymmetrySearchParams(0.1, 192)
    p = ss.SymmetrySearchParams(symprec=0.05, max_ops=7)
    assert ss.resolve(p) is p
    for bad in (1, "yes", 0.1):
        with pytest.raises(ValueError, match="find_symmetry"):
            ss.resolve(bad)
    for kw in (dict(symprec=0.0), dict(symprec=-1.0), dict(symprec=float("nan")), dict(symprec=float("inf")), dict(symprec="a"),
               dict(symprec=True), dict(max_ops=0), dict(max_ops=ss.MAX_OPS_CAP + 1), dict(max_ops=1.5), dict(max_ops=True)):
        with pytest.raises(ValueError):
            ss.SymmetrySearchParams(**kw)
    assert ss.describe(0) == "ok" and ss.describe(ss.OVERFLOW | ss.NOT_A_GROUP) == "OVERFLOW|NOT_A_GROUP"


def test_flagged_inputs_in_the_restatement():
    c = {c.name: c for c in cases.base_cases()}["CsCl"]
    frac = np.concatenate([c.frac, c.frac, c.frac])
    frac[2, 1] = np.nan
    lattice = np.stack([c.lattice, c.lattice, np.zeros((3, 3), np.float32), c.lattice])
    ref = ss.symmetry_reference_f64(frac, lattice, [2, 2, 2, 0], np.tile(c.types, 3))
    assert ref.flags.tolist() == [0, ss.NONFINITE, ss.CELL, ss.EMPTY]
    assert ref.n_ops.tolist() == [48, 0, 0, 0] and ref.point_group.tolist() == [31, -1, -1, -1]
    assert np.isnan(ref.residual[1:]).all()
    # a 3 A cubic cell with symprec 4 A: the deviations are 0, 1.24, 2.2 and 3 A (pass), 6 and 9 A (fail)
    one = {c.name: c for c in cases.base_cases()}["one atom, cubic"]
    loose = ss.symmetry_reference_f64(one.frac, one.lattice[None], [1], one.types, ss.SymmetrySearchParams(symprec=4.0))
    assert loose.flags.tolist() == [ss.AMBIGUOUS] and loose.n_lattice[0] > 48 and loose.n_ops[0] == 0


def test_contains():
    by_name = {c.name: c for c in cases.base_cases()}
    nacl, p4 = by_name["NaCl displaced"], by_name["P4/mmm"]
    r = _as_result(nacl, cases.reference(nacl))
    assert ss.contains(r, 0, cases.FM3M) and ss.contains(r, 0, cases.PM3M) and ss.contains(r, 0, ["x,y,z"])
    assert ss.contains(r, 0, SymmetrySpec.general_positions(("-y,x,z", "-x,-y,-z"), 1, "tetragonal"))
    assert not ss.contains(r, 0, ["x+1/4,y,z"])           # a translation the crystal does not have
    r4 = _as_result(p4, cases.reference(p4))
    assert ss.contains(r4, 0, p4.ops) and not ss.contains(r4, 0, cases.PM3M)  # the threefold axis is missing
    assert not ss.contains(r4, 0, ["x-y,x,z"])             # an entry outside the cell's rotations
    tri = by_name["triclinic with inversion, one atom moved away"]
    assert not ss.contains(_as_result(tri, cases.reference(tri)), 0, ["-x,-y,-z"])


def test_stats_and_summary_lines():
    picks = [c for c in cases.base_cases() if c.name in ("triclinic", "NaCl", "CsCl", "hcp", "Pnma")]
    refs = [cases.reference(c) for c in picks]
    result = {"point_group": np.array([int(r.point_group[0]) for r in refs] + [-1]),
              "flags": np.array([int(r.flags[0]) for r in refs] + [ss.AMBIGUOUS])}
    st = ss.stats_of(result, rank=1)
    assert st["attempted"] == 6 and st["classified"] == 5 and st["rank"] == 1
    assert st["systems"] == {"triclinic": 1, "monoclinic": 0, "orthorhombic": 1, "tetragonal": 0, "trigonal": 0, "hexagonal": 1, "cubic": 2}
    assert st["point_groups"]["m-3m"] == 2 and st["point_groups"]["6/mmm"] == 1 and sum(st["point_groups"].values()) == 5
    assert st["flags"]["AMBIGUOUS"] == 1 and st["flags"]["OVERFLOW"] == 0
    lines = ss.summary_lines([st, ss.stats_of(result, rank=0)])
    assert [line.split(":")[0] for line in lines] == ["symmetry rank 0", "symmetry rank 1", "symmetry total"]
    assert "classified 10 / attempted 12" in lines[2] and "cubic 4" in lines[2] and "m-3m: 4" in lines[2] and "AMBIGUOUS 2" in lines[2]
    assert ss.format_stats(ss.stats_of({"point_group": np.empty(0), "flags": np.empty(0)})).endswith("none; point groups none; flags none")


def test_file_round_trip_and_concatenation(tmp_path):
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results, select_crystals, symmetry_lines
    picks = [c for c in cases.base_cases() if c.name in ("triclinic", "NaCl")]
    parts = []
    for c in picks:
        sym = _as_result(c, cases.reference(c))
        parts.append(SampleResult(frac_x=c.frac.astype(np.float64), atomic_numbers=c.types.astype(np.float64), lattice=c.lattice[None].astype(np.float64),
                                  idx_start=np.zeros(1, np.int64), num_atoms=np.array([c.n]), symmetry=sym))
    res = concat_results(parts)
    assert res.symmetry["ops_rotation"].shape == (2, 192) and res.symmetry["n_ops"].tolist() == [1, 192]
    name = save_sample_results_to_hdf5(res, str(tmp_path / "c.npz"))
    back = load_sample_results_from_hdf5(name)
    for k in ss.SYM_KEYS:
        assert np.array_equal(back.symmetry[k], res.symmetry[k]), k
    assert ss.contains(back.symmetry, 1, cases.FM3M) and not ss.contains(back.symmetry, 0, cases.FM3M)
    assert symmetry_lines(back, spec=cases.FM3M)[-1] == "symmetry: 1 / 2 crystals contain the requested group (|G| = 192)"
    assert select_crystals(back, [False, True]).symmetry["point_group"].tolist() == [31]
    plain = SampleResult(**{k: getattr(res, k) for k in ("frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms")})
    with np.load(save_sample_results_to_hdf5(plain, str(tmp_path / "p.npz"))) as z:
        assert not [k for k in z.files if k.startswith("sym_")]
    assert load_sample_results_from_hdf5(str(tmp_path / "p.npz")).symmetry is None


def test_sample_argument_errors_come_before_any_work():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    loss = object.__new__(DiffusionLoss)  # no model, no device: the argument check is the first statement that can fail
    for bad in ("yes", 3, 0.1, ss.SymmetrySearchParams):
        with pytest.raises(ValueError, match="find_symmetry must be None, True or a SymmetrySearchParams"):
            DiffusionLoss.sample(loss, model=None, z_table=None, num_atoms_per_sample=4, num_samples_in_batch=2, find_symmetry=bad)


def test_command_line_flags():
    from arreau_amd import generate, screen
    for parser in (generate.build_parser(), screen.build_parser()):
        flags = {a for action in parser._actions for a in action.option_strings}
        assert {"--find_symmetry", "--symprec"} <= flags
    args = screen.build_parser().parse_args(["f.npz", "--find_symmetry", "--symprec", "0.05"])
    assert generate.instrument_params("find_symmetry", args, None) == ss.SymmetrySearchParams(symprec=0.05)
    errors = []
    args.symprec = -1.0
    generate.instrument_params("find_symmetry", args, errors.append)
    assert errors and "symprec" in errors[0]
