"""The Ewald sum's rules on the CPU: the float64 restatement (arreau_amd/diffusion/ewald.py: ewald_reference) against the textbook
Madelung constants, the Wigner lattice, its own independence of the splitting parameter, its exact identities (E = (1 / 2) sum q
potential as summed, the potential in volts, the four parts, the scaling with the charges, translations, permutations, descriptions of one crystal), the batches
of tests/ewald_cases.py (what each is meant to reach, and that no crystal sits on a cut), the float32 mode's table and its n_pairs,
the parameters and the string form of the charges, and the host layer: ENERGIES / COMPLETE, the file round trip, select and concat,
the parsers, the summary lines, the header and the binding.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from arreau_amd import _hip
from arreau_amd.diffusion import ewald
from arreau_amd.diffusion.diffusion_loss import SampleResult
from tests import ewald_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
TIGHT = ewald.EwaldParams(charges=cases.CHARGES, accuracy=1e-12)
ALPHAS = (0.25, 0.35, 0.6)


def exact(crystal, params=TIGHT, **kw):
    """The float64 restatement of one (frac, cell, species) crystal taken as the float64 numbers it is."""
    f, L, z = crystal
    return ewald.ewald_reference(f, L[None], [len(z)], ewald.host_charges(z, params), params, exact_inputs=True, **kw)


def test_the_case_list_and_no_crystal_sits_on_a_cut():
    assert cases.BATCHES == ("textbook", "ragged", "large", "rounds", "rounds 0.25", "rounds 0.35", "shells", "flags", "range")
    assert set(ewald.F32_DEVIATION) == set(cases.BATCHES) and ewald.parse_charges(cases.CHARGES_STRING) == ewald.parse_charges(cases.CHARGES)
    for name in cases.BATCHES:
        bt, r = cases.reference(name)
        ok = (r.flags & ewald.INVALID_MASK) == 0
        assert (r.reciprocal_margin[ok] >= ewald.MARGIN_GUARD).all(), name  # no crystal is left out of the exact counts
        assert np.isnan(r.energy[~ok]).all() and (r.n_pairs[~ok] == 0).all() and (r.n_reciprocal[~ok] == 0).all()
        assert not np.isnan(r.energy[ok]).any() and (r.n_pairs[ok] > 0).all()
    bt, r = cases.reference("textbook")
    assert bt.counts == [2, 8, 8, 12, 2, 16, 1] and r.flags.tolist() == [0] * 6 + [ewald.CHARGED]
    bt, r = cases.reference("ragged")
    assert len(bt.counts) == 70 and min(bt.counts) == 1 and max(bt.counts) == 24 and set(bt.species.tolist()) == set(cases.RAGGED_SPECIES)
    assert 35 < int((r.flags == ewald.CHARGED).sum()) < 70 and set(r.flags.tolist()) == {0, ewald.CHARGED}  # most are not neutral
    bt, r = cases.reference("large")
    assert bt.counts == [257] and r.flags[0] in (0, ewald.CHARGED)
    # several reciprocal rounds at alpha 0.6, one at the two others; the same crystal
    r = cases.reference("rounds")[1]
    assert r.entries[0] > 2 * ewald.ROUND and r.rounds[0] == 3 and r.alpha[0] == 0.6
    assert [cases.reference(n)[1].rounds[0] for n in ("rounds 0.25", "rounds 0.35")] == [1, 1]
    assert np.array_equal(cases.batch("rounds").frac, cases.batch("rounds 0.25").frac)
    # exactly max_shells images, and one more
    r32 = cases.reference32("shells")
    assert r32.images.tolist() == [[8, 2, 2], [0, 0, 0]] and r32.flags.tolist() == [0, ewald.CELL] and ewald.MAX_SHELLS == 8
    assert cases.reference("flags")[1].flags.tolist() == cases.FLAGS_EXPECTED
    # max_index one below the need
    bt, r = cases.reference("range")
    assert r.flags.tolist() == [ewald.RANGE] and bt.params.max_index == 2
    enough = ewald.ewald_reference(bt.frac, bt.lattice, bt.counts, cases.charges(bt), ewald.EwaldParams(charges=cases.CHARGES, max_index=3))
    assert enough.flags.tolist() == [0] and enough.box[0].tolist() == [3, 3, 3]


def test_madelung_constants():
    crystals = dict(zip(cases.TEXTBOOK_NAMES, cases.textbook_crystals()))
    for name, r0, units, value, tol in cases.MADELUNG:
        r = exact(crystals[name])
        got = ewald.madelung({"energy": r.energy}, 0, r0, units)
        assert r.flags[0] == 0 and abs(got - value) <= tol, (name, got, value)


def test_descriptions_of_nacl_agree_per_formula_unit():
    crystals = dict(zip(cases.TEXTBOOK_NAMES, cases.textbook_crystals()))
    per = [exact(crystals[n]).energy[0] / u for n, u in (("nacl", 4), ("nacl_primitive", 1), ("nacl_doubled", 8))]
    assert max(per) - min(per) <= 1e-9, per
    assert abs(per[0] - (-ewald.K * 1.7475645946 / (cases.A_NACL / 2.0))) <= 1e-8


def test_the_wigner_lattice():
    r = exact(cases.textbook_crystals()[-1])
    assert r.flags[0] == ewald.CHARGED and r.net_charge[0] == 1.0 and abs(r.energy[0] / ewald.K - cases.WIGNER) <= 1e-7
    assert r.background[0] < 0.0 and r.volume[0] == 1.0


def test_the_result_does_not_depend_on_alpha():
    """Energy and every potential over alpha in {0.25, 0.35, 0.6} at accuracy 1e-12, to 1e-7 of |E_self| (the energies) and of the
    potential's own scale (K 2 alpha max|q| / sqrt(pi), taken at the rule's alpha).  The unit cube at these alphas needs more
    images than max_shells allows: the yardstick runs `unbounded` there, which lifts the kernel's two caps and nothing else."""
    crystals = cases.textbook_crystals() + [tuple(np.asarray(a, dtype=F64) if i < 2 else a for i, a in enumerate(cases.random_crystal(s)))
                                            for s in cases.RAGGED_FIVE]
    for c in crystals:
        base = exact(c)
        q = np.abs(ewald.host_charges(c[2], TIGHT)).max()
        e_scale, p_scale = abs(base.self[0]), ewald.K * 2.0 * base.alpha[0] * q / math.sqrt(math.pi)
        for a in ALPHAS:
            r = exact(c, ewald.EwaldParams(charges=cases.CHARGES, accuracy=1e-12, alpha=a), unbounded=True)
            assert r.alpha[0] == a and (r.flags[0] & ewald.INVALID_MASK) == 0
            assert abs(r.energy[0] - base.energy[0]) <= 1e-7 * e_scale, (c[2], a)
            assert np.abs(r.potential - base.potential).max() <= 1e-7 * p_scale, (c[2], a)


def test_exact_identities():
    bt, r = cases.reference("ragged")
    q = cases.charges(bt).astype(F64)
    for b in range(len(bt.counts)):
        at = cases.atoms_of(bt, b)
        total = 0.0
        for qa, pa in zip(q[at], r.potential[at]):  # E = (1 / 2) sum q potential (volts: K is inside), exactly as summed
            total += qa * pa
        assert r.energy[b] == 0.5 * total
        parts = r.real[b] + r.reciprocal[b] + r.self[b] + r.background[b]
        assert abs(parts - r.energy[b]) <= 64 * np.finfo(F64).eps * (abs(r.real[b]) + abs(r.reciprocal[b]) + abs(r.self[b]) + abs(r.background[b]))
        assert r.net_charge[b] == q[at].sum() and r.self[b] < 0.0 and (r.background[b] <= 0.0)
        assert (r.background[b] == 0.0) == (q[at].sum() == 0.0)
    # all charges times c: E times c^2 (c = 2: exact in binary)
    one = cases.single(bt, cases.RAGGED_MIDDLE)
    a = ewald.ewald_reference(one.frac, one.lattice, one.counts, cases.charges(one), one.params)
    b2 = ewald.ewald_reference(one.frac, one.lattice, one.counts, 2.0 * cases.charges(one), one.params)
    assert b2.energy[0] == 4.0 * a.energy[0] and np.array_equal(b2.potential, 2.0 * a.potential)
    c3 = ewald.ewald_reference(one.frac, one.lattice, one.counts, 3.0 * cases.charges(one), one.params)
    assert abs(c3.energy[0] - 9.0 * a.energy[0]) <= 1e-13 * abs(a.self[0]) * 9.0


def test_translation_and_permutation():
    f, L, z = (np.asarray(a, dtype=F64) if i < 2 else a for i, a in enumerate(cases.random_crystal(11, 9)))
    base = exact((f, L, z))
    moved = exact((f + [0.31, -0.77, 1.4], L, z))
    scale = abs(base.self[0])
    assert abs(moved.energy[0] - base.energy[0]) <= 1e-10 * scale and np.abs(moved.potential - base.potential).max() <= 1e-10 * scale
    perm = np.random.default_rng(5).permutation(len(z))
    mixed = exact((f[perm], L, [z[i] for i in perm]))
    assert abs(mixed.energy[0] - base.energy[0]) <= 1e-12 * scale and np.abs(mixed.potential - base.potential[perm]).max() <= 1e-12 * scale
    assert mixed.n_pairs[0] == base.n_pairs[0] and mixed.n_reciprocal[0] == base.n_reciprocal[0]


def test_parameter_validation_and_the_string_form():
    p = ewald.EwaldParams(charges="Na=1, Cl=-1,8=-2")
    assert p.charges == ((8, -2.0), (11, 1.0), (17, -1.0)) and p == ewald.EwaldParams(charges={"Na": 1, 17: -1.0, "O": -2})
    assert (p.accuracy, p.alpha, p.max_shells, p.max_index) == (1e-8, None, 8, 64) and abs(p.s - math.sqrt(math.log(1e8))) < 1e-15
    assert ewald.EwaldParams(alpha=0).alpha is None and ewald.EwaldParams(alpha=0.4).alpha == 0.4 and hash(p) == hash(ewald.EwaldParams(charges=p.charges))
    for bad, word in (({"Xx": 1}, "unknown element symbol"), ({"Na": float("nan")}, "finite"), ({"Na": float("inf")}, "finite"), ({"Na": "1"}, "finite"),
                      ("Na=one", "not a number"), ("Na", "ELEMENT=CHARGE"), ("Na=1,11=2", "twice"), ({0: 1}, "atomic number"), ({1.5: 1}, "atomic number")):
        with pytest.raises(ValueError, match=word):
            ewald.EwaldParams(charges=bad)
    for kw, word in ((dict(accuracy=0.0), "accuracy"), (dict(accuracy=1.0), "accuracy"), (dict(accuracy=float("nan")), "accuracy"), (dict(accuracy=-1e-3), "accuracy"),
                     (dict(alpha=-0.1), "alpha"), (dict(alpha=float("inf")), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha="0.3"), "alpha"),
                     (dict(max_shells=0), "max_shells"), (dict(max_shells=9), "max_shells"), (dict(max_index=0), "max_index"), (dict(max_index=128), "max_index"),
                     (dict(max_index=2.5), "max_index")):
        with pytest.raises(ValueError, match=word):
            ewald.EwaldParams(charges={"Na": 1}, **kw)
    assert ewald.resolve(None) is None and ewald.resolve(False) is None and ewald.resolve(p) is p
    for bad, word in ((True, "no default charges"), (ewald.EwaldParams(), "charges is required"), (5, "ewald must be None or an EwaldParams")):
        with pytest.raises(ValueError, match=word):
            ewald.resolve(bad)
    q = ewald.host_charges([11, 17.0, 14, cases.MASK_ATOMIC_NUMBER, 8], p)
    assert q.dtype == np.float32 and q[[0, 1, 4]].tolist() == [1.0, -1.0, -2.0] and np.isnan(q[[2, 3]]).all()
    assert ewald.describe(ewald.CELL | ewald.CHARGED) == "CELL|CHARGED" and ewald.describe(0) == "ok"
    assert abs(ewald.auto_alpha(8, 5.64 ** 3) - math.sqrt(math.pi) * (8 / 5.64 ** 6) ** (1 / 6)) < 1e-15


def test_the_float32_table_is_what_the_restatement_measures():
    """ewald.F32_DEVIATION row by row, as tools/exp/ewald_f32_deviation.py prints it; and n_pairs of the float32 mode against the
    float64 mode.  The float32 d2 of a pair differs from the float64 one by the rounding of the positions, the shift and the
    difference, each within 2^-24 of a coordinate of at most (images + 1) cell lengths, some 30 A here: 6 * 30 * 2^-24 = 1.1e-5 A
    on a distance d, so d2 / r_cut^2 moves by 2 * 1.1e-5 / r_cut < 5e-6 at r_cut > 4.3 A: a crystal whose nearest pair lies
    further than 1e-5 (relative, on d2) from the cut must keep its count."""
    kept = 0
    for name in cases.BATCHES:
        bt, r64 = cases.reference(name)
        r32 = cases.reference32(name)
        assert np.array_equal(r32.flags, r64.flags) and np.array_equal(r32.n_reciprocal, r64.n_reciprocal)
        measured = max(cases.deviation(r64, r32, bt))  # (the table holds three digits; another libm may move the third: 5 %)
        assert measured <= 1.05 * ewald.F32_DEVIATION[name] and ewald.F32_DEVIATION[name] <= 1.05 * measured, (name, measured)
        ok = ((r64.flags & ewald.INVALID_MASK) == 0) & (r64.pair_margin > 1e-5)
        assert np.array_equal(r32.n_pairs[ok], r64.n_pairs[ok]), name
        kept += int(ok.sum())
    assert kept >= 60
    assert ewald.F32_BOUND == 16.0 * 0.000124 and ewald.BOUND_FACTOR == 16.0
    # what the bound cannot see, and what sees it: the smallest kept real-space term of `textbook` against the potential's scale
    bt, r = cases.reference("textbook")
    small = r.smallest_term[:6] / cases.potential_scale(r, bt)[:6]
    assert (small < ewald.F32_BOUND).all() and (small > 1e-12).all()  # a pair lost at the cut hides under it: n_pairs is exact instead


class NoEngine:
    def engine(self):
        raise AssertionError("the engine was touched")


def test_sample_resolves_the_keyword_before_any_engine():
    import inspect

    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    loss = object.__new__(DiffusionLoss)
    loss.T = 100
    state = np.random.get_state()
    kw = dict(model=NoEngine(), z_table=None, num_atoms_per_sample=4, num_samples_in_batch=2)
    for bad, word in ((5, "ewald must be None or an EwaldParams"), (True, "no default charges"), (ewald.EwaldParams(), "charges is required")):
        with pytest.raises(ValueError, match=word):
            DiffusionLoss.sample(loss, ewald=bad, **kw)
    assert np.array_equal(np.random.get_state()[1], state[1])  # nothing drawn
    with pytest.raises(AssertionError, match="the engine was touched"):  # a good value goes on to the sampler
        DiffusionLoss.sample(loss, ewald=ewald.EwaldParams(charges="Na=1,Cl=-1"), **kw)
    assert SampleResult().ewald is None
    for fn in (DiffusionLoss.sample, PONITA_DIFFUSION.sample):
        assert inspect.signature(fn).parameters["ewald"].default is None


def test_parsers_take_the_flags_and_report_bad_values(monkeypatch):
    from arreau_amd import generate, screen
    names = {"--ewald", "--ewald_charges", "--ewald_accuracy", "--ewald_alpha"}
    for parser in (generate.build_parser(), screen.build_parser()):
        assert names <= {s for a in parser._actions for s in a.option_strings}
    args = screen.build_parser().parse_args(["f.npz", "--ewald", "--ewald_charges", "Na=1,Cl=-1", "--ewald_accuracy", "1e-10", "--ewald_alpha", "0.4"])
    assert args.ewald and generate.instrument_params("ewald", args, None) == ewald.EwaldParams(charges={"Na": 1, "Cl": -1}, accuracy=1e-10, alpha=0.4)
    plain = screen.build_parser().parse_args(["f.npz"])
    assert not plain.ewald and plain.ewald_charges is None and generate.instrument_params("ewald", plain, None) == ewald.EwaldParams()
    for field, value, word in (("ewald_accuracy", 2.0, "accuracy"), ("ewald_alpha", -1.0, "alpha"), ("ewald_charges", "Qq=1", "charges: unknown")):
        args = screen.build_parser().parse_args(["f.npz", "--ewald"])
        setattr(args, field, value)
        errors = []
        generate.instrument_params("ewald", args, errors.append)
        assert errors and errors[0].startswith(f"ewald: {word}"), errors
    for main, argv in ((screen.main, ["nowhere.npz", "--ewald"]), (screen.main, ["nowhere.npz", "--ewald", "--ewald_charges", "Na=x"]),
                       (generate.main, ["--model_path", "nowhere.ckpt", "--ewald"]),
                       (generate.main, ["--model_path", "nowhere.ckpt", "--ewald", "--ewald_charges", "Na=1", "--ewald_accuracy", "0"])):
        monkeypatch.setattr("sys.argv", ["prog"] + argv)
        with pytest.raises(SystemExit) as e:
            main()
        assert e.value.code == 2


def test_header_and_binding_agree():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        text = fh.read()
    assert "int arreau_crystal_ewald(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, const float* d_charges" in text
    defs = dict(re.findall(r"#define ARREAU_EWALD_(\w+) ([\w.\-]+)", text))
    assert float(defs.pop("K")) == ewald.K == 14.399645
    assert {k: int(v) for k, v in defs.items()} == {name: bit for bit, name in ewald.FLAG_NAMES}
    fields = re.search(r"typedef struct arreau_ewald_result \{(.*?)\} arreau_ewald_result;", text, re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == ewald.RESULT_KEYS + ("work",) == tuple(n for n, _ in _hip.EwaldResultC._fields_)
    params = re.search(r"typedef struct arreau_ewald_params \{(.*?)\} arreau_ewald_params;", text, re.S).group(1)
    assert tuple(re.findall(r"^\s*(?:double|int32_t) (\w+);", params, re.M)) == tuple(n for n, _ in _hip.EwaldParamsC._fields_) \
        == ("accuracy", "alpha", "max_shells", "max_index")
    assert "arreau_crystal_ewald" in _hip.EXPORTS and set(ewald.STORED_KEYS) - set(ewald.RESULT_KEYS) == {"energy_per_atom", "charge", "species"}
    from arreau_amd import build, engine
    assert "ewald.hip" in build.SOURCES and "ewald.hip" in build.ASM_LINT and callable(engine.ewald) and hasattr(engine.HipEngine, "ewald")
    assert ewald.ROUND == 256 and ewald.cb.STAGED_ATOMS == 256 and ewald.INVALID_MASK == 63


def arrays_of(bt, ref):
    return ewald.sample_arrays({k: np.asarray(getattr(ref, k)) for k in ewald.RESULT_KEYS}, cases.charges(bt), bt.species, bt.counts)


def result_of(bt, ref):
    num = np.array(bt.counts, dtype=np.int64)
    return SampleResult(frac_x=bt.frac.astype(F64), atomic_numbers=bt.species.astype(F64), lattice=bt.lattice.astype(F64),
                        num_atoms=num, idx_start=np.cumsum(num) - num, ewald=arrays_of(bt, ref))


def test_sample_arrays_stats_and_summary_lines():
    bt, r = cases.reference("textbook")
    a = arrays_of(bt, r)
    assert set(a) == set(ewald.STORED_KEYS) and a["potential"].shape == a["charge"].shape == a["species"].shape == (49,)
    assert np.array_equal(a["energy_per_atom"], r.energy / np.array(bt.counts)) and a["charge"].dtype == np.float32 and a["species"].dtype == np.int64
    st = ewald.stats_of(a, 0)
    assert st["crystals"] == 7 and st["energies"] == 7 and st["charged"] == 1 and st["flags"]["CHARGED"] == 1 and st["elements"][11][0] == 4 + 1 + 8
    assert abs(st["energy_min"] - a["energy_per_atom"].min()) == 0 and abs(st["energy_sum"] - a["energy_per_atom"].sum()) < 1e-12
    na = np.abs(r.potential[bt.species == 11]).sum()
    assert abs(st["elements"][11][1] - na) < 1e-12
    line = ewald.format_stats(st)
    assert re.fullmatch(r"ewald rank 0: 7 crystals, 7 energies; eV per atom mean -\d+\.\d{3}, min -\d+\.\d{3}, max -\d+\.\d{3}; charged 14\.3%; "
                        r"mean \|potential\| H: \d+\.\d\d V, F: .* Cs: \d+\.\d\d V; flags CHARGED 1", line), line
    two = ewald.summary_lines([ewald.stats_of(a, 1), st])
    assert len(two) == 3 and two[0].startswith("ewald rank 0") and two[2].startswith("ewald total: 14 crystals, 14 energies;")
    bt, r = cases.reference("flags")
    a = arrays_of(bt, r)
    assert np.isnan(a["energy_per_atom"][:6]).all() and not np.isnan(a["energy_per_atom"][6:8]).any() and np.isnan(a["charge"]).sum() == 2
    st = ewald.stats_of(a)
    assert st["flags"] == {"NONFINITE": 1, "CELL": 1, "EMPTY": 1, "RANGE": 1, "UNASSIGNED": 2, "OVERLAP": 1, "CHARGED": 1} and st["energies"] == 2
    assert ewald.format_stats(st).endswith("flags NONFINITE 1, CELL 1, EMPTY 1, RANGE 1, UNASSIGNED 2, OVERLAP 1, CHARGED 1") and "charged 50.0%" in ewald.format_stats(st)
    assert ewald.format_stats(ewald.total_stats([])) == "ewald total: 0 crystals, 0 energies; eV per atom n/a; mean |potential| n/a; flags none"
    with pytest.raises(ValueError, match="do not match"):
        ewald.sample_arrays({k: np.asarray(getattr(r, k)) for k in ewald.RESULT_KEYS}, cases.charges(bt)[:-1], bt.species, bt.counts)


def test_table_file_round_trip_select_and_concat(tmp_path):
    from arreau_amd.diffusion import instruments
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results, select_crystals
    # the table: every tuple that existed keeps its value, the new one follows
    assert instruments.FULL == instruments.WHOLE + instruments.PATTERNS and "ewald" not in instruments.FULL_KEYWORDS
    assert [e.keyword for e in instruments.FULL] == ["screen", "unique", "find_symmetry", "reduce_cell", "symmetrize", "match_to", "conventional_cell",
                                                     "coordination", "bond_order", "voronoi", "xrd"]
    assert [e.keyword for e in instruments.ENERGIES] == ["ewald"] and instruments.COMPLETE == instruments.FULL + instruments.ENERGIES
    assert list(instruments.COMPLETE_KEYWORDS) == [e.keyword for e in instruments.COMPLETE] and instruments.COMPLETE[-2].keyword == "xrd"
    e = instruments.COMPLETE_KEYWORDS["ewald"]
    assert (e.field, e.prefix, e.stats_key, e.params) == ("ewald", "ewald_", "ewald_stats", "EwaldParams") and e.atom_keys == ("potential", "charge", "species")
    assert dict(e.flags) == {"charges": "ewald_charges", "accuracy": "ewald_accuracy", "alpha": "ewald_alpha"}
    assert e.keys == ewald.STORED_KEYS and e.module is ewald and callable(e.run)
    bt, r = cases.reference("textbook")
    res = result_of(bt, r)
    back = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "c.npz")))
    assert set(back.ewald) == set(ewald.STORED_KEYS)
    for k in ewald.STORED_KEYS:
        assert np.array_equal(back.ewald[k], res.ewald[k], equal_nan=True) and back.ewald[k].dtype == res.ewald[k].dtype, k
    assert np.load(str(tmp_path / "c.npz")).files[5:] == ["ewald_" + k for k in ewald.STORED_KEYS]
    fields = instruments.file_fields(e, res.ewald, len(bt.counts), int(np.sum(bt.counts)))
    assert list(fields) == ["ewald_" + k for k in ewald.STORED_KEYS] and fields["ewald_potential"] is not None
    # a result without the arrays writes the file it always wrote
    res.ewald = None
    plain = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "p.npz")))
    assert plain.ewald is None and list(np.load(str(tmp_path / "p.npz")).files) == ["frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms"]
    res.ewald = arrays_of(bt, r)
    keep = np.zeros(len(bt.counts), dtype=bool)
    keep[[1, 4]] = True
    some = select_crystals(res, keep)
    assert some.ewald["energy"].tolist() == r.energy[[1, 4]].tolist() and some.ewald["potential"].shape == (10,)
    assert np.array_equal(some.ewald["potential"], np.concatenate([r.potential[cases.atoms_of(bt, 1)], r.potential[cases.atoms_of(bt, 4)]]))
    assert some.ewald["species"].tolist() == [11] * 4 + [17] * 4 + [11, 17] and some.ewald["charge"].tolist() == [1.0] * 4 + [-1.0] * 4 + [1.0, -1.0]
    twice = concat_results([some, some])
    assert twice.ewald["energy"].shape == (4,) and twice.ewald["potential"].shape == (20,) and twice.ewald["flags"].tolist() == [0] * 4
    assert concat_results([some, select_crystals(plain, keep)]).ewald is None
    with pytest.raises(ValueError, match="ewald"):
        res.ewald = {k: v for k, v in res.ewald.items() if k != "charge"}
        save_sample_results_to_hdf5(res, str(tmp_path / "bad.npz"))
    with pytest.raises(ValueError, match="per atom"):
        instruments.file_fields(e, dict(arrays_of(bt, r), potential=r.potential[:-1]), len(bt.counts), int(np.sum(bt.counts)))
