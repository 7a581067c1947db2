"""The powder pattern's float64 restatement (arreau_amd/diffusion/xrd.py: xrd_reference) against the textbook -- which reflections
a lattice has and what they carry --, its invariances (basis, primitive cell, supercell, translation, permutation, rotation),
the closure of the grid integral, `distance`, the parameter validation and the flags, the measured float32 table, and the table
layer: PATTERNS / FULL, the file round trip, select and concat, the parsers, the header and the binding.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from arreau_amd import _hip
from arreau_amd.diffusion import xrd
from arreau_amd.diffusion.diffusion_loss import SampleResult
from tests import xrd_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


def exact(crystal, params=None, weights=None):
    """The float64 restatement of one crystal (frac, cell, atomic numbers) from its float64 numbers: (namespace, pattern)."""
    f, L, z = crystal
    w = np.asarray(z if weights is None else weights, dtype=np.float32)
    r = xrd.xrd_reference(np.asarray(f, dtype=F64).reshape(-1, 3), np.asarray(L, dtype=F64)[None], [len(z)], w, params, exact_inputs=True)
    return r, r.pattern[0]


def angle(a, hkl, wavelength=xrd.XrdParams().wavelength):
    """2 theta in degrees of reflection hkl of a cubic cell of edge a."""
    return 2.0 * math.degrees(math.asin(0.5 * wavelength * math.sqrt(sum(i * i for i in hkl)) / a))


def at(pattern, two_theta, params=None):
    """The pattern's value at the grid point nearest to an angle."""
    return float(pattern[int(np.argmin(np.abs(xrd.grid(params) - two_theta)))])


def lp(two_theta):
    th = np.radians(two_theta) / 2.0
    return (1.0 + np.cos(2.0 * th) ** 2) / (np.sin(th) ** 2 * np.cos(th))


def f2_of(r, volume):
    """|F|^2 of the kept reflections from their intensities: I V^2 / (2 LP)."""
    tt, inten = r.reflections[0]
    return tt, inten * volume ** 2 / (2.0 * lp(tt))


def test_the_case_list_and_no_crystal_sits_on_a_cut():
    assert cases.BATCHES == ("textbook", "cscl unit", "invariance", "ragged", "large", "flags", "points 2", "points 257", "points 4096",
                             "narrow", "wide", "b_iso") and set(xrd.F32_DEVIATION) == set(cases.BATCHES)
    for name in cases.BATCHES:
        bt, r = cases.reference(name)
        ok = r.flags == 0
        assert (r.margin[ok] >= xrd.MARGIN_GUARD).all() and np.isnan(r.margin[~ok]).all(), (name, r.margin)  # no crystal is left out
    bt, r = cases.reference("ragged")
    assert len(bt.counts) == 70 and min(bt.counts) == 1 and max(bt.counts) == 24 and (r.flags == 0).all()
    vol = np.abs(np.linalg.det(bt.lattice.astype(F64)))
    assert np.allclose(vol / np.array(bt.counts), 18.0, rtol=1e-5)
    assert cases.batch("large").counts == [xrd.cb.STAGED_ATOMS + 1]
    inv = cases.reference("invariance")[1]
    assert inv.rounds.min() == 1 and inv.rounds.max() > 1  # a box of one round of 256 entries, and one of several
    assert inv.box.tolist()[:2] == [[3, 3, 3], [2, 2, 2]] and inv.n_reflections[:2].tolist() == [170, 50]
    assert abs(inv.margin[0] - 2.8e-3) < 1e-4 and abs(xrd.grid()[np.argmax(inv.pattern[0])] - 43.4) < 0.026
    d = xrd.derived(cases.NARROW)
    assert 2.0 * d.six_sigma < d.step  # one grid point in a window at most
    assert 9.9 < xrd.derived(cases.WIDE).six_sigma <= xrd.MAX_WINDOW


def test_simple_cubic_has_every_reflection_at_z_squared():
    crystal = cases.textbook_crystals()[0]
    r, P = exact(crystal)
    tt, f2 = f2_of(r, cases.A_PO ** 3)
    assert np.allclose(f2, 84.0 ** 2, rtol=1e-12)
    # every lattice point of the shell, counted in a box twice as large as needed
    d = xrd.derived(xrd.XrdParams())
    h = np.stack(np.meshgrid(*[np.arange(-8, 9)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ds = np.linalg.norm(h, axis=1) / cases.A_PO
    assert r.n_reflections[0] == int(((ds >= d.dlo) & (ds <= d.dhi) & (ds > 0)).sum()) == 2 * tt.size
    for hkl in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 0, 0), (2, 1, 0)):
        assert at(P, angle(cases.A_PO, hkl)) > 1e-3 * P.max(), hkl


def test_centring_shows_as_systematic_absences():
    sc, bcc, fcc, diamond, rock_salt, cscl = cases.textbook_crystals()
    _, P = exact(bcc)
    assert at(P, angle(cases.A_FE, (1, 0, 0))) < 1e-12 * P.max() and at(P, angle(cases.A_FE, (1, 1, 1))) < 1e-12 * P.max()  # h + k + l odd
    assert at(P, angle(cases.A_FE, (1, 1, 0))) > 0.5 * P.max() and at(P, angle(cases.A_FE, (2, 0, 0))) > 0.05 * P.max()
    _, P = exact(fcc)
    for hkl in ((1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 1, 1)):  # mixed parity
        assert at(P, angle(cases.A_CU, hkl)) < 1e-12 * P.max(), hkl
    for hkl in ((1, 1, 1), (2, 0, 0), (2, 2, 0), (3, 1, 1)):
        assert at(P, angle(cases.A_CU, hkl)) > 0.05 * P.max(), hkl
    wide = xrd.XrdParams(two_theta_max=120.0, n_points=2301)
    _, P = exact(diamond, wide)
    for hkl in ((1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 2, 2)):  # fcc's, and h + k + l = 4 n + 2
        assert at(P, angle(cases.A_C, hkl), wide) < 1e-12 * P.max(), hkl
    for hkl in ((1, 1, 1), (2, 2, 0), (3, 1, 1), (4, 0, 0)):
        assert at(P, angle(cases.A_C, hkl), wide) > 0.02 * P.max(), hkl
    # rock salt: the all-odd reflections carry (Z_1 - Z_2)^2, the all-even ones (Z_1 + Z_2)^2, four formula units each
    r, _ = exact(rock_salt)
    tt, f2 = f2_of(r, cases.A_NACL ** 3)
    odd, even = np.abs(tt - angle(cases.A_NACL, (1, 1, 1))) < 1e-6, np.abs(tt - angle(cases.A_NACL, (2, 0, 0))) < 1e-6
    assert odd.sum() == 4 and even.sum() == 3  # the half space's share of 8 and of 6
    assert np.allclose(f2[odd], 16.0 * (11 - 17) ** 2, rtol=1e-10) and np.allclose(f2[even], 16.0 * (11 + 17) ** 2, rtol=1e-10)
    # CsCl with unit amplitudes is bcc
    unit = xrd.XrdParams(scattering="unit")
    _, P = exact(cscl, unit, weights=xrd.host_weights(cscl[2], unit))
    assert at(P, angle(cases.A_CSCL, (1, 0, 0))) < 1e-12 * P.max() and at(P, angle(cases.A_CSCL, (1, 1, 0))) > 0.5 * P.max()
    _, P = exact(cscl)
    assert at(P, angle(cases.A_CSCL, (1, 0, 0))) > 0.05 * P.max()  # with Z it is not


def test_the_pattern_does_not_depend_on_the_description():
    crystals = dict(zip(cases.INVARIANCE_NAMES, cases.invariance_crystals()))
    for a, b in cases.INVARIANCE_PAIRS:
        (ra, Pa), (rb, Pb) = exact(crystals[a]), exact(crystals[b])
        assert np.abs(Pa - Pb).max() <= 1e-13 * Pa.max(), (a, b, np.abs(Pa - Pb).max() / Pa.max())
        assert abs(xrd.distance(Pa, Pb)) < 1e-12 and not np.array_equal(ra.box, rb.box)
    boxes = {n: exact(crystals[n])[0] for n in cases.INVARIANCE_NAMES}
    assert boxes["triclinic"].n_reflections[0] == boxes["triclinic_rebased"].n_reflections[0]  # a basis change keeps the lattice
    assert boxes["triclinic_doubled"].n_reflections[0] > boxes["triclinic"].n_reflections[0]   # a supercell's is denser
    # the box comes from the direct cell: every lattice point of the skewed description's shell, counted in a far larger box
    f, L, z = crystals["triclinic_rebased"]
    d, R = xrd.derived(xrd.XrdParams()), np.linalg.inv(np.asarray(L, dtype=F64)).T
    h = np.stack(np.meshgrid(*[np.arange(-12, 13)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ds = np.linalg.norm(h @ R, axis=1)
    assert boxes["triclinic_rebased"].n_reflections[0] == int(((ds >= d.dlo) & (ds <= d.dhi) & (ds > 0)).sum())
    reach = np.abs(h[ds <= d.dhi]).max(axis=0)
    assert (reach <= np.floor(d.dhi * np.linalg.norm(L, axis=1))).all()  # the rule's bound holds them all ...
    assert (reach > np.floor(d.dhi / np.linalg.norm(R, axis=1))).any()    # ... the reciprocal lengths' would lose some


def test_translation_permutation_and_rotation_leave_the_pattern():
    f, L, z = cases.triclinic_crystal()
    _, P = exact((f, L, z))
    _, moved = exact((f + [0.137, -0.42, 2.3], L, z))
    order = [3, 0, 4, 2, 1]
    _, shuffled = exact((f[order], L, [z[i] for i in order]))
    c, s = math.cos(0.7), math.sin(0.7)
    Q = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, math.cos(1.9), -math.sin(1.9)], [0, math.sin(1.9), math.cos(1.9)]])
    _, turned = exact((f, L @ Q.T, z))
    for name, other in (("translation", moved), ("permutation", shuffled), ("rotation", turned)):
        assert np.abs(P - other).max() <= 1e-12 * P.max(), (name, np.abs(P - other).max() / P.max())


def test_the_grid_integral_is_the_sum_of_the_intensities():
    p = xrd.XrdParams()
    d = xrd.derived(p)
    for crystal in (cases.invariance_crystals()[0], cases.triclinic_crystal()):
        r, P = exact(crystal)
        tt, inten = r.reflections[0]
        inside = (tt - d.six_sigma >= p.two_theta_min) & (tt + d.six_sigma <= p.two_theta_max)
        outside = (tt + d.six_sigma < p.two_theta_min) | (tt - d.six_sigma > p.two_theta_max)
        partly = inten[~inside & ~outside].sum()
        total = P.sum() * d.step
        assert inside.sum() >= 5 and inten[inside].sum() * (1 - 1e-8) <= total <= (inten[inside].sum() + partly) * (1 + 1e-8)
        if partly == 0:
            assert abs(total / inten[inside].sum() - 1.0) < 1e-8  # (the cut at 6 sigma: erfc(6 / sqrt 2) = 2e-9)
    assert exact(cases.invariance_crystals()[0])[0].reflections[0][0].size == 85  # (Cu: half of 170)


def test_distance():
    fcc = cases.invariance_crystals()[0]
    _, P = exact(fcc)
    _, Q = exact(cases.invariance_crystals()[1])
    _, other = exact(([[0, 0, 0], [0.5, 0.5, 0.5]], cases.cube(cases.A_FE), [29, 29]))  # bcc of the same element
    assert abs(xrd.distance(P, Q)) < 1e-12 and xrd.distance(P, 3.0 * P) < 1e-15 and xrd.distance(P, other) > 0.1
    m = xrd.distance_matrix(np.stack([P, Q, other]))
    assert m.shape == (3, 3) and np.allclose(m, m.T) and np.abs(np.diag(m)).max() < 1e-15 and abs(m[0, 2] - xrd.distance(P, other)) < 1e-15
    assert xrd.distance_matrix(np.stack([P, other]), np.stack([Q])).shape == (2, 1)
    assert math.isnan(xrd.distance(P, np.full_like(P, np.nan))) and math.isnan(xrd.distance(P, np.zeros_like(P)))
    with pytest.raises(ValueError, match="different grids"):
        xrd.distance(P, P[:-1])
    lines = xrd.against_lines(np.stack([P, other]), np.stack([Q, other]))
    assert lines == ["xrd against: 2 / 2 pairs; paired distance mean 0.000000, median 0.000000"]
    lines = xrd.against_lines(np.stack([P, other, np.full_like(P, np.nan)]), np.stack([Q]))
    assert lines[0] == "xrd against: crystal 0: smallest distance 0.000000 (target 0)" and lines[2] == "xrd against: crystal 2: no pattern"
    assert len(lines) == 3 and lines[1].startswith("xrd against: crystal 1: smallest distance 0.")


def test_parameter_validation():
    d = xrd.XrdParams()
    assert (d.wavelength, d.two_theta_min, d.two_theta_max, d.n_points, d.fwhm, d.b_iso, d.scattering, d.max_index) == \
        (1.54184, 5.0, 90.0, 1701, 0.2, 0.0, "Z", 64)
    assert xrd.resolve(None) is None and xrd.resolve(False) is None and xrd.resolve(True) == d
    p = xrd.XrdParams(wavelength=0.7093, two_theta_min=0, two_theta_max=160, n_points=2, fwhm=3.9, b_iso=2, scattering="unit", max_index=127)
    assert xrd.resolve(p) is p and p.two_theta_min == 0.0 and p.n_points == 2
    for bad in (0, -1.0, float("nan"), float("inf"), "1.5", True, None):
        with pytest.raises(ValueError, match="wavelength"):
            xrd.XrdParams(wavelength=bad)
    for lo, hi in ((-1, 90), (5, 5), (90, 5), (5, 160.5), (float("nan"), 90), (5, float("inf"))):
        with pytest.raises(ValueError, match="two_theta"):
            xrd.XrdParams(two_theta_min=lo, two_theta_max=hi)
    for name, bads in (("n_points", (1, 4097, 100.0, True)), ("max_index", (0, 128, 2.0, True))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                xrd.XrdParams(**{name: bad})
    for bad in (0, -0.2, float("nan"), 3.93, 50.0):  # 6 sigma of 3.93 is 10.01 degrees: past the window's cap
        with pytest.raises(ValueError, match="fwhm"):
            xrd.XrdParams(fwhm=bad)
    assert xrd.XrdParams(fwhm=3.92).fwhm == 3.92
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="b_iso"):
            xrd.XrdParams(b_iso=bad)
    with pytest.raises(ValueError, match="scattering"):
        xrd.XrdParams(scattering="cromer-mann")
    with pytest.raises(ValueError, match="xrd must be None, True or a XrdParams"):
        xrd.resolve(5)
    with pytest.raises(ValueError, match="weights"):
        xrd.resolve(xrd.XrdParams(scattering="weights"))  # (the sampler has no array to give)
    g = xrd.grid()
    assert g.shape == (1701,) and g[0] == 5.0 and g[-1] == 90.0 and abs(g[1] - g[0] - 0.05) < 1e-12
    assert np.array_equal(xrd.grid(xrd.grid_row(p)), xrd.grid(p)) and xrd.grid(p).tolist() == [0.0, 160.0]


def test_every_flag_blanks_the_crystal():
    bt, r = cases.reference("flags")
    assert r.flags.tolist() == cases.FLAGS_EXPECTED and [xrd.describe(f) for f in r.flags] == ["NONFINITE", "CELL", "EMPTY", "RANGE", "ok"]
    assert np.isnan(r.pattern[:4]).all() and (r.n_reflections[:4] == 0).all() and np.isnan(r.volume[:4]).all() and np.isnan(r.weight_sum[:4]).all()
    assert not np.isnan(r.pattern[4]).any() and r.n_reflections[4] > 0 and r.volume[4] == 27.0 and r.weight_sum[4] == 13.0
    assert xrd.box_of(bt.lattice[3], bt.params)[0] > bt.params.max_index >= xrd.box_of(bt.lattice[3], bt.params)[1]  # the 200 A axis alone
    # an amplitude that is not finite is NONFINITE too
    one = cases.single(bt, 4)
    assert xrd.xrd_reference(one.frac, one.lattice, one.counts, [np.inf], one.params).flags.tolist() == [xrd.NONFINITE]
    assert xrd.xrd_reference(one.frac, one.lattice, one.counts, [13.0], xrd.XrdParams(max_index=1)).flags.tolist() == [xrd.RANGE]


def test_the_float32_table_is_what_the_restatement_measures():
    """xrd.F32_DEVIATION row by row: the float32 mode against float64 on the CPU, as tools/exp/xrd_f32_deviation.py prints it."""
    for name in cases.BATCHES:
        bt, r64 = cases.reference(name)
        r32 = xrd.xrd_reference(bt.frac, bt.lattice, bt.counts, cases.weights(bt), bt.params, dtype=np.float32)
        assert np.array_equal(r32.n_reflections, r64.n_reflections) and np.array_equal(r32.flags, r64.flags) and r32.pattern.dtype == np.float32
        ok = r64.flags == 0
        err = np.abs(r32.pattern[ok].astype(F64) - r64.pattern[ok]).max(axis=1) / cases.scale(r64)[ok]
        assert float(f"{err.max():.3g}") == xrd.F32_DEVIATION[name], (name, err.max())
        assert np.array_equal(r32.weight_sum[ok], r64.weight_sum[ok]) and np.array_equal(r32.volume[ok], r64.volume[ok])
    assert xrd.F32_BOUND == 16.0 * 5.93e-07 and xrd.BOUND_FACTOR == 16.0
    # the derived part: the reduced phase's error bound at the largest indices the batches reach
    assert 2 * math.pi * (3 * 21 + 2) * 2.0 ** -24 < 2.5e-5


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
    with pytest.raises(ValueError, match="xrd must be None, True or a XrdParams"):
        DiffusionLoss.sample(loss, xrd=5, **kw)
    assert np.array_equal(np.random.get_state()[1], state[1])  # nothing drawn
    with pytest.raises(AssertionError, match="the engine was touched"):  # a good value goes on to the sampler
        DiffusionLoss.sample(loss, xrd=xrd.XrdParams(fwhm=0.3), **kw)
    assert SampleResult().xrd is None
    for fn in (DiffusionLoss.sample, PONITA_DIFFUSION.sample):
        assert inspect.signature(fn).parameters["xrd"].default is None


def test_parsers_take_the_flags_and_report_bad_values(monkeypatch):
    from arreau_amd import generate, screen
    names = {"--xrd", "--xrd_wavelength", "--xrd_fwhm", "--xrd_two_theta_min", "--xrd_two_theta_max", "--xrd_points", "--xrd_b_iso", "--xrd_scattering"}
    for parser in (generate.build_parser(), screen.build_parser()):
        assert names <= {s for a in parser._actions for s in a.option_strings}
    assert "--xrd_against" in {s for a in screen.build_parser()._actions for s in a.option_strings}
    args = screen.build_parser().parse_args(["f.npz", "--xrd", "--xrd_wavelength", "0.7093", "--xrd_fwhm", "0.1", "--xrd_two_theta_min", "3",
                                             "--xrd_two_theta_max", "60", "--xrd_points", "571", "--xrd_b_iso", "0.5", "--xrd_scattering", "unit"])
    assert args.xrd and generate.instrument_params("xrd", args, None) == \
        xrd.XrdParams(wavelength=0.7093, fwhm=0.1, two_theta_min=3, two_theta_max=60, n_points=571, b_iso=0.5, scattering="unit")
    plain = screen.build_parser().parse_args(["f.npz"])
    assert not plain.xrd and plain.xrd_against is None and generate.instrument_params("xrd", plain, None) == xrd.XrdParams()
    for field, value, word in (("xrd_fwhm", 0.0, "fwhm"), ("xrd_points", 1, "n_points"), ("xrd_two_theta_max", 170.0, "0 <= two_theta_min")):
        args = screen.build_parser().parse_args(["f.npz", "--xrd"])
        setattr(args, field, value)
        errors = []
        generate.instrument_params("xrd", args, errors.append)
        assert errors and errors[0].startswith(f"xrd: {word}"), errors
    for main, argv in ((screen.main, ["nowhere.npz", "--xrd", "--xrd_fwhm", "-1"]), (screen.main, ["nowhere.npz", "--xrd_against", "t.npz"]),
                       (generate.main, ["--model_path", "nowhere.ckpt", "--xrd", "--xrd_points", "5000"]),
                       (generate.main, ["--model_path", "nowhere.ckpt", "--xrd", "--xrd_scattering", "weights"])):
        monkeypatch.setattr("sys.argv", ["prog"] + argv)
        with pytest.raises(SystemExit) as e:
            main()
        assert e.value.code == 2


def test_header_and_binding_agree():
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        text = fh.read()
    assert "int arreau_crystal_xrd(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, const float* d_weights" in text
    defs = dict(re.findall(r"#define ARREAU_XRD_(\w+) ([\w.\-]+)", text))
    assert (int(defs.pop("MAX_POINTS")), int(defs.pop("MAX_INDEX")), float(defs.pop("MAX_TWO_THETA")), float(defs.pop("MAX_WINDOW"))) == \
        (xrd.MAX_POINTS, xrd.MAX_INDEX, xrd.MAX_TWO_THETA, xrd.MAX_WINDOW)
    assert {k: int(v) for k, v in defs.items()} == {name: bit for bit, name in xrd.FLAG_NAMES}
    fields = re.search(r"typedef struct arreau_xrd_result \{(.*?)\} arreau_xrd_result;", text, re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", fields)) == xrd.RESULT_KEYS == tuple(n for n, _ in _hip.XrdResultC._fields_)
    params = re.search(r"typedef struct arreau_xrd_params \{(.*?)\} arreau_xrd_params;", text, re.S).group(1)
    assert tuple(re.findall(r"^\s*(?:double|int32_t) (\w+);", params, re.M)) == tuple(n for n, _ in _hip.XrdParamsC._fields_) \
        == ("wavelength", "two_theta_min", "two_theta_max", "fwhm", "b_iso", "n_points", "max_index")
    assert "arreau_crystal_xrd" in _hip.EXPORTS and set(xrd.STORED_KEYS) - set(xrd.RESULT_KEYS) == {"max_intensity", "two_theta_peak", "grid"}
    from arreau_amd import build, engine
    assert "xrd.hip" in build.SOURCES and "xrd.hip" in build.ASM_LINT and callable(engine.xrd) and hasattr(engine.HipEngine, "xrd")
    assert xrd.ROUND == 256 and xrd.cb.STAGED_ATOMS == 256


def arrays_of(bt, ref):
    return xrd.sample_arrays({k: np.asarray(getattr(ref, k)) for k in xrd.RESULT_KEYS}, bt.params)


def result_of(bt, ref):
    num = np.array(bt.counts, dtype=np.int64)
    return SampleResult(frac_x=bt.frac.astype(F64), atomic_numbers=bt.species.astype(F64), lattice=bt.lattice.astype(F64),
                        num_atoms=num, idx_start=np.cumsum(num) - num, xrd=arrays_of(bt, ref))


def test_sample_arrays_stats_and_summary_lines():
    bt, r = cases.reference("textbook")
    a = arrays_of(bt, r)
    assert set(a) == set(xrd.STORED_KEYS) and a["pattern"].shape == (6, 1701) and a["grid"].shape == (6, 5)
    assert a["grid"][0].tolist() == [1.54184, 5.0, 90.0, 1701.0, 0.2] and np.array_equal(xrd.grid(a["grid"][3]), xrd.grid())
    assert np.array_equal(a["max_intensity"], r.pattern.max(axis=1).astype(np.float32))
    fcc = cases.TEXTBOOK_NAMES.index("fcc")
    assert abs(a["two_theta_peak"][fcc] - angle(cases.A_CU, (1, 1, 1))) < 0.026 and a["two_theta_peak"][fcc] in xrd.grid()
    st = xrd.stats_of(a, 0)
    assert st["crystals"] == 6 and st["patterns"] == 6 and st["n_reflections"] == int(r.n_reflections.sum()) and not any(st["flags"].values())
    line = xrd.format_stats(st)
    assert re.fullmatch(r"xrd rank 0: 6 crystals, 6 patterns; mean n_reflections \d+\.\d; two_theta_peak mean \d+\.\d\d, min \d+\.\d\d, max \d+\.\d\d; flags none", line), line
    two = xrd.summary_lines([xrd.stats_of(a, 1), st])
    assert len(two) == 3 and two[0].startswith("xrd rank 0") and two[2].startswith("xrd total: 12 crystals, 12 patterns;")
    bt, r = cases.reference("flags")
    a = arrays_of(bt, r)
    assert np.isnan(a["max_intensity"][:4]).all() and np.isnan(a["two_theta_peak"][:4]).all() and not np.isnan(a["two_theta_peak"][4])
    st = xrd.stats_of(a)
    assert st["flags"] == {"NONFINITE": 1, "CELL": 1, "EMPTY": 1, "RANGE": 1} and st["patterns"] == 1
    assert xrd.format_stats(st).endswith("flags NONFINITE 1, CELL 1, EMPTY 1, RANGE 1")
    assert xrd.format_stats(xrd.total_stats([])) == "xrd total: 0 crystals, 0 patterns; mean n_reflections n/a; two_theta_peak n/a; flags none"


def test_table_file_round_trip_select_and_concat(tmp_path):
    from arreau_amd.diffusion import instruments
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results, select_crystals
    # the table: every tuple that existed keeps its value, the new one follows
    assert instruments.WHOLE == instruments.TABLE + instruments.CELLS and "xrd" not in instruments.WHOLE_KEYWORDS
    assert [e.keyword for e in instruments.PATTERNS] == ["xrd"] and instruments.FULL == instruments.WHOLE + instruments.PATTERNS
    assert list(instruments.FULL_KEYWORDS) == [e.keyword for e in instruments.FULL] and instruments.FULL[-2].keyword == "voronoi"
    e = instruments.FULL_KEYWORDS["xrd"]
    assert (e.field, e.prefix, e.stats_key, e.params) == ("xrd", "xrd_", "xrd_stats", "XrdParams") and e.atom_keys == ()
    assert dict(e.flags) == {"wavelength": "xrd_wavelength", "fwhm": "xrd_fwhm", "two_theta_min": "xrd_two_theta_min", "two_theta_max": "xrd_two_theta_max",
                             "n_points": "xrd_points", "b_iso": "xrd_b_iso", "scattering": "xrd_scattering"}
    assert e.keys == xrd.STORED_KEYS and e.module is xrd and callable(e.run)
    bt, r = cases.reference("textbook")
    res = result_of(bt, r)
    back = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "c.npz")))
    assert set(back.xrd) == set(xrd.STORED_KEYS)
    for k in xrd.STORED_KEYS:
        assert np.array_equal(back.xrd[k], res.xrd[k], equal_nan=True) and back.xrd[k].dtype == res.xrd[k].dtype, k
    assert np.load(str(tmp_path / "c.npz")).files[5:] == ["xrd_" + k for k in xrd.STORED_KEYS]
    # after voronoi_* when both are there
    from arreau_amd.diffusion import voronoi as vo
    from tests import voronoi_cases
    vb, vr = voronoi_cases.reference("one atom")
    num = np.array(vb.counts, dtype=np.int64)
    ref = xrd.xrd_reference(vb.frac, vb.lattice, vb.counts, vb.species.astype(np.float32))
    both = SampleResult(frac_x=vb.frac.astype(F64), atomic_numbers=vb.species.astype(F64), lattice=vb.lattice.astype(F64), num_atoms=num,
                        idx_start=np.cumsum(num) - num, voronoi=vo.sample_arrays({k: np.asarray(getattr(vr, k)) for k in vo.RESULT_KEYS}, vb.species),
                        xrd=xrd.sample_arrays({k: np.asarray(getattr(ref, k)) for k in xrd.RESULT_KEYS}))
    files = np.load(save_sample_results_to_hdf5(both, str(tmp_path / "b.npz"))).files
    assert files[5:] == ["voronoi_" + k for k in vo.STORED_KEYS] + ["xrd_" + k for k in xrd.STORED_KEYS]
    # a result without the arrays writes the file it always wrote
    res.xrd = None
    plain = load_sample_results_from_hdf5(save_sample_results_to_hdf5(res, str(tmp_path / "p.npz")))
    assert plain.xrd is None and list(np.load(str(tmp_path / "p.npz")).files) == ["frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms"]
    res.xrd = arrays_of(bt, r)
    keep = np.zeros(len(bt.counts), dtype=bool)
    keep[[1, 4]] = True
    some = select_crystals(res, keep)
    assert some.xrd["pattern"].shape == (2, 1701) and np.array_equal(some.xrd["pattern"], res.xrd["pattern"][[1, 4]])
    assert some.xrd["n_reflections"].tolist() == r.n_reflections[[1, 4]].tolist() and some.xrd["grid"].shape == (2, 5)
    twice = concat_results([some, some])
    assert twice.xrd["pattern"].shape == (4, 1701) and twice.xrd["flags"].tolist() == [0] * 4
    assert concat_results([some, select_crystals(plain, keep)]).xrd is None
    with pytest.raises(ValueError, match="xrd"):
        res.xrd = {k: v for k, v in res.xrd.items() if k != "grid"}
        save_sample_results_to_hdf5(res, str(tmp_path / "bad.npz"))
