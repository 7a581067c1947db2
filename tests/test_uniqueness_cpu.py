"""Duplicate detection, the restatements alone (no GPU): the six invariances of the fingerprint distance in float64, polymorphs
and other formulas, parameter validation, flags, the measured float32-against-float64 deviation behind the GPU tests' bound and
the conditions on the shared inputs under which that bound may be asked for, the file round trip and the statistics lines."""
import numpy as np
import pytest

from arreau_amd.diffusion import screening as sc
from arreau_amd.diffusion import uniqueness as uq
from arreau_amd.diffusion.diffusion_loss import SampleResult
from tests import uniqueness_cases as cases

BATCHES = ("invariance", "ragged", "match_x", "match_y")


def _batch(which):
    return {"invariance": cases.invariance_set, "ragged": cases.ragged_batch, "match_x": lambda: cases.match_sets()[0],
            "match_y": lambda: cases.match_sets()[1]}[which]()


def test_the_six_invariances_hold_in_float64():
    ref = cases.reference_f64("invariance")
    m = uq.match_reference(ref)
    names = cases.INVARIANCE_NAMES
    assert not ref.flags.any()
    for k, name in enumerate(cases.VARIANTS):
        assert ref.species[k].tolist() == [11, 17] + [-1] * 6 and ref.counts[k].tolist() == [1, 1] + [0] * 6, name
        assert abs(m.d[k, 0]) <= 1e-9, (name, m.d[k, 0])
        assert np.abs(ref.fingerprint[k] - ref.fingerprint[0]).max() <= 1e-9, name
        assert m.duplicate_of[k] == (0 if k else -1), name
    assert abs(np.linalg.norm(ref.fingerprint[0]) - 1.0) <= 1e-12
    # the other AB structure: one formula, a different crystal
    cscl = names.index("cscl")
    assert m.candidate[cscl, 0] and m.d[cscl, 0] > 10 * uq.DEFAULT_TOLERANCE, m.d[cscl, 0]
    assert m.duplicate_of[cscl] == -1 and m.nearest[cscl] >= 0
    # other formulas are never comparable -- not AB2 with A2B, not AB with another pair of species
    ab2, a2b, other = names.index("ab2"), names.index("a2b"), names.index("other_pair")
    assert ref.counts[ab2].tolist()[:2] == [1, 2] and ref.counts[a2b].tolist()[:2] == [2, 1]
    for k in (ab2, a2b, other):
        assert not m.candidate[k].any() and not m.candidate[:, k].any(), names[k]
        assert m.duplicate_of[k] == -1 and m.nearest[k] == -1 and np.isinf(m.nearest_distance[k]) and m.unique[k]
    assert abs(m.d[other, 0]) <= 1e-9  # (the same geometry: only the formula keeps them apart)
    assert m.unique.tolist() == [True] + [False] * 6 + [True] * 4


def test_flags_of_the_restatements():
    b, ref = cases.ragged_batch(), cases.reference_f64("ragged")
    r32 = uq.fingerprint_reference_f32(b.frac, b.lattice, b.counts, b.types, cases.params())
    assert ref.flags.tolist() == r32.flags.tolist() == cases.RAGGED_FLAGS
    for k, f in enumerate(cases.RAGGED_FLAGS):
        if f:
            assert not ref.fingerprint[k].any() and not r32.fingerprint[k].any()
            assert (ref.species[k] == -1).all() and (ref.counts[k] == 0).all()
        else:
            assert abs(np.linalg.norm(ref.fingerprint[k]) - 1.0) <= 1e-12
    assert b.counts[:6] == [1, 2, 7, 20, 65, uq.STAGED_ATOMS + 1]
    assert [int((ref.species[k] >= 0).sum()) for k in (0, 2, 4)] == [1, 3, 8]
    m = uq.match_reference(ref)
    assert not m.candidate[np.array(cases.RAGGED_FLAGS) != 0].any() and not m.candidate[:, np.array(cases.RAGGED_FLAGS) != 0].any()
    assert m.duplicate_of[12] == 3 and m.d[12, 3] <= 1e-12  # the same crystal twice
    assert uq.describe(uq.CELL | uq.EMPTY) == "CELL|EMPTY" and uq.describe(0) == "ok"
    # a collapsed cell and more images than max_shells allows are both CELL
    flat = uq.fingerprint_reference_f64([[0.1, 0.2, 0.3]], [np.diag([5.0, 5.0, 0.0])], [1], [0])
    assert flat.flags.tolist() == [uq.CELL]
    few = uq.fingerprint_reference_f64([[0.1, 0.2, 0.3]], [np.eye(3) * 4.0], [1], [0], uq.FingerprintParams(max_shells=1))
    assert few.flags.tolist() == [uq.CELL]


def test_the_contact_counts_straddle_a_wave_and_the_list():
    n = cases.reference_f64("ragged").n_contacts
    ok = np.array(cases.RAGGED_FLAGS) == 0
    assert (n[ok] < 64).any() and ((n[ok] > 64) & (n[ok] <= uq.DRAIN)).any() and ((n[ok] > uq.DRAIN) & (n[ok] <= 2 * uq.LIST)).any()
    assert (n[ok] > 3 * uq.LIST).any()  # several drains in one crystal


def test_the_inputs_allow_the_float32_bound():
    """No contact within screening.distance_bound of r_cut; no candidate distance within 10 D_BOUND of the tolerance; in the
    match sets, whose `nearest` the GPU test compares, the nearest candidate is either exactly tied (copies) or clear by more
    than 2 D_BOUND (the invariance variants tie by construction, to rounding).  Zero cases excluded."""
    for which in BATCHES:
        ref = cases.reference_f64(which)
        assert (ref.near_cut == 0).all(), (which, np.nonzero(ref.near_cut)[0].tolist())
    x, y = cases.reference_f64("match_x"), cases.reference_f64("match_y")
    checked = 0
    for k, m in enumerate((uq.match_reference(x), uq.match_reference(x, y), uq.match_reference(y, x),
                           uq.match_reference(cases.reference_f64("invariance")), uq.match_reference(cases.reference_f64("ragged")))):
        d = m.d[m.candidate]
        assert (np.abs(d - uq.DEFAULT_TOLERANCE) > 10 * uq.D_BOUND).all()
        for r in range(m.d.shape[0] if k < 3 else 0):
            near = np.sort(m.d[r, m.candidate[r]])
            if near.size > 1:
                checked += 1
                assert near[1] == near[0] or near[1] - near[0] > 2 * uq.D_BOUND, (r, near[:3])
    assert checked > 100


def test_float32_deviation_behind_the_gpu_bound():
    """The measured deviation the module states, from which FHAT_BOUND and D_BOUND follow (4 x): the float32 restatement
    against the float64 one over every shared case, in a component of the row and in a distance."""
    worst_f, worst_d, r32 = 0.0, 0.0, {}
    for which in BATCHES:
        b, r64 = _batch(which), cases.reference_f64(which)
        r32[which] = uq.fingerprint_reference_f32(b.frac, b.lattice, b.counts, b.types, cases.params())
        assert r32[which].flags.tolist() == r64.flags.tolist() and (r32[which].species == r64.species).all() and (r32[which].counts == r64.counts).all()
        dev = np.abs(r32[which].fingerprint.astype(np.float64) - r64.fingerprint).max(axis=1)
        print(f"{which}: worst component deviation per crystal {dev.max():.3e} (crystal {int(dev.argmax())})")
        worst_f = max(worst_f, float(dev.max()))
    for a, c in (("invariance", None), ("ragged", None), ("match_x", None), ("match_x", "match_y"), ("match_y", "match_x")):
        m32 = uq.match_reference(r32[a], r32[c] if c else None)
        m64 = uq.match_reference(cases.reference_f64(a), cases.reference_f64(c) if c else None)
        if m64.candidate.any():
            worst_d = max(worst_d, float(np.abs(m32.d - m64.d)[m64.candidate].max()))
    print(f"float32 against float64: component {worst_f:.3e}, distance {worst_d:.3e}")
    assert worst_f <= uq.F32_DEVIATION_FHAT and worst_d <= uq.F32_DEVIATION_D
    assert worst_f >= uq.F32_DEVIATION_FHAT / 2 and worst_d >= uq.F32_DEVIATION_D / 2  # the stated values are the measured ones, rounded up
    assert uq.FHAT_BOUND == 4 * uq.F32_DEVIATION_FHAT and uq.D_BOUND == 4 * uq.F32_DEVIATION_D


def test_match_reference_rules():
    x, y = cases.reference_f64("match_x"), cases.reference_f64("match_y")
    m = uq.match_reference(x)
    assert m.duplicate_of[12] == 3 and m.duplicate_of[20] == 3 and m.nearest[20] == 3  # two equal earlier candidates: the smaller index
    assert m.duplicate_of[50] == 3 and m.duplicate_of[35] == 17 and m.duplicate_of[69] == 0
    assert m.duplicate_of[25] == 5 and 0 < m.distance[25] <= uq.DEFAULT_TOLERANCE  # a near copy
    assert m.duplicate_of[9] == m.duplicate_of[40] == m.duplicate_of[30] == -1 and m.nearest[30] == -1  # flagged, flagged, lone
    assert not m.unique[9] and not m.unique[40] and m.unique[30] and m.unique[0]
    assert (m.duplicate_of < np.arange(70)).all()
    t = uq.match_reference(x, y)
    assert t.duplicate_of[0] == 2 and t.duplicate_of[7] == 16 and t.duplicate_of[31] == 33 and t.duplicate_of[3] == 65
    assert t.duplicate_of[12] == 65 and t.duplicate_of[61] == 48
    assert uq.match_reference(x, tolerance=0.0).duplicate_of[25] == -1
    empty = uq.match_reference(cases.prefix(x, 0))
    assert empty.duplicate_of.shape == (0,)


def test_parameter_validation():
    p = uq.FingerprintParams()
    assert (p.r_max, p.n_bins, p.sigma, p.tolerance, p.max_shells) == (6.0, 64, 0.1, 0.01, 8) and float(p.r_cut) == float(np.float32(6.5))
    for kw in (dict(r_max=0.0), dict(r_max=float("nan")), dict(r_max="6"), dict(sigma=-0.1), dict(sigma=float("inf")), dict(n_bins=0),
               dict(n_bins=65), dict(n_bins=8.0), dict(n_bins=True), dict(tolerance=-0.01), dict(tolerance=1.5), dict(max_shells=9),
               dict(max_shells=0)):
        with pytest.raises(ValueError):
            uq.FingerprintParams(**kw)
    with pytest.raises(Exception):
        p.r_max = 5.0  # frozen
    assert uq.resolve(None) is None and uq.resolve(False) is None and uq.resolve(True) == p and uq.resolve(p) is p
    with pytest.raises(ValueError, match="unique must be"):
        uq.resolve("yes")
    with pytest.raises(ValueError, match="tolerance"):
        uq.match_reference(cases.reference_f64("invariance"), tolerance=2.0)
    # fewer bins: the bins beyond n_bins are zero, the row is still a unit vector
    b = cases.invariance_set()
    r = uq.fingerprint_reference_f64(b.frac[:8], b.lattice[:1], [8], b.types[:8], uq.FingerprintParams(n_bins=10))
    row = r.fingerprint[0].reshape(uq.COMPONENTS, uq.BINS)
    assert not row[:, 10:].any() and row[:3, :10].all() and not row[3:].any() and abs(np.linalg.norm(row) - 1) < 1e-12


def _result(with_uniqueness):
    b = cases.invariance_set()
    n = np.array(b.counts, dtype=np.int64)
    res = SampleResult(num_atoms=n, frac_x=b.frac.astype(np.float64), atomic_numbers=b.types.astype(np.float64),
                       lattice=b.lattice.astype(np.float64), idx_start=np.cumsum(n) - n)
    if with_uniqueness:
        m = uq.match_reference(cases.reference_f64("invariance"))
        res.uniqueness = {"duplicate_of": m.duplicate_of, "distance": m.distance.astype(np.float32), "nearest": m.nearest,
                          "nearest_distance": m.nearest_distance.astype(np.float32), "flags": m.flags, "unique": m.unique}
    return res


def test_file_round_trip(tmp_path):
    from arreau_amd.diffusion.inference import process_generated_crystals as pgc
    plain, full = _result(False), _result(True)
    assert plain.uniqueness is None
    p1 = pgc.save_sample_results_to_hdf5(plain, str(tmp_path / "plain.npz"))
    p2 = pgc.save_sample_results_to_hdf5(full, str(tmp_path / "full.npz"))
    with np.load(p1) as z:
        assert sorted(z.files) == sorted(pgc.KEYS)
    # a file without the arrays is what it was: the bytes np.savez writes for the five keys
    np.savez(str(tmp_path / "five.npz"), **{k: np.asarray(getattr(plain, k), dtype=pgc._DTYPES[k]) for k in pgc.KEYS})
    assert open(p1, "rb").read() == open(str(tmp_path / "five.npz"), "rb").read()
    with np.load(p2) as z:
        assert sorted(z.files) == sorted(list(pgc.KEYS) + ["unique_" + k for k in uq.UNIQUE_KEYS])
    back = pgc.load_sample_results_from_hdf5(p2)
    assert back.metrics is None and set(back.uniqueness) == set(uq.UNIQUE_KEYS)
    for k in uq.UNIQUE_KEYS:
        a, b = np.asarray(full.uniqueness[k]), back.uniqueness[k]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert pgc.load_sample_results_from_hdf5(p1).uniqueness is None
    full.uniqueness.pop("nearest")
    with pytest.raises(ValueError, match="nearest"):
        pgc.save_sample_results_to_hdf5(full, str(tmp_path / "bad.npz"))


def test_statistics_lines():
    m = uq.match_reference(cases.reference_f64("match_x"))
    u = {k: getattr(m, k) for k in uq.UNIQUE_KEYS}
    st = uq.stats_of(u, rank=1)
    assert st["attempted"] == 70 and st["flagged"] == 2 and st["unique"] == int(m.unique.sum()) and st["duplicates"] == int((m.duplicate_of >= 0).sum())
    assert st["unique"] + st["duplicates"] + st["flagged"] == 70
    line = uq.format_stats(st)
    assert line.startswith(f"unique rank 1: unique {st['unique']} / attempted 70; duplicates {st['duplicates']}, flagged 2; nearest_distance min ")
    assert uq.format_stats(uq.stats_of(u, "total"), "novel").startswith(f"novel total: novel {st['unique']} / attempted 70; matched ")
    none = uq.stats_of({k: np.zeros(0) for k in uq.UNIQUE_KEYS})
    assert uq.format_stats(none) == "unique rank 0: unique 0 / attempted 0; duplicates 0, flagged 0"
    assert sc.METRIC_KEYS == ("min_distance", "pair", "n_close", "volume", "number_density", "flags")
