"""The table of per-crystal instruments (arreau_amd/diffusion/instruments.py) and the consumers that loop over it: the crystals file's
layout, concat_results / select_crystals, the file layer's rejections and the driver's per-rank statistics.  Synthetic numpy
dicts; no GPU."""
import sys

import numpy as np
import pytest

from arreau_amd.diffusion import instruments
from arreau_amd.diffusion.diffusion_loss import SampleResult
from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
from arreau_amd.generate import _gather_results, concat_results, instrument_lines, select_crystals

BASE = ["frac_x", "atomic_numbers", "lattice", "idx_start", "num_atoms"]
# the file contract, written out: the keys of a crystals file that carries every instrument's arrays, in the file's order
FILE_KEYS = BASE + [
    "screen_min_distance", "screen_pair", "screen_n_close", "screen_volume", "screen_number_density", "screen_flags", "screen_valid",
    "unique_duplicate_of", "unique_distance", "unique_nearest", "unique_nearest_distance", "unique_flags", "unique_unique",
    "sym_n_lattice", "sym_n_ops", "sym_n_translations", "sym_ops_rotation", "sym_ops_translation", "sym_ops_residual", "sym_residual",
    "sym_point_group", "sym_flags", "sym_symprec",
    "reduced_multiplicity", "reduced_n_translations", "reduced_lattice", "reduced_transform", "reduced_num_atoms", "reduced_flags",
    "reduced_selling_steps", "reduced_symprec", "reduced_frac_x", "reduced_atomic_numbers", "reduced_keep",
    "symmetrized_frac_x", "symmetrized_lattice", "symmetrized_lengths", "symmetrized_angles", "symmetrized_orbit",
    "symmetrized_orbit_size", "symmetrized_site_order", "symmetrized_n_orbits", "symmetrized_max_displacement",
    "symmetrized_rms_displacement", "symmetrized_ops_translation", "symmetrized_flags",
    "match_target", "match_n_comparable", "match_rms", "match_rms_norm", "match_max_dist", "match_mapping", "match_translation",
    "match_partner", "match_n_mappings", "match_n_candidates", "match_n_permutations", "match_matched", "match_flags"]
COUNTS, REDUCED_COUNTS, MAX_OPS = [2, 3, 1], [1, 3, 1], 4
B, N, NR = len(COUNTS), sum(COUNTS), sum(REDUCED_COUNTS)
FIELDS = ("metrics", "uniqueness", "symmetry", "reduced", "symmetrized", "match")
CARRIED = tuple(f for f in FIELDS if f != "uniqueness")


def _rows(n, *tail, dtype=np.float32, start=0):
    """[n, *tail] with row r filled with start + r: a row's value says which crystal (or atom) it belongs to."""
    return (np.arange(start, start + n).reshape((n,) + (1,) * len(tail)) * np.ones((n,) + tail)).astype(dtype)


def _result(start=0):
    """A result of three crystals that carries all six fields; per-crystal rows hold the crystal's index (+ start), per-atom rows
    the atom's."""
    c = lambda *tail, **kw: _rows(B, *tail, start=start, **kw)   # one row per crystal
    a = lambda *tail, **kw: _rows(N, *tail, start=start, **kw)   # per atom
    r = lambda *tail, **kw: _rows(NR, *tail, start=start, **kw)  # per reduced atom
    i32 = dict(dtype=np.int32)
    fields = {
        "metrics": {"min_distance": c(), "pair": c(5, **i32), "n_close": c(**i32), "volume": c(), "number_density": c(), "flags": np.array([0, 4, 0], np.int32),
                    "valid": np.array([True, False, True])},
        "uniqueness": {"duplicate_of": np.array([-1, 0, -1], np.int32), "distance": c(), "nearest": c(**i32), "nearest_distance": c(),
                       "flags": np.zeros(B, np.int32), "unique": np.array([True, False, True])},
        "symmetry": {"n_lattice": c(**i32), "n_ops": c(**i32), "n_translations": c(**i32), "ops_rotation": c(MAX_OPS, **i32),
                     "ops_translation": c(MAX_OPS, 3), "ops_residual": c(MAX_OPS), "residual": c(), "point_group": np.array([0, 31, -1], np.int32),
                     "flags": np.array([0, 0, 8], np.int32), "symprec": c()},
        "reduced": {"multiplicity": np.array([2, 1, 1], np.int32), "n_translations": c(**i32), "lattice": c(3, 3), "transform": c(3, 3),
                    "num_atoms": np.array(REDUCED_COUNTS, np.int64), "flags": np.zeros(B, np.int32), "selling_steps": c(**i32), "symprec": c(),
                    "frac_x": r(3), "atomic_numbers": r(dtype=np.int64), "keep": r(**i32)},
        "symmetrized": {"frac_x": a(3), "lattice": c(3, 3), "lengths": c(3), "angles": c(3), "orbit": a(**i32), "orbit_size": a(**i32),
                        "site_order": a(**i32), "n_orbits": np.array([1, 2, 1], np.int32), "max_displacement": c(), "rms_displacement": c(),
                        "ops_translation": c(MAX_OPS, 3), "flags": np.zeros(B, np.int32)},
        "match": {"target": c(**i32), "n_comparable": c(**i32), "rms": c(), "rms_norm": c(), "max_dist": c(), "mapping": c(**i32),
                  "translation": c(3), "partner": a(**i32), "n_mappings": c(**i32), "n_candidates": c(**i32), "n_permutations": c(**i32),
                  "matched": np.array([1, 0, 1], np.int32), "flags": np.array([0, 8, 0], np.int32)},
    }
    return SampleResult(**_plain_arrays(), **fields)


def _plain_arrays():
    num = np.array(COUNTS, np.int64)
    return dict(frac_x=_rows(N, 3, dtype=np.float64), atomic_numbers=_rows(N, dtype=np.float64), lattice=_rows(B, 3, 3, dtype=np.float64),
                num_atoms=num, idx_start=np.cumsum(num) - num)


def test_the_table_imports_without_torch_and_names_the_modules_own_keys():
    import subprocess
    code = "import sys, arreau_amd.diffusion.instruments; assert 'torch' not in sys.modules and 'arreau_amd._hip' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
    assert [e.field for e in instruments.INSTRUMENTS] == list(FIELDS)
    assert [e.prefix + k for e in instruments.INSTRUMENTS for k in e.keys] == FILE_KEYS[len(BASE):]
    assert [e.field for e in instruments.INSTRUMENTS if e.carried] == list(CARRIED)
    assert all(set(e.atom_keys) <= set(e.keys) and getattr(e.module, e.params) for e in instruments.INSTRUMENTS)


def test_file_layout(tmp_path):
    res = _result()
    name = save_sample_results_to_hdf5(res, str(tmp_path / "all.npz"))
    with np.load(name) as z:
        assert z.files == FILE_KEYS
    back = load_sample_results_from_hdf5(name)
    for k in BASE:
        assert np.array_equal(getattr(back, k), getattr(res, k)), k
    for f in FIELDS:
        want, got = getattr(res, f), getattr(back, f)
        assert set(got) == set(want) | ({"lattice"} if f == "symmetry" else set()), f
        for k, v in want.items():
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), (f, k)
    assert back.symmetry["lattice"].dtype == np.float32 and np.array_equal(back.symmetry["lattice"], res.lattice.astype(np.float32))
    plain = SampleResult(**_plain_arrays())
    with np.load(save_sample_results_to_hdf5(plain, str(tmp_path / "plain.npz"))) as z:
        assert z.files == BASE
    back = load_sample_results_from_hdf5(str(tmp_path / "plain.npz"))
    assert all(getattr(back, f) is None for f in FIELDS)


def test_concat_and_select():
    r, plain = _result(), SampleResult(**_plain_arrays())
    both = concat_results([r, r])
    assert both.num_atoms.tolist() == COUNTS * 2 and both.idx_start.tolist() == [0, 2, 5, 6, 8, 11] and both.uniqueness is None
    for f in CARRIED:
        for k, v in getattr(r, f).items():
            assert np.array_equal(getattr(both, f)[k], np.concatenate([v, v])), (f, k)
    mixed = concat_results([r, plain])
    assert len(mixed.num_atoms) == 2 * B and all(getattr(mixed, f) is None for f in FIELDS)
    kept = select_crystals(r, [True, False, True])
    assert kept.num_atoms.tolist() == [2, 1] and kept.idx_start.tolist() == [0, 2] and kept.frac_x[:, 0].tolist() == [0, 1, 5]
    assert kept.uniqueness is None
    crystals, atoms, reduced_atoms = [0, 2], [0, 1, 5], [0, 4]  # (reduced counts 1, 3, 1: crystal 2's reduced atom is row 4)
    for f, entry in zip(FIELDS, instruments.INSTRUMENTS):
        if f == "uniqueness":
            continue
        rows_of = lambda k: (reduced_atoms if f == "reduced" else atoms) if k in entry.atom_keys else crystals
        for k, v in getattr(r, f).items():
            assert np.array_equal(getattr(kept, f)[k], v[rows_of(k)]), (f, k)
    assert kept.symmetrized["orbit"].tolist() == atoms and kept.match["partner"].tolist() == atoms
    assert kept.reduced["keep"].tolist() == reduced_atoms and kept.reduced["num_atoms"].tolist() == [1, 1] and kept.reduced["frac_x"].shape == (2, 3)
    none = select_crystals(r, [False, False, False])
    assert none.reduced["frac_x"].shape == (0, 3) and none.match["partner"].shape == (0,) and none.metrics["pair"].shape == (0, 5)


def _save_with(tmp_path, field, arrays):
    res = _result()
    setattr(res, field, arrays)
    return save_sample_results_to_hdf5(res, str(tmp_path / "bad.npz"))


@pytest.mark.parametrize("entry", instruments.INSTRUMENTS, ids=lambda e: e.field)
def test_rejections_of_every_key(tmp_path, entry):
    good = getattr(_result(), entry.field)
    assert tuple(good) == entry.keys
    for k in entry.keys:
        with pytest.raises(ValueError, match=rf"SampleResult\.{entry.field}\['{k}'\] is missing"):
            _save_with(tmp_path, entry.field, {j: v for j, v in good.items() if j != k})
        longer = np.concatenate([good[k], good[k][:1]])  # one row more than the crystals (or the atoms) it belongs to
        with pytest.raises(ValueError, match=rf"SampleResult\.{entry.field}\['{k}'\]"):
            _save_with(tmp_path, entry.field, {**good, k: longer})
        with pytest.raises(ValueError, match=rf"SampleResult\.{entry.field}\['{k}'\]"):
            _save_with(tmp_path, entry.field, {**good, k: good[k][:-1]})


def test_rejections_of_a_wrong_shape(tmp_path):
    r = _result()
    with pytest.raises(ValueError, match=r"SampleResult\.metrics\['pair'\]"):
        _save_with(tmp_path, "metrics", {**r.metrics, "pair": r.metrics["pair"][:, :4]})
    for k in r.uniqueness:
        with pytest.raises(ValueError, match=rf"SampleResult\.uniqueness\['{k}'\]"):
            _save_with(tmp_path, "uniqueness", {**r.uniqueness, k: r.uniqueness[k].reshape(B, 1)})
    for k in r.metrics:
        if k != "pair":
            with pytest.raises(ValueError, match=rf"SampleResult\.metrics\['{k}'\]"):
                _save_with(tmp_path, "metrics", {**r.metrics, k: r.metrics[k].reshape(B, 1)})
    with pytest.raises(ValueError, match=r"SampleResult\.symmetry\['ops_rotation'\]"):
        _save_with(tmp_path, "symmetry", {**r.symmetry, "ops_rotation": r.symmetry["ops_rotation"][:, 0]})
    with pytest.raises(ValueError, match=r"SampleResult\.symmetry\['ops_translation'\]"):
        _save_with(tmp_path, "symmetry", {**r.symmetry, "ops_translation": r.symmetry["ops_translation"][:, :, 0]})
    with pytest.raises(ValueError, match=r"SampleResult\.symmetry\['n_ops'\]"):
        _save_with(tmp_path, "symmetry", {**r.symmetry, "n_ops": r.symmetry["n_ops"].reshape(B, 1)})
    assert _save_with(tmp_path, "symmetrized", {**r.symmetrized, "ops_translation": r.symmetrized["ops_translation"][:, :2]})  # leading only


def test_per_rank_statistics_and_their_lines():
    ranks = [_result(), _result(start=3)]
    sent = []
    assert _gather_results(ranks[1], 1, 2, gather=sent.append) is None  # rank 1 sends its result, its statistics in it
    whole = _gather_results(ranks[0], 0, 2, gather=lambda local: [local] + sent)
    assert len(whole.num_atoms) == 2 * B and whole.uniqueness is None
    host = [e for e in instruments.INSTRUMENTS if e.carried]
    assert [e.stats_key for e in host] == ["screen_stats", "symmetry_stats", "reduce_stats", "symmetrize_stats", "match_stats"]
    assert set(whole.info) == {e.stats_key for e in host}
    for e in host:
        stats = whole.info[e.stats_key]
        assert [st["rank"] for st in stats] == [0, 1] and all(st["attempted"] == B for st in stats), e.stats_key
        assert stats == [e.stats_of(getattr(ranks[rank], e.field), rank) for rank in (0, 1)]
        lines = instrument_lines(e.keyword, whole, stats)
        assert lines == e.module.summary_lines(stats) and len(lines) == 3
        assert lines[0].split(":")[0].endswith("rank 0") and lines[1].split(":")[0].endswith("rank 1") and lines[2].split(":")[0].endswith("total")
        assert instrument_lines(e.keyword, whole) == e.module.summary_lines([e.stats_of(getattr(whole, e.field))])  # (no parts: one set)
    assert whole.info["screen_stats"][0]["accepted"] == 2 and whole.info["match_stats"][1]["matched"] == 2
