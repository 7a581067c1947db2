"""Bond angles and Steinhardt order parameters without a GPU: the float64 restatement against the textbook shells, the identity
with the spherical harmonics, the invariances; the float32 restatement (the kernel's bit-for-bit yardstick) against the float64 one
within the derived bounds; header, binding and build list; the instrument table, the file layer and the command lines."""
import inspect
import os
import re

import numpy as np
import pytest

from arreau_amd.diffusion import bond_order as bo
from arreau_amd.diffusion import coordination as co
from arreau_amd.diffusion import instruments
from tests import bond_order_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hist(row):
    return {int(5 * k): int(v) for k, v in enumerate(row) if v}


# --------------------------------------------------------------------------------------------------------- analytic shells
@pytest.mark.parametrize("shell,case,atom", cases.analytic_shells())
def test_analytic_shell(shell, case, atom):
    _, _, r64 = cases.references()[case]
    m, q, hist = cases.ANALYTIC[shell]
    print(shell, case, atom, r64.n_used[atom], r64.q[atom], _hist(r64.angles[atom]))
    assert r64.n_used[atom] == m
    assert np.abs(r64.q[atom] - np.array(q)).max() <= 1e-6
    assert _hist(r64.angles[atom]) == hist
    assert r64.angles[atom].sum() == m * (m - 1) // 2


def test_analytic_values_agree_with_numpys_legendre():
    """The table's q values from numpy's own Legendre evaluation on ideal shells (no cell, no list)."""
    from numpy.polynomial import legendre
    g = (1 + np.sqrt(5)) / 2
    perms = lambda v: [np.roll(v, k) for k in range(3)]
    signs = lambda v: {tuple(np.array(v) * s) for s in np.ndindex(2, 2, 2) for s in [1 - 2 * np.array(s)]}
    shells = {"fcc": {t for p in perms([0, 1, 1]) for t in signs(p)}, "bcc": signs([1, 1, 1]), "simple_cubic": {t for p in perms([0, 0, 1]) for t in signs(p)},
              "diamond": {(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)}, "icosahedron": {t for p in perms([0, 1, g]) for t in signs(p)}}
    for name, vecs in shells.items():
        u = np.array(sorted(vecs), dtype=np.float64)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        m, q, _ = cases.ANALYTIC[name]
        assert len(u) == m
        c = np.clip(u @ u.T, -1, 1)
        got = [np.sqrt(max(legendre.legval(c, [0] * l + [1]).sum(), 0.0)) / m for l in bo.L_VALUES]
        assert np.abs(np.array(got) - np.array(q)).max() <= 1e-6, name


def _sph_harm(l, mm, theta, phi):
    """Y_l^mm (Condon-Shortley), mm >= 0, float64: the associated Legendre function as the mm-th derivative of numpy's Legendre
    series, P_l^mm(x) = (-1)^mm (1 - x^2)^(mm/2) d^mm P_l / dx^mm."""
    from math import factorial

    from numpy.polynomial.legendre import Legendre
    x = np.cos(theta)
    series = Legendre.basis(l)
    p = (-1) ** mm * (1 - x * x) ** (mm / 2.0) * (series.deriv(mm)(x) if mm else series(x))
    return np.sqrt((2 * l + 1) / (4 * np.pi) * factorial(l - mm) / factorial(l + mm)) * p * np.exp(1j * mm * phi)


def test_q_equals_the_spherical_harmonic_form():
    """q_l^2 = (4 pi / (2l+1)) sum_mm |mean_e Y_lmm(u_e)|^2 for one random shell: the identity and its normalisation."""
    case, _, r64 = cases.references()["random"]
    atom = int(np.argmax(r64.n_used >= 5))
    first = cases.first_atoms(case)
    b = int(np.searchsorted(first, atom, side="right") - 1)
    m = int(r64.n_used[atom])
    p = co.cb.positions_and_shifts(case.frac[first[b]:first[b + 1]].astype(np.float64), case.lattice[b].astype(np.float64), (0, 0, 0), np.float64)[0]
    disp, d2 = bo._bonds(p, case.lattice[b].astype(np.float64), atom - first[b], case.neighbors[atom, :m].astype(np.int64), np.float64)
    u = disp / np.sqrt(d2)[:, None]
    theta, phi = np.arccos(np.clip(u[:, 2], -1, 1)), np.arctan2(u[:, 1], u[:, 0])
    for k, l in enumerate(bo.L_VALUES):
        total = 0.0
        for mm in range(0, l + 1):
            mean = _sph_harm(l, mm, theta, phi).mean()
            total += (1 if mm == 0 else 2) * abs(mean) ** 2  # (|Y_l,-mm| = |Y_l,mm|)
        assert abs(4 * np.pi / (2 * l + 1) * total - r64.q2[atom, k]) <= 1e-12, l


def test_q_is_invariant_under_rotation_and_permutation():
    case, _, r64 = cases.references()["random"]
    c0 = cases.single(case, 0)
    rng = np.random.RandomState(5)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    # rotate the cell (float64 -> float32 would round: rotate in the float64 restatement's own domain by giving it float64)
    rot = bo.bond_order_reference_f64(c0.frac, c0.lattice, c0.counts, c0.cn, c0.neighbors)
    base = rot.q.copy()
    L = c0.lattice[0].astype(np.float64) @ Q
    frac64, n = c0.frac.astype(np.float64), c0.counts[0]
    p = co.cb.positions_and_shifts(frac64, L, (0, 0, 0), np.float64)[0]
    got = np.zeros_like(base)
    for i in range(n):
        m = int(min(c0.cn[i], c0.neighbors.shape[1]))
        perm = rng.permutation(m)
        disp, d2 = bo._bonds(p, L, i, c0.neighbors[i, :m][perm].astype(np.int64), np.float64)
        u = disp / np.sqrt(d2)[:, None]
        c = np.clip(u @ u.T, -1, 1)[np.triu_indices(m, 1)]
        got[i] = np.sqrt(np.maximum((m + 2 * bo._legendre(c, np.float64).sum(axis=1)) / (m * m), 0))
    assert np.abs(got - base).max() <= 1e-12


# ------------------------------------------------------------------------------------------------- float32 against float64
@pytest.mark.parametrize("name", [c.name for c in cases.all_cases()])
def test_float32_restatement_within_the_derived_bounds(name):
    case, r32, r64 = cases.references()[name]
    first = cases.first_atoms(case)
    assert (r32.flags == r64.flags).all() and (r32.n_used == r64.n_used).all()
    for k in ("q", "q2", "cos_min", "cos_max", "mean_q"):
        assert (np.isnan(getattr(r32, k)) == np.isnan(getattr(r64, k))).all(), k
    worst = 0.0
    for b, n in enumerate(case.counts):
        rows = slice(first[b], first[b + 1])
        if not np.isfinite(r64.c_bound[b]):
            continue
        with np.errstate(invalid="ignore"):
            dq2 = np.nan_to_num(np.abs(r32.q2[rows].astype(np.float64) - r64.q2[rows]))
            dc = np.nan_to_num(np.abs(np.stack([r32.cos_min[rows], r32.cos_max[rows]]).astype(np.float64) - np.stack([r64.cos_min[rows], r64.cos_max[rows]])))
        worst = max(worst, float((dq2 / r64.q2_bound[b][None, :]).max(initial=0.0)), float(dc.max(initial=0.0) / r64.c_bound[b]))
        assert (dq2 <= r64.q2_bound[b][None, :]).all() and (dc <= r64.c_bound[b]).all(), (name, b)
        for i in range(first[b], first[b + 1]):
            l1 = int(np.abs(r32.angles[i].astype(np.int64) - r64.angles[i]).sum())
            assert l1 <= (0 if r64.guarded[i] else 2 * r64.n_below[i]), (name, i, l1)
    print(name, "largest error / bound", worst)


def test_the_conditions_of_the_comparison_hold():
    """Decided by the float64 restatement alone: every atom of the known structures is guarded, at most a tenth of the random
    crystals' atoms are not."""
    _, _, known = cases.references()["known"]
    assert known.guarded.all()
    _, _, rnd = cases.references()["random"]
    share = 1.0 - rnd.guarded.mean()
    print("unguarded atoms of the random crystals:", int((~rnd.guarded).sum()), "of", rnd.guarded.size)
    assert share <= 0.1


def test_flags_and_sizes():
    refs = cases.references()
    _, r, _ = refs["shells"]
    assert list(r.flags) == [0, 0, bo.ISOLATED, 0, 0, 0, bo.OVERLAP]
    case = refs["shells"][0]
    first = cases.first_atoms(case)
    assert r.n_used[first[2]] == 0 and np.isnan(r.q[first[2]]).all() and np.isnan(r.mean_q[2]).all()
    assert list(r.n_used[first[3]:first[4]]) == [1, 1] and (r.q2[first[3]:first[4]] == 1).all() and np.isnan(r.cos_min[first[3]])
    assert r.n_used[first[4]] == 2 and _hist(r.angles[first[4]]) == {180: 1} and r.cos_min[first[4]] == r.cos_max[first[4]] == -1
    assert list(r.n_used[first[5]:first[6]]) == [2, 1, 1] and _hist(r.angles[first[5]]) == {105: 1}
    pair = slice(first[6], first[6] + 2)  # the coincident atoms: degenerate; the third atom of that crystal is computed
    assert np.isnan(r.q[pair]).all() and (r.angles[pair] == 0).all() and (r.n_used[pair] == 1).all() and np.isfinite(r.q[first[6] + 2]).all()
    _, r, _ = refs["full"]
    assert r.n_used[0] == 64 and r.angles[0].sum() == 2016 and r.flags[0] == 0 and r.flags[1] == bo.TRUNCATED
    assert refs["full"][0].cn[1] == 78 and r.n_used[1] == 64 and r.angles[1].sum() == 2016
    _, r, _ = refs["bad_list"]
    assert list(r.flags) == [0, bo.BAD_LIST, bo.BAD_LIST, 0]
    assert np.isnan(r.q[8:24]).all() and (r.n_used[8:24] == 0).all() and (r.angles[8:24] == 0).all() and np.isnan(r.mean_q[1:3]).all()
    assert (r.q[24:32].view(np.int32) == r.q[0:8].view(np.int32)).all()
    _, r, _ = refs["overflow"]
    assert list(r.flags) == [bo.TRUNCATED, bo.TRUNCATED] and list(r.n_used) == [4, 4]
    case, r, _ = refs["flags"]
    assert list(r.flags[:7]) == [0, bo.EMPTY, bo.NONFINITE, bo.OVERLAP, bo.ISOLATED, bo.ISOLATED, bo.NONFINITE]
    assert list(case.coord_flags[:7]) == [0, co.EMPTY, co.NONFINITE, co.OVERLAP, co.ISOLATED, co.CELL, co.NONFINITE]
    assert r.n_angles.sum() == r.angles.sum() and (r.angle_hist.sum(axis=1) == r.n_angles).all()


def test_constants():
    assert bo.L_VALUES == (2, 4, 6, 8) and bo.ANGLE_BINS == 37 and bo.COS_EDGES.shape == (36,) and bo.COS_EDGES.dtype == np.float32
    assert (np.diff(bo.COS_EDGES) < 0).all() and -1 < bo.COS_EDGES[-1] and bo.COS_EDGES[0] < 1
    assert list(bo.angle_centres()[[0, 12, 18, 36]]) == [0.0, 60.0, 90.0, 180.0]
    # 60, 90, 120 and 180 degrees sit in the middle of their bins
    c = np.cos(np.array([60.0, 90.0, 120.0, 180.0]) * np.pi / 180).astype(np.float32)
    assert list(bo._bins(c, bo.COS_EDGES)) == [12, 18, 24, 36]
    assert bo.describe(bo.OVERLAP | bo.TRUNCATED) == "OVERLAP|TRUNCATED" and bo.describe(0) == "ok"


# ----------------------------------------------------------------------------------------- header, binding, build list
def test_header_binding_and_build_agree():
    from arreau_amd import _hip, build
    header = open(os.path.join(ROOT, "include", "arreau_hip.h")).read()
    assert "arreau_crystal_bond_order" in _hip.EXPORTS and "bond_order.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "bond_order.hip"))
    for bit, name in bo.FLAG_NAMES:
        assert re.search(rf"#define ARREAU_BOND_{name} {bit}\b", header), name
    assert re.search(rf"#define ARREAU_BOND_ANGLE_BINS {bo.ANGLE_BINS}\b", header) and re.search(rf"#define ARREAU_BOND_ORDER_L {len(bo.L_VALUES)}\b", header)
    body = re.search(r"typedef struct arreau_bond_order_result \{(.*?)\} arreau_bond_order_result;", header, re.S).group(1)
    assert tuple(re.findall(r"\*\s*(\w+);", body)) == bo.RESULT_KEYS == tuple(n for n, _ in _hip.BondOrderResultC._fields_)
    body = re.search(r"typedef struct arreau_bond_order_params \{(.*?)\} arreau_bond_order_params;", header, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[[^\]]*\])?;", body) == [n for n, _ in _hip.BondOrderParamsC._fields_]
    import ctypes
    assert ctypes.sizeof(_hip.BondOrderParamsC) == 4 + 4 * (bo.ANGLE_BINS - 1)
    proto = re.search(r"int arreau_crystal_bond_order\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_hip._prototypes()["arreau_crystal_bond_order"]) == 10


# ------------------------------------------------------------------------------------------------ table, files, commands
def test_the_pinned_tables_are_unchanged_and_the_new_entry_is_in_the_new_one():
    assert [e.keyword for e in instruments.INSTRUMENTS] == ["screen", "unique", "find_symmetry", "reduce_cell", "symmetrize", "match_to"]
    assert [e.keyword for e in instruments.DERIVED] == ["conventional_cell"] and [e.keyword for e in instruments.LOCAL] == ["coordination"]
    assert instruments.ALL == instruments.INSTRUMENTS + instruments.DERIVED and instruments.EVERY == instruments.ALL + instruments.LOCAL
    assert list(instruments.BY_KEYWORD) == [e.keyword for e in instruments.EVERY]
    assert [e.keyword for e in instruments.SHELL] == ["bond_order"] and instruments.TABLE == instruments.EVERY + instruments.SHELL
    assert list(instruments.KEYWORDS) == [e.keyword for e in instruments.TABLE]
    e = instruments.KEYWORDS["bond_order"]
    assert (e.field, e.prefix, e.stats_key, e.keys) == ("bond_order", "order_", "bond_order_stats", bo.STORED_KEYS)
    assert e.atom_keys == bo.ATOM_KEYS and dict(e.shapes)["angles"] == (37,) and dict(e.shapes)["q"] == (4,)


def _stored(name="shells"):
    case, r32, _ = cases.references()[name]
    arrays = {k: getattr(r32, k) for k in bo.RESULT_KEYS}
    arrays["coord_flags"] = case.coord_flags if case.coord_flags is not None else np.zeros(len(case.counts), np.int32)  # (hand-made lists)
    return case, bo.sample_arrays(arrays, case.species)


def _sample_result(case, stored):
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    counts = np.asarray(case.counts, dtype=np.int64)
    return SampleResult(frac_x=case.frac.astype(np.float64), atomic_numbers=case.species.astype(np.float64), lattice=case.lattice.astype(np.float64),
                        num_atoms=counts, idx_start=np.cumsum(counts) - counts, bond_order=stored)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


def test_file_round_trip_select_and_concat(tmp_path):
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    from arreau_amd.generate import concat_results, select_crystals
    case, stored = _stored()
    assert tuple(stored) == bo.STORED_KEYS
    res = _sample_result(case, stored)
    name = save_sample_results_to_hdf5(res, str(tmp_path / "crystals.npz"))
    with np.load(name) as z:
        assert [k for k in z.files if k.startswith("order_")] == ["order_" + k for k in bo.STORED_KEYS]
    back = load_sample_results_from_hdf5(name)
    _same(back.bond_order, stored)
    assert back.coordination is None
    keep = np.array([True, False, True, True, False, False, True])
    first = cases.first_atoms(case)
    part = select_crystals(res, keep)
    atoms = np.repeat(keep, case.counts)
    _same(part.bond_order, {k: v[atoms if k in bo.ATOM_KEYS else keep] for k, v in stored.items()})
    rest = select_crystals(res, ~keep)
    both = concat_results([part, rest])
    order = np.concatenate([np.flatnonzero(keep), np.flatnonzero(~keep)])
    atom_order = np.concatenate([np.arange(first[b], first[b + 1]) for b in order])
    _same(both.bond_order, {k: v[atom_order if k in bo.ATOM_KEYS else order] for k, v in stored.items()})
    bad = dict(stored, q=stored["q"][:, :3])
    with pytest.raises(ValueError, match="bond_order"):
        save_sample_results_to_hdf5(_sample_result(case, bad), str(tmp_path / "bad.npz"))


def test_statistics_lines():
    case, stored = _stored("known")
    st = bo.stats_of(stored, 1)
    _, r32, _ = cases.references()["known"]
    assert st["crystals"] == len(case.counts) and st["atoms"] == len(case.species) and st["n_angles"] == int(r32.n_angles.sum())
    assert st["angles"] == _hist(r32.angle_hist.sum(axis=0)) and set(st["elements"]) == set(int(z) for z in case.species)
    line = bo.format_stats(st)
    q4 = r32.q[:, 1].astype(np.float64).mean()
    assert line.startswith(f"bond order rank 1: {len(case.counts)} crystals, {len(case.species)} atoms; angles ") and f"mean q4 {q4:.3f}, q6 " in line
    assert " 90: " in line and "Z 29: 0.191 / 0.575" in line and line.endswith("flags none")
    lines = bo.summary_lines([bo.stats_of(stored, 1), bo.stats_of(stored, 0)])
    assert [l.split(":")[0] for l in lines] == ["bond order rank 0", "bond order rank 1", "bond order total"]
    assert f"{2 * len(case.species)} atoms" in lines[2] and f"({2 * st['n_angles']} pairs)" in lines[2]
    # the atoms of blanked crystals are left out; the flags are counted
    _, stored = _stored("bad_list")
    st = bo.stats_of(stored)
    assert st["atoms"] == 16 and st["computed"] == 2 and st["flags"]["BAD_LIST"] == 2
    assert "flags BAD_LIST 2" in bo.format_stats(st)
    _, stored = _stored("flags")
    st = bo.stats_of(stored)
    assert st["computed"] == len(stored["flags"]) - 3  # two NONFINITE, one CELL of the search
    assert instruments.summary_lines(instruments.KEYWORDS["bond_order"], stored)[-1].startswith("bond order total")


def test_parameters_and_parser_flags():
    from arreau_amd import generate, screen
    p = bo.BondOrderParams(tol=0.2, cutoff=5)
    assert p.coordination() == co.CoordinationParams(tol=0.2, cutoff=5.0) and isinstance(p.cutoff, float)
    for bad in (dict(tol=-1), dict(cutoff=0), dict(max_neighbors=65), dict(max_neighbors=0), dict(max_shells=9), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            bo.BondOrderParams(**bad)
    assert bo.resolve(None) is None and bo.resolve(False) is None and bo.resolve(True) == bo.BondOrderParams() and bo.resolve(p) is p
    with pytest.raises(ValueError):
        bo.resolve(co.CoordinationParams())
    bo.check_shared(p, None), bo.check_shared(None, co.CoordinationParams()), bo.check_shared(p, p.coordination())
    with pytest.raises(ValueError, match="must agree"):
        bo.check_shared(p, co.CoordinationParams())
    for parser, argv in ((generate.build_parser(), ["--model_path", "m.ckpt"]), (screen.build_parser(), ["file.npz"])):
        args = parser.parse_args(argv)
        assert args.bond_order is False
        args = parser.parse_args(argv + ["--bond_order", "--cn_tol", "0.25", "--cn_cutoff", "4.5"])
        assert args.bond_order is True
        errors = []
        got = generate.instrument_params("bond_order", args, errors.append)
        assert got == bo.BondOrderParams(tol=0.25, cutoff=4.5) and not errors
        assert generate.instrument_params("coordination", args, errors.append) == got.coordination()
        args = parser.parse_args(argv + ["--bond_order", "--cn_cutoff", "-1"])
        assert generate.instrument_params("bond_order", args, errors.append) is None and errors and errors[0].startswith("bond order: ")


def test_sample_signatures():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss, SampleResult
    from arreau_amd.engine import HipEngine
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    for fn in (DiffusionLoss.sample, PONITA_DIFFUSION.sample):
        assert inspect.signature(fn).parameters["bond_order"].default is None
    assert SampleResult.__dataclass_fields__["bond_order"].default is None
    assert list(inspect.signature(HipEngine.bond_order).parameters)[1:] == ["frac", "lattice", "offsets", "params", "coordination_result"]
    from arreau_amd import engine
    assert list(inspect.signature(engine.bond_order).parameters) == ["frac", "lattice", "offsets", "params"]
