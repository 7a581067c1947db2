"""The Voronoi construction on the device (arreau_crystal_voronoi, csrc/voronoi.hip) on the batches of tests/voronoi_cases.py:
against the float64 restatement (integers, flags and the neighbour list equal on the guarded atoms, the reals within the bounds
measured on the CPU by tools/exp/voronoi_f32_deviation.py -- never from the kernel's output), a crystal alone against the same
crystal inside the 70-crystal batch and two launches bit for bit, closure, reciprocity and the sum of volumes on the device's own
numbers, sample(voronoi=...), the bond order on Voronoi shells, the two command lines, the argument errors and the export.  Needs
an MI355X: `-m gpu`."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import bond_order as bo
from arreau_amd.diffusion import voronoi as vo
from tests import voronoi_cases as cases
from tests.sampling_helpers import S, T, dev, fused_model, model_seed  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR_PI = 4.0 * np.pi
PER_ATOM_REALS = ("volume", "omega_sum", "max_radius", "cn_eff")
_RUN = {}


def up(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def device_batch(dev, bt):
    off = np.concatenate([[0], np.cumsum(bt.counts)]).astype(np.int32)
    return up(dev, bt.frac.reshape(-1, 3)), up(dev, bt.lattice), up(dev, off)


def launch(dev, bt):
    return vo.result_to_numpy(vo.voronoi(*device_batch(dev, bt), bt.params))


def run(dev, name):
    """The kernel's arrays of one named batch (one launch each, cached)."""
    if name not in _RUN:
        _RUN[name] = launch(dev, cases.reference(name)[0])
    return _RUN[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def first_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def is_closed(flags, omega):
    return ~np.isnan(omega) & ((flags & (vo.OPEN | vo.OVERLAP | vo.OVERFLOW)) == 0)


@pytest.mark.parametrize("name", cases.NAMES)
def test_kernel_matches_the_float64_restatement(dev, name):
    bt, r = cases.reference(name)
    got = run(dev, name)
    assert set(got) == set(vo.RESULT_KEYS)
    for k in vo.RESULT_KEYS:
        want = getattr(r, k)
        assert got[k].shape == want.shape and got[k].dtype == (np.int32 if k in vo.INTEGER_KEYS else np.float32), (name, k, got[k].dtype, got[k].shape)
    first, crystal = first_of(bt.counts), np.repeat(np.arange(len(bt.counts)), bt.counts)
    built = np.array([m is not None for m in r.margins], dtype=bool)  # a cell was built: the others are blank in both
    decided = r.guarded | ~built
    # integers, flags and the neighbour list on the guarded atoms (and on the atoms nothing was built for)
    for k in ("cn", "atom_flags", "neighbors"):
        assert np.array_equal(got[k][decided], getattr(r, k)[decided]), (name, k, np.flatnonzero((got[k] != getattr(r, k)).reshape(len(built), -1).any(axis=1) & decided)[:8])
    whole = np.array([decided[first[b]:first[b + 1]].all() for b in range(len(bt.counts))], dtype=bool)
    for k in ("n_faces", "min_cn", "max_cn", "flags"):
        assert np.array_equal(got[k][whole], getattr(r, k)[whole]), (name, k)
    if bt.expect["flags"] is not None:
        assert got["flags"].tolist() == bt.expect["flags"], name
    if bt.expect["cn"] is not None:
        assert got["cn"].tolist() == bt.expect["cn"], name
    # blank atoms: NaN where the restatement has NaN
    for k in PER_ATOM_REALS + vo.FACE_KEYS:
        assert np.array_equal(np.isnan(got[k][decided]), np.isnan(getattr(r, k)[decided])), (name, k)
    # the reals within the measured bounds: a closed atom is held to the closed atoms' bound
    closed_b, any_b = cases.bounds(bt)
    shut = is_closed(r.atom_flags, r.omega_sum)
    worst = {}
    for a in np.flatnonzero(r.guarded):
        bound = closed_b if shut[a] else any_b
        k_ = min(int(r.cn[a]), bt.params.max_faces)
        for k in vo.FACE_KEYS:
            err = np.abs(got[k][a, :k_].astype(np.float64) - getattr(r, k)[a, :k_]).max(initial=0.0)
            worst[k] = max(worst.get(k, 0.0), err / bound[k][crystal[a]])
            assert err <= bound[k][crystal[a]], (name, k, a, err, bound[k][crystal[a]])
        for k in PER_ATOM_REALS:
            err = abs(float(got[k][a]) - float(getattr(r, k)[a]))
            worst[k] = max(worst.get(k, 0.0), err / bound[k][crystal[a]])
            assert err <= bound[k][crystal[a]], (name, k, a, err, bound[k][crystal[a]])
    print(name, "largest error / bound:", {k: round(v, 4) for k, v in worst.items()})
    # per crystal, where every atom is guarded: mean_cn one float32 division, the two sums within their atoms' bounds
    for b in np.flatnonzero(whole & (np.array(bt.counts) > 0) & ~np.isnan(r.volume_sum)):
        n = bt.counts[b]
        bound = closed_b if shut[first[b]:first[b + 1]].all() else any_b
        assert abs(float(got["mean_cn"][b]) - float(r.mean_cn[b])) <= 2.0 ** -23 * max(float(r.mean_cn[b]), 1.0), (name, b)
        assert abs(float(got["mean_cn_eff"][b]) - float(r.mean_cn_eff[b])) <= bound["cn_eff"][b] + 2.0 ** -22 * n * float(r.mean_cn_eff[b]), (name, b)
        assert abs(float(got["volume_sum"][b]) - float(r.volume_sum[b])) <= n * bound["volume"][b] + 2.0 ** -22 * n * float(r.volume_sum[b]), (name, b)
    want_guarded = {"known": 29, "known half": 29, "one atom": 1, "skewed": 1, "flags": 2, "overflow": 0, "truncated": 2, "ragged": 1200, "large": 244}
    want_guarded.update(cases.WANT_GUARDED)  # (the batches at the caps: 95 % of the atoms a cell is built for, test_voronoi_cpu.py)
    assert r.guarded.sum() >= want_guarded[name]  # (the comparison is not vacuous: at least 95 % of the ragged and large atoms)


def test_paths_and_flags_on_the_device(dev):
    got = run(dev, "flags")
    bt = cases.reference("flags")[0]
    first = first_of(bt.counts)
    assert got["flags"].tolist() == [vo.NONFINITE, vo.CELL, vo.EMPTY, vo.OVERLAP, vo.OPEN, 0]
    assert np.isnan(got["volume"][:first[4]]).all() and (got["cn"][:first[4]] == 0).all() and (got["neighbors"][:first[4]] == -1).all()
    assert got["atom_flags"][first[3]:first[4]].tolist() == [vo.OVERLAP] * 2 and got["atom_flags"][first[4]] == vo.OPEN and got["omega_sum"][first[4]] == 0
    assert got["min_cn"][2] == -1 and np.isnan(got["mean_cn"][2]) and got["cn"][first[5]] == 12
    over = run(dev, "overflow")
    assert over["flags"].tolist() == [vo.OVERFLOW] and over["cn"].tolist() == [0] and np.isnan(over["volume"][0]) and (over["neighbors"] == -1).all()
    cut = run(dev, "truncated")
    assert cut["flags"].tolist() == [vo.TRUNCATED] * 2 and cut["cn"].tolist() == [12, 6] and cut["neighbors"].shape == (2, 4, 4) and (cut["neighbors"][:, :, 0] == 0).all()
    large, lb = run(dev, "large"), cases.reference("large")[0]
    assert lb.counts == [vo.cb.STAGED_ATOMS + 1] and is_closed(large["atom_flags"], large["omega_sum"]).sum() >= 100
    known = run(dev, "known")
    kb = cases.reference("known")[0]
    at = lambda name: first_of(kb.counts)[cases.KNOWN_NAMES.index(name)]
    assert known["cn"][at("simple_cubic")] == 6 and known["cn"][at("fcc_primitive")] == 12 and known["cn"][at("bcc_primitive")] == 14
    assert run(dev, "known half")["cn"][at("bcc_primitive")] == 8 and (known["flags"] == 0).all()
    # tol = 0: every face counts, a zero-area face weighs 0 (never a negative or NaN weight), cn_eff is still 6
    one = cases.single(kb, cases.KNOWN_NAMES.index("simple_cubic"))
    one.params = vo.VoronoiParams(cutoff=5.3, tol=0.0, max_faces=64)
    zero = launch(dev, one)
    w = zero["face_weight"][0, :zero["cn"][0]]
    assert zero["cn"][0] > 6 and (w >= 0).all() and (np.sort(w)[-6:] > 0.999).all() and (np.sort(w)[:-6] < 1e-5).all()
    assert abs(float(zero["cn_eff"][0]) - 6.0) < 1e-4 and zero["flags"][0] == 0
    # no crystals at all: nothing is launched
    empty = vo.voronoi(torch.empty((0, 3), device=dev), torch.empty((0, 3, 3), device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
    assert empty["flags"].shape == (0,) and empty["neighbors"].shape == (0, 32, 4) and empty["face_area"].shape == (0, 32)


def test_a_crystal_alone_gives_the_bits_it_gives_in_the_batch(dev):
    bt = cases.reference("ragged")[0]
    got = run(dev, "ragged")
    assert len(bt.counts) == 70 and bt.counts[cases.RAGGED_BIG] == 67
    first = first_of(bt.counts)
    for b in (cases.RAGGED_BIG, 0, 69):
        alone = launch(dev, cases.single(bt, b))
        for k in vo.CRYSTAL_KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(got[k][b])), (b, k)
        for k in vo.RESULT_KEYS[len(vo.CRYSTAL_KEYS):]:
            assert np.array_equal(bits(alone[k]), bits(got[k][first[b]:first[b + 1]])), (b, k)
    again = launch(dev, bt)  # and a second launch of the whole batch
    for k in vo.RESULT_KEYS:
        assert np.array_equal(bits(again[k]), bits(got[k])), k


@pytest.mark.parametrize("name", ["known", "ragged", "large", "cages", "hub40", "hub70"])
def test_closure_reciprocity_and_volumes_on_the_device(dev, name):
    """The device's own numbers: on every closed atom omega_sum is 4 pi within the bound (the float64 restatement's is 4 pi to
    1e-10), the volumes of a crystal closed in all its atoms sum to the cell's, and a stored face's partner has its area.  On the
    batches at the caps each of the three is allowed what the float64 restatement itself misses it by: the cages' float32
    coordinates split the vertex at the cage's centre by 1e-7 A, and the restatement closes them to 2e-5 in omega_sum, to 8e-7 of
    the volume and to 2e-5 A^2 between partners (the hubs: to 1e-14; test_voronoi_cpu.py)."""
    caps = name in cases.NEW_NAMES
    bt, r = cases.reference(name)
    got = run(dev, name)
    closed_b, _ = cases.bounds(bt)
    first, crystal = first_of(bt.counts), np.repeat(np.arange(len(bt.counts)), bt.counts)
    shut = is_closed(got["atom_flags"], got["omega_sum"]) & r.guarded
    assert shut.sum() >= {"known": 29, "ragged": 400, "large": 100, "cages": 77, "hub40": 46, "hub70": 75}[name]
    err = np.abs(got["omega_sum"][shut].astype(np.float64) - FOUR_PI)
    slack = 1e-6 if name == "known" else 0.0  # (ideal hcp in float32: its split vertices close the cell to 4e-7 only, in float64 too)
    own = np.abs(r.omega_sum[shut] - FOUR_PI) if caps else 0.0
    assert (err <= closed_b["omega_sum"][crystal[shut]] + slack + own).all(), (name, float(err.max()))
    whole = 0
    for b, n in enumerate(bt.counts):
        if n and shut[first[b]:first[b + 1]].all():
            vol = abs(np.linalg.det(bt.lattice[b].astype(np.float64)))
            total = got["volume"][first[b]:first[b + 1]].astype(np.float64).sum()
            own = abs(float(r.volume_sum[b]) - vol) if caps else 0.0
            assert abs(total - vol) <= n * closed_b["volume"][b] + 1e-6 * vol + own, (name, b, total, vol)
            assert abs(float(got["volume_sum"][b]) - vol) <= n * closed_b["volume"][b] + 1e-6 * vol + 2.0 ** -22 * n * vol + own
            whole += 1
    assert whole >= {"known": 8, "ragged": 1, "large": 0, "cages": 4, "hub40": 0, "hub70": 1}[name]
    pairs = 0
    for b, n in enumerate(bt.counts):
        for i in range(n):
            a = first[b] + i
            if not shut[a]:
                continue
            for s in range(min(int(got["cn"][a]), bt.params.max_faces)):
                j, n1, n2, n3 = got["neighbors"][a, s]
                c = first[b] + j
                if not shut[c]:
                    continue
                back = np.flatnonzero((got["neighbors"][c] == np.array([i, -n1, -n2, -n3])).all(axis=1))
                if back.size == 0:  # the partner weighs less than tol on its own atom, or lies past that atom's max_faces (hub70's
                    # centre keeps 64 of 70): not stored there (the restatement agrees)
                    kept = [(jj, im) for (jj, im, _, _, _), w in zip(r.faces[c], faces_weights(r, c)) if w >= bt.params.tol]
                    assert (i, (-n1, -n2, -n3)) not in kept[:bt.params.max_faces], (name, b, i, j)
                    continue
                assert back.size == 1
                own = abs(float(r.face_area[a, s]) - float(r.face_area[c, back[0]])) if caps else 0.0  # (both guarded: the same rows there)
                assert abs(float(got["face_area"][a, s]) - float(got["face_area"][c, back[0]])) <= 2.0 * closed_b["face_area"][b] + slack + own, (name, b, i, j)
                assert got["face_distance"][a, s] == got["face_distance"][c, back[0]] or \
                    abs(float(got["face_distance"][a, s]) - float(got["face_distance"][c, back[0]])) <= 2.0 * closed_b["face_distance"][b]
                pairs += 1
    assert pairs >= {"known": 200, "ragged": 1000, "large": 500, "cages": 400, "hub40": 300, "hub70": 400}[name]


def faces_weights(r, a):
    """The weights of atom a's kept faces in the float64 restatement, in their order."""
    top = max((om for _, _, _, _, om in r.faces[a]), default=0.0)
    return [om / top if top > 0 else 0.0 for _, _, _, _, om in r.faces[a]]


def assert_blank(got, a, flags):
    """Atom a has no cell: cn 0, its flags, the reals NaN, the list -1."""
    assert got["cn"][a] == 0 and got["atom_flags"][a] == flags, (a, got["cn"][a], got["atom_flags"][a])
    assert all(np.isnan(got[k][a]).all() for k in PER_ATOM_REALS + vo.FACE_KEYS) and (got["neighbors"][a] == -1).all(), a


def assert_same_atoms(x, y, atoms):
    for k in vo.RESULT_KEYS[len(vo.CRYSTAL_KEYS):]:
        assert np.array_equal(bits(x[k][atoms]), bits(y[k][atoms])), k


def test_the_caps_on_the_device(dev):
    """What the batches at the caps are for, read off the device's arrays (the numbers are the float64 restatement's,
    test_voronoi_cpu.py): a face of more than 64 vertex copies is built, one of more than 128 is OVERFLOW; 40 rows stored and the
    rest blank; 70 faces counted and 64 stored."""
    bt, r = cases.reference("cages")
    got, first = run(dev, "cages"), first_of(bt.counts)
    assert got["flags"].tolist() == [0, 0, 0, 0, vo.OVERFLOW, 0]
    c16, c17, c18, c20 = (cases.CAGE_NAMES.index(n) for n in ("cage16", "cage17", "cage18", "cage20"))
    for b, n_cage in ((c16, 16), (c17, 17), (c18, 18)):
        sl = slice(first[b], first[b] + n_cage)
        assert (r.max_vertices[sl] > 64).all() and (got["atom_flags"][sl] == 0).all() and np.array_equal(got["cn"][sl], r.cn[sl])
    full = first[c18] + np.flatnonzero(r.max_vertices[first[c18]:first[c18 + 1]] == vo.FACE_VERTICES)  # exactly 128 copies: built
    assert full.size >= 1 and r.guarded[full].all() and (got["atom_flags"][full] == 0).all() and not np.isnan(got["volume"][full]).any()
    for a in range(first[c20], first[c20] + 20):
        assert r.max_vertices[a] > vo.FACE_VERTICES and r.n_candidates[a] <= vo.MAX_CANDIDATES
        assert_blank(got, a, vo.OVERFLOW)
    fill = slice(first[c20] + 20, first[c20 + 1])
    assert (got["atom_flags"][fill] == 0).all() and np.array_equal(got["cn"][fill], r.cn[fill]) and not np.isnan(got["volume"][fill]).any()
    assert np.isnan(got["volume_sum"][c20]) and got["min_cn"][c20] == 0 and got["n_faces"][c20] == r.cn[fill].sum()
    bt, r = cases.reference("hub40")
    got = run(dev, "hub40")
    assert r.cn[0] == 40 and got["cn"][0] == 40 and got["flags"].tolist() == [0] and got["neighbors"].shape == (48, 64, 4)
    assert np.array_equal(got["neighbors"][0], r.neighbors[0]) and (got["neighbors"][0, :40, 0] > 0).all() and (got["neighbors"][0, 40:] == -1).all()
    assert all(np.isnan(got[k][0, 40:]).all() and not np.isnan(got[k][0, :40]).any() for k in vo.FACE_KEYS)
    bt, r = cases.reference("hub70")
    got = run(dev, "hub70")
    assert r.cn[0] == 70 and got["cn"][0] == 70 and got["atom_flags"][0] == vo.TRUNCATED and got["flags"].tolist() == [vo.TRUNCATED]
    assert np.array_equal(got["neighbors"][0], r.neighbors[0]) and (got["neighbors"][0, :, 0] > 0).all() and (got["atom_flags"][1:] == 0).all()
    assert not any(np.isnan(got[k][0]).any() for k in vo.FACE_KEYS) and got["max_cn"][0] == 70
    assert abs(float(got["volume_sum"][0]) - 729.0) <= 78 * cases.bounds(bt)[0]["volume"][0] + 2.0 ** -22 * 78 * 729.0


def test_max_candidates_at_the_largest_count_and_one_below(dev):
    """hub70 with room for exactly its largest candidate count (the restatement's: 108) gives the bits it gives with room for 128;
    with room for one less exactly the atoms that have that many are OVERFLOW and blank, and every other atom keeps its bits."""
    bt, r = cases.reference("hub70")
    got, top = run(dev, "hub70"), int(r.n_candidates.max())
    full = r.n_candidates == top
    assert 64 < top < vo.MAX_CANDIDATES and 1 <= full.sum() < len(full)
    exact = launch(dev, cases.with_params(bt, max_candidates=top))
    for k in vo.RESULT_KEYS:
        assert np.array_equal(bits(exact[k]), bits(got[k])), k
    less = launch(dev, cases.with_params(bt, max_candidates=top - 1))
    for a in np.flatnonzero(full):
        assert_blank(less, a, vo.OVERFLOW)
    assert_same_atoms(less, got, ~full)
    assert less["flags"].tolist() == [int(got["flags"][0]) | vo.OVERFLOW] and less["n_faces"][0] == got["cn"][~full].sum()
    assert less["min_cn"][0] == 0 and less["max_cn"][0] == got["cn"][~full].max() and np.isnan(less["volume_sum"][0]) and np.isnan(less["mean_cn_eff"][0])


def test_the_hard_cap_of_128_candidates(dev):
    """One crystal at two cutoffs 0.009 A apart: at the first its densest atom has exactly 128 candidates (the last slot of the
    wave's slice) and is built as the restatement builds it (test_kernel_matches_the_float64_restatement holds its numbers); at
    the second it has 129 and is OVERFLOW, while the atom that now has exactly 128 is built."""
    bt, r = cases.reference("hard cap")
    got, a, nxt = run(dev, "hard cap"), cases.HARD_CAP_ATOM, cases.HARD_CAP_NEXT
    assert r.n_candidates[a] == r.n_candidates.max() == vo.MAX_CANDIDATES and r.guarded[a] and r.atom_flags[a] == 0
    assert got["flags"].tolist() == [0] and got["atom_flags"][a] == 0 and got["cn"][a] == r.cn[a] > 0 and np.array_equal(got["neighbors"][a], r.neighbors[a])
    over = cases.hard_cap_batch(cases.HARD_CAP_OVER)
    count = cases.candidate_counts(over)
    assert count[a] == count.max() == vo.MAX_CANDIDATES + 1 and count[nxt] == vo.MAX_CANDIDATES and (np.delete(count, a) <= vo.MAX_CANDIDATES).all()
    more = launch(dev, over)
    assert_blank(more, a, vo.OVERFLOW)
    rest = np.delete(np.arange(len(count)), a)
    assert more["flags"][0] & vo.OVERFLOW and ((more["atom_flags"][rest] & vo.OVERFLOW) == 0).all() and not np.isnan(more["volume"][rest]).any()
    assert more["cn"][nxt] >= r.cn[nxt] > 0 and more["atom_flags"][nxt] == r.atom_flags[nxt] == 0  # (a plane more cuts no face open)


def sweep(dev, bt, r, got, values):
    """max_faces alone changes: cn, the flags and the stored rows are the restatement's, cut (cases.cut), on the atoms it decides;
    the rows past cn are blank; every stored real and per-atom real has the bits of the launch `got` with the longest list."""
    built = np.array([m is not None for m in r.margins], dtype=bool)
    decided = r.guarded | ~built
    for mf in values:
        one = launch(dev, cases.with_params(bt, max_faces=mf))
        want = cases.cut(r, mf)
        assert one["neighbors"].shape == (len(r.cn), mf, 4)
        for k in ("cn", "atom_flags", "neighbors"):
            assert np.array_equal(one[k][decided], getattr(want, k)[decided]), (mf, k)
        assert np.array_equal((one["atom_flags"] & vo.TRUNCATED) != 0, one["cn"] > mf), mf
        beyond = np.arange(mf)[None, :] >= one["cn"][:, None]
        assert (one["neighbors"][beyond] == -1).all() and (one["neighbors"][~beyond][:, 0] >= 0).all(), mf
        for k in vo.FACE_KEYS:
            assert np.isnan(one[k][beyond]).all() and np.array_equal(bits(one[k]), bits(got[k][:, :mf])), (mf, k)
        for k in PER_ATOM_REALS + ("cn",):
            assert np.array_equal(bits(one[k]), bits(got[k])), (mf, k)
        assert np.array_equal(one["neighbors"], got["neighbors"][:, :mf]) and one["n_faces"][0] == got["n_faces"][0]
        assert one["flags"][0] == (int(got["flags"][0]) & ~vo.TRUNCATED) | (vo.TRUNCATED if (one["cn"] > mf).any() else 0), mf


def test_max_faces_sweeps(dev):
    """fcc at max_faces 1..13 (12 faces: the cut inside the first 64 candidates, then none), hub40 about the number of faces its
    centre (40, all among its first 64 candidates) and a filler (18 of 25) have among their first 64 candidates, and hub70 about
    its centre's (59 of 70): the cut inside the first call of the kernel's store(), exactly between the two and inside the second."""
    kb, kr = cases.reference("known")
    b = cases.KNOWN_NAMES.index("fcc_primitive")
    at = slice(first_of(kb.counts)[b], first_of(kb.counts)[b + 1])
    fcc = cases.single(kb, b)
    one_r = cases.atoms(kr, at)
    assert one_r.cn.tolist() == [12]
    sweep(dev, fcc, one_r, launch(dev, fcc), range(1, 14))
    for name in ("hub40", "hub70"):
        bt, r = cases.reference(name)
        sweep(dev, bt, r, run(dev, name), cases.SWEEPS[name])


def test_a_cage_alone_gives_the_bits_it_gives_in_the_batch(dev):
    bt = cases.reference("cages")[0]
    got, first = run(dev, "cages"), first_of(bt.counts)
    assert first[1] > 0
    for name in ("cage16", "cage17", "cage18", "cage20"):
        b = cases.CAGE_NAMES.index(name)
        alone = launch(dev, cases.single(bt, b))
        for k in vo.CRYSTAL_KEYS:
            assert np.array_equal(bits(alone[k][0]), bits(got[k][b])), (name, k)
        for k in vo.RESULT_KEYS[len(vo.CRYSTAL_KEYS):]:
            assert np.array_equal(bits(alone[k]), bits(got[k][first[b]:first[b + 1]])), (name, k)


def test_two_launches_of_hub70_give_the_same_bits(dev):
    bt = cases.reference("hub70")[0]
    got, again = run(dev, "hub70"), launch(dev, bt)
    for k in vo.RESULT_KEYS:
        assert np.array_equal(bits(again[k]), bits(got[k])), k


def test_sample_with_voronoi(dev, fused_model):
    m, _ = fused_model
    params = vo.VoronoiParams(tol=0.1, cutoff=5.0, max_faces=16)
    out = []
    for kw in ({}, dict(voronoi=True), dict(voronoi=None), dict(voronoi=params, coordination=True, bond_order=True, screen=True, reduce_cell=True),
               dict(coordination=True, bond_order=True, screen=True, reduce_cell=True)):
        torch.manual_seed(3)
        np.random.seed(3)
        r = m.sample([4, 7, 1], 3, seed=777, max_steps=6, **kw)
        out.append((r, torch.random.get_rng_state(), np.random.uniform()))
    plain = out[0][0]
    for r, rng, after in out[1:]:
        assert np.array_equal(plain.frac_x, r.frac_x) and np.array_equal(plain.atomic_numbers, r.atomic_numbers)
        assert np.array_equal(plain.lattice, r.lattice) and np.array_equal(plain.num_atoms, r.num_atoms)
        assert torch.equal(out[0][1], rng) and out[0][2] == after
    a, none, every, others = out[1][0], out[2][0], out[3][0], out[4][0]
    assert plain.voronoi is None and none.voronoi is None and others.voronoi is None
    assert a.metrics is None and a.coordination is None and a.bond_order is None and a.reduced is None
    for field in ("metrics", "reduced", "coordination", "bond_order"):  # every other instrument's arrays: as without the keyword
        x, y = getattr(every, field), getattr(others, field)
        assert set(x) == set(y)
        for k in x:
            assert np.array_equal(bits(np.asarray(x[k])), bits(np.asarray(y[k]))), (field, k)
    for r, p in ((a, None), (every, params)):  # the engine-free entry point on the returned crystals
        c = r.voronoi
        assert set(c) == set(vo.STORED_KEYS) and c["cn"].shape == (12,) and c["flags"].shape == (3,)
        assert c["neighbors"].shape == (12, 32 if p is None else 16, 4) and np.array_equal(c["species"], np.rint(r.atomic_numbers).astype(np.int64))
        direct = vo.voronoi_sample_result(r, p, dev)
        for k in vo.STORED_KEYS:
            assert np.array_equal(bits(c[k]), bits(direct[k])), k
        ref = vo.voronoi_reference(r.frac_x, r.lattice, r.num_atoms, p)
        g = ref.guarded
        for k in ("cn", "atom_flags", "neighbors"):
            assert np.array_equal(c[k][g], getattr(ref, k)[g]), k


def test_bond_order_on_voronoi_shells(dev):
    """from_voronoi: the Voronoi list of fcc gives q6 = 0.575 and the 60 / 90 / 120 / 180 degree counts of twelve cuboctahedral
    bonds (24, 12, 24, 6); the bcc list at tol 0.05 has 14 bonds."""
    bt = cases.reference("known")[0]
    frac, lattice, off = device_batch(dev, bt)
    v = vo.voronoi(frac, lattice, off, bt.params)
    got = bo.result_to_numpy(bo.from_voronoi(frac, lattice, off, v))
    assert set(bo.RESULT_KEYS) <= set(got) and "coord_flags" not in got
    first = first_of(bt.counts)
    fcc, bcc = first[cases.KNOWN_NAMES.index("fcc_primitive")], first[cases.KNOWN_NAMES.index("bcc_primitive")]
    assert got["n_used"][fcc] == 12 and abs(float(got["q"][fcc, bo.L_VALUES.index(6)]) - 0.57452) < 5e-4
    assert abs(float(got["q"][fcc, bo.L_VALUES.index(4)]) - 0.19094) < 5e-4
    hist = {int(5 * k): int(c) for k, c in enumerate(got["angles"][fcc]) if c}
    assert hist == {60: 24, 90: 12, 120: 24, 180: 6}
    assert got["n_used"][bcc] == 14 and int(got["angles"][bcc].sum()) == 14 * 13 // 2
    # the same launch as from_coordination on the same arrays
    same = bo.result_to_numpy(bo.from_coordination(frac, lattice, off, {"cn": v["cn"], "neighbors": v["neighbors"]}))
    for k in bo.RESULT_KEYS:
        assert np.array_equal(bits(same[k]), bits(got[k])), k
    half = vo.voronoi(frac, lattice, off, cases.KNOWN_HALF)
    assert bo.result_to_numpy(bo.from_voronoi(frac, lattice, off, half))["n_used"][bcc] == 8


def _child(argv, seconds):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-m"] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=seconds + 30)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_command_lines_write_and_print_the_same_numbers(dev, tmp_path):
    """generate --voronoi, then screen --voronoi --out on the file it wrote: each a fresh process."""
    from arreau_amd.checkpoint import make_synthetic_model, save_lightning_checkpoint
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.diffusion.inference.process_generated_crystals import load_sample_results_from_hdf5, save_sample_results_to_hdf5
    ckpt = save_lightning_checkpoint(str(tmp_path / "last.ckpt"), make_synthetic_model(S=S, seed=3, num_timesteps=T))
    out, out2 = str(tmp_path / "out" / "crystals.npz"), str(tmp_path / "again.npz")
    flags = ["--voronoi", "--vor_tol", "0.1", "--vor_cutoff", "5.5"]
    text = _child(["arreau_amd.generate", "--model_path", ckpt, "--num_crystals", "5", "--num_atoms", "6", "--batch", "4", "--num_steps", "10",
                   "--seed", "5", "--out", out] + flags, 300)
    lines = [ln for ln in text.splitlines() if ln.startswith("voronoi ")]
    assert len(lines) == 2 and re.match(r"voronoi rank 0: 5 crystals, \d+ atoms; cn ", lines[0]) and lines[1].startswith("voronoi total: 5 crystals"), text
    assert "coordination rank" not in text and "bond order" not in text, text  # the other instruments print nothing unasked
    res = load_sample_results_from_hdf5(out)
    c = res.voronoi
    assert set(c) == set(vo.STORED_KEYS) and c["cn"].shape == (30,) and c["neighbors"].shape == (30, 32, 4) and res.coordination is None
    ref = vo.voronoi_reference(res.frac_x, res.lattice, res.num_atoms, vo.VoronoiParams(tol=0.1, cutoff=5.5))
    for k in ("cn", "atom_flags", "neighbors"):
        assert np.array_equal(c[k][ref.guarded], getattr(ref, k)[ref.guarded]), k
    text2 = _child(["arreau_amd.screen", out, "--out", out2] + flags, 120)
    lines2 = [ln for ln in text2.splitlines() if ln.startswith("voronoi ")]
    assert lines2 == lines, (lines, lines2)
    back = load_sample_results_from_hdf5(out2)
    for k in vo.STORED_KEYS:
        assert np.array_equal(bits(back.voronoi[k]), bits(c[k])), k
    # a file of the known structures: the textbook numbers, printed and stored
    bt, r = cases.reference("known")
    num = np.array(bt.counts, dtype=np.int64)
    known, out3 = str(tmp_path / "known.npz"), str(tmp_path / "known_out.npz")
    save_sample_results_to_hdf5(SampleResult(frac_x=bt.frac.astype(np.float64), atomic_numbers=bt.species.astype(np.float64),
                                             lattice=bt.lattice.astype(np.float64), num_atoms=num, idx_start=np.cumsum(num) - num), known)
    text3 = _child(["arreau_amd.screen", known, "--voronoi", "--vor_cutoff", "5.3", "--out", out3], 120)
    assert "voronoi total: 8 crystals, 29 atoms; cn 4: 2, 6: 9, 8: 4, 10: 8, 12: 3, 14: 3; mean cn " in text3 and "open 0 / 29 atoms" in text3, text3
    stored = load_sample_results_from_hdf5(out3).voronoi
    assert np.array_equal(stored["cn"], r.cn) and np.array_equal(stored["neighbors"], r.neighbors) and np.array_equal(stored["species"], bt.species)


def test_argument_errors_touch_nothing(dev):
    bt = cases.single(cases.reference("known")[0], 1)
    frac, lattice, off = device_batch(dev, bt)
    with pytest.raises(ValueError, match="voronoi: offsets"):
        vo.voronoi(frac, lattice, off.to(torch.int64))
    out = vo.voronoi(frac, lattice, off, bt.params)
    before = {k: out[k].clone() for k in vo.RESULT_KEYS}
    r = _hip.VoronoiResultC(*[_hip.ptr(out[k]).value for k in vo.RESULT_KEYS])
    good = (0.05, 5.3, 32, 128, 8)
    call = _hip.lib().arreau_crystal_voronoi
    EINVAL = -1  # ARREAU_EINVAL
    B, N = 1, int(frac.shape[0])
    trials = [(B, N, None, ctypes.byref(r)), (B, N, good, None), (-1, N, good, ctypes.byref(r)), (B, -1, good, ctypes.byref(r)),
              (B, N, good, ctypes.byref(_hip.VoronoiResultC()))]
    trials += [(B, N, bad, ctypes.byref(r)) for bad in ((-0.1, 5.3, 32, 128, 8), (1.5, 5.3, 32, 128, 8), (float("nan"), 5.3, 32, 128, 8),
                                                       (0.05, 0.0, 32, 128, 8), (0.05, float("inf"), 32, 128, 8), (0.05, float("nan"), 32, 128, 8),
                                                       (0.05, 5.3, 0, 128, 8), (0.05, 5.3, 65, 128, 8), (0.05, 5.3, 32, 0, 8),
                                                       (0.05, 5.3, 32, 129, 8), (0.05, 5.3, 32, 128, 0), (0.05, 5.3, 32, 128, 9))]
    for b, n, p, res in trials:
        c = ctypes.byref(_hip.VoronoiParamsC(*p)) if p is not None else None
        assert call(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), b, n, c, res, _hip.stream_ptr(dev)) == EINVAL, (b, n, p)
        assert b"arreau_crystal_voronoi" in _hip.lib().arreau_last_error()
    c = ctypes.byref(_hip.VoronoiParamsC(*good))
    assert call(None, _hip.ptr(lattice), _hip.ptr(off), B, N, c, ctypes.byref(r), _hip.stream_ptr(dev)) == EINVAL
    one_null = _hip.VoronoiResultC(*[_hip.ptr(out[k]).value if k != "cn_eff" else None for k in vo.RESULT_KEYS])
    assert call(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), B, N, c, ctypes.byref(one_null), _hip.stream_ptr(dev)) == EINVAL
    skewed = _hip.VoronoiResultC(*[_hip.ptr(out[k]).value + (4 if k == "neighbors" else 0) for k in vo.RESULT_KEYS])  # unaligned neighbors
    assert call(_hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(off), B, N, c, ctypes.byref(skewed), _hip.stream_ptr(dev)) == EINVAL
    assert call(None, None, None, 0, 0, c, ctypes.byref(_hip.VoronoiResultC()), _hip.stream_ptr(dev)) == 0  # B == 0: OK
    torch.cuda.synchronize()
    for k in vo.RESULT_KEYS:
        assert torch.equal(before[k], out[k]) or (torch.isnan(before[k]) == torch.isnan(out[k])).all() and torch.equal(torch.nan_to_num(before[k]), torch.nan_to_num(out[k])), k


def test_sample_takes_the_keyword_and_the_symbol_is_exported(fused_model):
    """What fails without the feature: sample(voronoi=...) is a TypeError and the entry point is not in the library."""
    import inspect
    m, _ = fused_model
    assert "voronoi" in inspect.signature(m.sample).parameters
    assert "arreau_crystal_voronoi" in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.LIB_PATH), "arreau_crystal_voronoi")
    with open(os.path.join(ROOT, "include", "arreau_hip.h")) as fh:
        assert "int arreau_crystal_voronoi(" in fh.read()
