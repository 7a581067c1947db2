"""The float32 restatement of the neighbour list (tests/neighbor_reference.py) checked on the CPU, before the GPU tests lean on
it: it equals the oracle on the tie-free random inputs and the reference's fixtures, it equals the oracle's stable-sort variant
on every input small enough for the oracle, every shared input reaches the kernel paths it declares (with an exact tie at the
cut on each of the five paths), and a selection that broke ties the other way round would be noticed."""
import os

import numpy as np
import pytest
import torch

from oracle import geometry as OG
from tests import neighbor_reference as NR
from tests.helpers import random_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the oracle builds a dense [pairs, 3, 27] tensor per batch: compared on cases whose largest crystal has at most this many atoms
ORACLE_ATOM_CAP = 256
CASES = NR.cases()
SELECTED, DIAGNOSED = {}, {}


def selected(case):
    if case.name not in SELECTED:
        SELECTED[case.name] = NR.select(case.cart, case.lattice, case.counts, case.radius, case.k)
    return SELECTED[case.name]


def diagnosed(case):
    if case.name not in DIAGNOSED:
        DIAGNOSED[case.name] = NR.diagnose(case.cart, case.lattice, case.counts, case.radius, case.k)
    return DIAGNOSED[case.name]


def assert_equals_oracle(sel, oracle_out, what):
    o_ei, o_cells, _cnt, o_dist, o_dir = oracle_out
    ei, cells, dist, direction = NR.to_edges(sel)
    assert np.array_equal(ei, o_ei.numpy()), what
    assert np.array_equal(cells, o_cells.numpy()), what
    # the oracle's offsets come from a matrix product and its d2 from a library reduction: same edges, values to rounding
    np.testing.assert_allclose(dist, o_dist.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(direction, o_dir.numpy(), atol=1e-6, rtol=0)


@pytest.mark.parametrize("num_atoms,cell,seed", [
    ([20] * 16, (4.0, 8.0), 0), ([1, 2, 3, 5, 8, 13, 20, 7], (3.0, 6.0), 1), ([64, 64], (6.0, 9.0), 2), ([2] * 5, (9.0, 12.0), 3),
    ([33], (2.5, 4.0), 4), ([48, 64, 29, 57], (7.0, 11.0), 5), ([64], (2.0, 3.0), 6), ([40, 40], (3.5, 5.0), 7),
    ([150, 3, 128, 129], (8.0, 12.0), 8)])
def test_select_equals_the_oracle_on_tie_free_random_input(num_atoms, cell, seed):
    """The inputs of test_gpu_parity.py::test_radius_graph_vs_oracle_random (positions formed on the CPU here): no receiver
    has a tie at the cut, and the restatement selects the oracle's edges through the oracle's image cells."""
    frac, _, lengths, angles, na = random_state(12, num_atoms, seed, cell=cell)
    lattice = OG.lattice_from_params(lengths, angles)
    cart = OG.frac_to_cart_coords(frac, lattice, na)
    sel = NR.select(cart.numpy(), lattice.numpy(), num_atoms, 5.0, 8)
    about = NR.diagnose(cart.numpy(), lattice.numpy(), num_atoms, 5.0, 8)
    assert not about.tied.any()
    assert_equals_oracle(sel, OG.radius_graph_pbc(cart, lattice, na, 5.0, 8), (num_atoms, seed))
    p = NR.paths_of(about)
    assert not p["fallback"].any()  # (none of these reaches the re-evaluating rounds)


def _golden_cases():
    z = np.load(os.path.join(GOLDEN, "radius_graph.npz"))
    return [i for i in range(int(z["n_cases"])) if str(z[f"c{i}_dtype"]) == "f32"]


@pytest.mark.parametrize("i", _golden_cases())
def test_select_equals_the_reference_fixtures(i):
    z = np.load(os.path.join(GOLDEN, "radius_graph.npz"))
    p = f"c{i}_"
    sel = NR.select(z[p + "cart"], z[p + "lattice"], z[p + "num_atoms"].tolist(), float(z[p + "radius"]), int(z[p + "k"]))
    ei, cells, dist, direction = NR.to_edges(sel)
    assert ei.shape[1] == int(z[p + "count"].sum())
    if str(z[p + "flag"]).startswith("ties"):  # the reference's unstable sort chose among tied images: count and distances
        np.testing.assert_allclose(np.sort(dist), np.sort(z[p + "dist"]), atol=1e-6, rtol=0)
        return
    assert np.array_equal(ei, z[p + "edge_index"]) and np.array_equal(cells, z[p + "cells"])
    np.testing.assert_allclose(dist, z[p + "dist"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(direction, z[p + "dir"], atol=1e-6, rtol=0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_reaches_the_paths_it_declares(case):
    """By atom counts and by the emulated threshold (passing_keys).  For the `fallback` cases this is a condition on the
    INPUT: were it not met, the case would be wrong."""
    sel, deg = diagnosed(case), selected(case).deg
    reached = NR.paths_of(sel)
    tie_on = [name for name in NR.PATHS if (reached[name] & sel.tied).any()]
    print(f"\n[paths] {case.name}: atoms {case.counts if len(case.counts) < 9 else len(case.counts)}, k {case.k}, radius {case.radius}: "
          + ", ".join(f"{n} {int(reached[n].sum())}" for n in NR.PATHS if reached[n].any())
          + f"; receivers tied at the cut {int(sel.tied.sum())} of {len(sel.tied)} (on: {', '.join(tie_on) or 'none'})"
          + f"; near-tied (gap < 1e-5, not tied) {int(((sel.gap < 1e-5) & ~sel.tied).sum())}; most keys passed {int(sel.passed.max())}")
    for name in case.paths:
        assert reached[name].any(), (case.name, name)
    if case.tie is not None:
        assert bool(sel.tied.any()) == case.tie, case.name
    if hasattr(case, "degrees"):
        assert deg.tolist() == case.degrees
    if hasattr(case, "cluster"):
        fb = reached["fallback"]
        inside = np.zeros(len(fb), bool)
        inside[case.cluster] = True
        assert not (fb & ~inside).any()  # (the other atoms: the LDS list)
        if case.finite_threshold:
            finite = fb & (sel.lanes >= case.k)  # T is a key, and still more than 384 keys pass
            print(f"[paths] {case.name}: fallback with a finite threshold {int(finite.sum())}, without {int((fb & ~finite).sum())}")
            assert int(finite.sum()) >= 64
        else:
            assert fb[case.cluster].all() and (sel.lanes[case.cluster] < case.k).all()  # T = KEY_NONE
            assert (sel.tied & fb).any()
        assert sel.atoms[0] > 1024  # more receivers than one chunk of the edge-offset scan


def test_a_tie_at_the_cut_on_each_of_the_five_paths():
    seen = set()
    for case in CASES:
        sel = diagnosed(case)
        seen |= {name for name, mask in NR.paths_of(sel).items() if (mask & sel.tied).any()}
    assert seen == set(NR.PATHS), seen


def test_the_self_edge_threshold_is_met_from_both_sides():
    case = next(c for c in CASES if c.name == "self_edge_threshold")
    sel = selected(case)
    assert sel.deg.tolist() == [0, 0, 1, 1]  # d2 = 9.8e-5 is a self edge, d2 = 1.02e-4 a neighbour
    assert 0 < float(sel.dist[2, 0]) ** 2 - 1e-4 < 3e-6


@pytest.mark.parametrize("case", [c for c in CASES if max(c.counts) <= ORACLE_ATOM_CAP], ids=lambda c: c.name)
def test_the_stable_oracle_equals_select(case):
    cart, lattice, na = torch.from_numpy(case.cart), torch.from_numpy(case.lattice), torch.tensor(case.counts)
    for k in sorted({case.k, 1, 13, 64}):
        sel = selected(case) if k == case.k else NR.select(case.cart, case.lattice, case.counts, case.radius, k)
        assert_equals_oracle(sel, OG.radius_graph_pbc(cart, lattice, na, case.radius, k, stable_ties=True), (case.name, k))


def test_the_oracle_cap_leaves_out_the_fallback_cases_only():
    assert sorted(c.name for c in CASES if max(c.counts) > ORACLE_ATOM_CAP) == ["fallback_finite_threshold", "fallback_no_threshold"]


@pytest.mark.parametrize("name", ["rock_salt", "sc3", "sc4", "sc6", "coincident"])
def test_a_flipped_tie_order_changes_the_selection(name):
    """A kernel that broke ties by descending c would select other edges for exactly the receivers tied at the cut."""
    case = next(c for c in CASES if c.name == name)
    sel, about = selected(case), diagnosed(case)
    flipped = NR.select(case.cart, case.lattice, case.counts, case.radius, case.k, descending_ties=True)
    changed = (sel.src != flipped.src).any(axis=1) | (sel.cell != flipped.cell).any(axis=1)
    assert about.tied.any() and np.array_equal(changed, about.tied)
