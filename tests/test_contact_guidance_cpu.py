"""Contact guidance without a GPU (rules in include/arreau_hip.h, "contact guidance"; arreau_amd/diffusion/contact_guidance.py): the
float64 restatement against finite differences of its own penalty, its invariances, the step identity, the cases' own
preconditions, validation, the header / binding / build list, and the keyword's way into sample()."""
import inspect
import os
import re

import numpy as np
import pytest

from arreau_amd.diffusion import contact_guidance as cg
from tests import contact_guidance_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases.all_cases()
IDS = [c.name for c in CASES]
LAUNCH_CASES = cases.launch_cases()  # one restatement each: too large for the finite-difference and invariance tests below


def _ref(case, frac=None, lattice=None):
    """The restatement on the case's values in float64 (exactly the float32 inputs, or the float64 arrays given)."""
    f = np.asarray(case.frac if frac is None else frac, dtype=np.float64)
    L = np.asarray(case.lattice if lattice is None else lattice, dtype=np.float64)
    return cg.reference(f, L, case.offsets, case.params)


# ----------------------------------------------------------------------------------------------------- the cases themselves
@pytest.mark.parametrize("case", CASES + LAUNCH_CASES, ids=IDS + [c.name for c in LAUNCH_CASES])
def test_cases_hold_their_own_preconditions(case):
    """Every contact at d >= 0.05 A, every pair and image at least 1e-3 A from d0 (the coincident pair of `overlap` is skipped by
    the rule and so by the margin), flags and contacts as the case states them."""
    r = _ref(case)
    assert list(r.flags) == list(case.flags)
    if case.contacts is not None:
        assert list(r.contacts) == list(case.contacts)
    for b in range(case.B):
        print(case.name, b, "contacts", r.contacts[b], "U", r.U[b], "d_min", r.d_min[b], "margin", r.margin[b].min() if r.margin[b].size else None)
        assert r.ordered[b] == 2 * r.contacts[b]  # every contact is seen from both ends
        assert r.d[b].size == 0 or r.d[b].min() >= cases.MIN_D
        assert r.margin[b].size == 0 or r.margin[b].min() >= cases.MIN_MARGIN
        if r.flags[b] & cg.SKIPPED:
            assert r.U[b] == 0 and r.contacts[b] == 0
    # the float32 inputs and their float32 wrap are what the kernel reads: the restatement on them sees the same crystals
    r32 = cg.reference(case.frac, case.lattice, case.offsets, case.params)
    assert list(r32.flags) == list(r.flags) and list(r32.contacts) == list(r.contacts)


def test_cases_cover_what_they_are_for():
    by = {c.name: _ref(c) for c in CASES}
    tri = cases.triclinic_case()
    assert max(by["triclinic"].shells[0]) == 2  # two shells along the 2 A axis
    # several images of one j in contact with one i
    from arreau_amd.diffusion import crystal_batch as cb
    L = tri.lattice[0].astype(np.float64)
    p = tri.frac.astype(np.float64) @ L
    s = cb.shift_table(by["triclinic"].shells[0])[0] @ L
    assert (np.linalg.norm(p[1] + s - p[0], axis=1) < 2.5).sum() >= 2
    assert by["single"].shells[0].min() >= 2 and by["single"].contacts[0] == 0  # its own images lie inside d0 and are left out
    assert by["flat"].flags[0] == cg.CELL and cases.flat_case().params.max_shells == 1
    assert cases.ragged_case().counts == [1, 2, 7, 20, 65] and list(cases.ragged_case().t) == [1, 2, cases.T // 2, cases.T - 1, cases.T]
    assert by["ragged"].contacts[4] > 10 and by["ragged"].contacts[1] == 1
    mixed = cases.mixed_batch()
    assert list(_ref(mixed).flags) == [0, cg.NONFINITE, 0, cg.EMPTY, cg.OVERLAP, 0]


def test_launch_cases_cover_what_they_are_for():
    """`large`: 257 atoms (one past the staged path) between two small crystals, at least 300 contacts, the last atom without one
    and farther than d0 from every atom and image, every margin decided; the 256-atom crystal is its first 256 atoms in the same
    cell with the same shells, so the same image count.  `eight shells`: [1, 1, 8] accepted next to a CELL twin.  `seventy`: 70
    crystals, the counts of `ragged` cycling, timesteps from 1 to T.  The forces of every unflagged crystal sum to zero."""
    from arreau_amd.diffusion import crystal_batch as cb
    by = {c.name: (c, _ref(c)) for c in LAUNCH_CASES}
    big, r = by["large"]
    a, e = big.offsets[1], big.offsets[2]
    assert big.counts == [3, cases.LARGE_N, 3] and cases.LARGE_N == 257 and list(r.flags) == [0, 0, 0]
    assert r.contacts[0] > 0 and r.contacts[2] == r.contacts[0]  # the neighbours in the batch are guided too
    assert r.contacts[1] >= 300 and r.atom_contacts[e - 1] == 0 and r.margin[1].min() >= 1e-3
    L = big.lattice[1].astype(np.float64)
    p = cg._wrap(big.frac[a:e]).astype(np.float64) @ L
    s = cb.shift_table(r.shells[1])[0] @ L
    d0 = float(np.float32(big.params.min_distance))
    assert np.linalg.norm(p[:-1, None, :] + s[None] - p[-1], axis=-1).min() > d0
    assert np.linalg.norm(s[np.abs(s).sum(1) > 0], axis=1).min() > d0  # its own images too
    less = cases.large_case(n=256)
    r256 = _ref(less)
    assert np.array_equal(less.frac, big.frac[a:e - 1]) and np.array_equal(less.lattice[0], big.lattice[1])
    assert list(r256.shells[0]) == list(r.shells[1]) and r256.contacts[0] == r.contacts[1]
    assert np.array_equal(r256.atom_contacts, r.atom_contacts[a:e - 1])  # the same contacts; the float64 sums in numpy's order
    assert abs(r256.U[0] - r.U[1]) <= 1e-12 * r.U[1] and np.abs(r256.g - r.g[a:e - 1]).max() <= 1e-12 * np.abs(r256.g).max()
    eight, r8 = by["eight shells"]
    assert list(r8.shells[0]) == [1, 1, 8] and list(r8.flags) == [0, cg.CELL] and r8.contacts[0] > 0 and eight.params.max_shells == 8
    assert r8.margin[0].min() >= 1e-3 and np.array_equal(eight.frac[:3], eight.frac[3:])
    sev, r70 = by["seventy"]
    assert sev.B == 70 and sev.counts == [1, 2, 7, 20, 65] * 14 and not r70.flags.any()
    assert sev.t[0] == 1 and sev.t[-1] == cases.T and (np.diff(sev.t) >= 1).all() and len(set(sev.t.tolist())) == 70
    assert (r70.contacts[4::5] > 10).all()
    assert list(np.clip(cases.BAD_T, 1, cases.T)) == [1, 1, cases.T, 5, cases.T] and len(cases.BAD_T) == cases.ragged_case().B
    for case, ref in list(by.values()) + [(cases.ragged_case(), _ref(cases.ragged_case()))]:
        for b in range(case.B):
            if not ref.flags[b] & cg.SKIPPED:
                x, y = case.offsets[b], case.offsets[b + 1]
                # sum_i g_i L = sum_i D_i = 0: every contact is seen from both ends with opposite displacements
                assert np.abs((ref.g[x:y] @ case.lattice[b].astype(np.float64)).sum(0)).max() <= 1e-12, (case.name, b)


# ----------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_is_the_finite_difference_of_the_penalty(case):
    """D_i = dU / dr_i by central differences with a Cartesian step of 1e-6 A, to 1e-6 of the crystal's largest |D|.  Coincident
    atoms (`overlap`) are moved together: the rule skips their pair at d == 0, so U is defined on the set where they coincide, and
    its derivative along that set is the sum of their D."""
    h = 1e-6
    for b in range(case.B):
        one = case.crystal(b)  # (a crystal's U depends on its own atoms alone)
        r = _ref(one)
        if r.flags[0] & cg.SKIPPED:
            assert not r.D.any() and not r.g.any()
            continue
        frac = one.frac.astype(np.float64)
        Linv = np.linalg.inv(one.lattice[0].astype(np.float64))
        groups = [[0, 1], [2]] if case.name == "overlap" else [[i] for i in range(one.counts[0])]
        scale = np.abs(r.D).max()
        for grp in groups:
            for d in range(3):
                step = np.zeros(3)
                step[d] = h
                up, dn = frac.copy(), frac.copy()
                up[grp] += step @ Linv
                dn[grp] -= step @ Linv
                fd = (_ref(one, up).U[0] - _ref(one, dn).U[0]) / (2 * h)
                assert abs(fd - r.D[grp, d].sum()) <= 1e-6 * scale, (case.name, b, grp, d, fd, r.D[grp, d].sum())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fractional_gradient_times_the_cell_is_the_cartesian_one(case):
    r = _ref(case)
    for b in range(case.B):
        a, e = case.offsets[b], case.offsets[b + 1]
        if not r.flags[b] & cg.SKIPPED:
            np.testing.assert_allclose(r.g[a:e] @ case.lattice[b].astype(np.float64), r.D[a:e], rtol=0, atol=1e-12 * max(1.0, np.abs(r.D[a:e]).max()))
        if e > a:
            assert abs(r.D[a:e].sum(0)).max() <= 1e-12 * max(1.0, np.abs(r.D[a:e]).max())  # the forces of a pair cancel


def test_isolated_pair_ends_at_min_distance():
    """d = 0.3 A, d0 = 0.5, w = 0.5: the fractional move -w g puts the pair at d0 exactly (each atom moves w (d0 - d))."""
    case = cases.pair_case()
    r = _ref(case)
    assert abs(r.d[0][0] - 0.3) < 1e-6
    moved = case.frac.astype(np.float64) - case.params.weight * r.g
    L = case.lattice[0].astype(np.float64)
    assert abs(np.linalg.norm((moved[1] - moved[0]) @ L) - float(np.float32(case.params.min_distance))) <= 1e-12
    after = _ref(case, moved)
    assert after.U[0] <= 1e-24 and after.contacts[0] in (0, 1)  # at the threshold: nothing left to push


# ----------------------------------------------------------------------------------------------------- invariances
def _guided(case):
    return [b for b in range(case.B) if not case.flags[b] & cg.SKIPPED]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_invariant_under_an_atom_permutation(case):
    r = _ref(case)
    rng = np.random.RandomState(3)
    perm = np.concatenate([case.offsets[b] + rng.permutation(case.counts[b]) for b in range(case.B)] + [np.zeros(0, np.int64)]).astype(np.int64)
    q = _ref(case, case.frac.astype(np.float64)[perm])
    assert list(q.flags) == list(r.flags) and list(q.contacts) == list(r.contacts)
    np.testing.assert_allclose(q.U, r.U, rtol=0, atol=1e-12)
    np.testing.assert_allclose(q.D, r.D[perm], rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_invariant_under_lattice_translations_of_single_atoms(case):
    r = _ref(case)
    rng = np.random.RandomState(4)
    shift = rng.randint(-3, 4, case.frac.shape).astype(np.float64)
    if case.name == "overlap":
        shift[1] = shift[0]  # (coincident atoms stay bitwise coincident: the rule's d == 0 is an exact comparison)
    q = _ref(case, case.frac.astype(np.float64) + shift)
    assert list(q.flags) == list(r.flags) and list(q.contacts) == list(r.contacts)
    np.testing.assert_allclose(q.U, r.U, rtol=0, atol=1e-12)
    np.testing.assert_allclose(q.D, r.D, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_invariant_under_a_unimodular_change_of_basis(case):
    """L' = M L, f' = f M^-1 with an integer M of determinant 1: the same crystal, so the same U, D and contacts (g changes with
    the basis: g' L' = D still holds)."""
    M = np.array([[1, 1, 0], [0, 1, 0], [-1, 0, 1]], dtype=np.float64)
    assert round(np.linalg.det(M)) == 1
    r = _ref(case)
    L2 = np.einsum("ij,bjk->bik", M, case.lattice.astype(np.float64))
    f2 = case.frac.astype(np.float64) @ np.linalg.inv(M)
    if case.name == "flat":  # (CELL either way: the sheared flat cell needs no fewer images)
        assert list(cg.reference(f2, L2, case.offsets, case.params).flags) == [cg.CELL]
        return
    q = cg.reference(f2, L2, case.offsets, case.params)
    assert list(q.flags) == list(r.flags) and list(q.contacts) == list(r.contacts)
    np.testing.assert_allclose(q.U, r.U, rtol=0, atol=1e-12)
    np.testing.assert_allclose(q.D, r.D, rtol=0, atol=1e-12)
    for b in _guided(case):
        a, e = case.offsets[b], case.offsets[b + 1]
        np.testing.assert_allclose(q.g[a:e] @ L2[b], r.D[a:e], rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------------------------------- guided eps and bounds
def test_guided_eps_and_the_bounds():
    case = cases.ragged_case()
    r = _ref(case)
    sig = np.linspace(0.0, 1.0, cases.T + 1) ** 2 + 0.01
    eps = np.random.RandomState(1).normal(size=case.frac.shape)
    k = cg.sigma_coefficient(sig, case.t, case.params.weight)
    assert np.allclose(k, 0.5 / sig[case.t] ** 2) and np.allclose(cg.sigma_coefficient(sig, [0, cases.T + 5], 1.0), 1 / sig[[1, cases.T]] ** 2)
    out = cg.guided_eps(eps, r, case.offsets, sig, case.t, case.params)
    np.testing.assert_allclose(out, eps + np.repeat(k, case.counts)[:, None] * r.g)
    # the bound: zero without contacts, grows with the contact count and as d_min falls, far below the gradient itself
    L, shells = case.lattice[4], r.shells[4]
    most = int(r.atom_contacts[case.offsets[4]:].max())
    assert r.atom_contacts[case.offsets[4]:].sum() == r.ordered[4] and most >= 3
    gb = cg.g_bound(0.9, r.d_min[4], L, shells, most)
    assert cg.g_bound(0.9, np.inf, L, shells, 0) == 0.0
    assert 0 < cg.g_bound(0.9, r.d_min[4], L, shells, 1) < gb < cg.g_bound(0.9, r.d_min[4] / 10, L, shells, most)
    print("g bound", gb, "largest |g|", np.abs(r.g[case.offsets[4]:]).max())
    assert gb < 1e-2 * np.abs(r.g[case.offsets[4]:]).max()
    assert 0 < cg.energy_bound(0.9, L, shells, r.ordered[4], r.U[4]) < 1e-3 * r.U[4]


# ----------------------------------------------------------------------------------------------------- validation
def test_parameters_and_validation():
    p = cg.ContactGuidance()
    assert (p.min_distance, p.weight, p.max_shells) == (0.5, 0.5, 8) and isinstance(cg.ContactGuidance(min_distance=1, weight=0).weight, float)
    for bad in (dict(min_distance=0), dict(min_distance=-1), dict(min_distance=float("nan")), dict(min_distance=float("inf")), dict(weight=-0.1),
                dict(weight=float("inf")), dict(weight=1e40), dict(weight="1"), dict(min_distance=True), dict(max_shells=0), dict(max_shells=9),
                dict(max_shells=2.0), dict(max_shells=True), dict(min_distance=1e-60)):
        with pytest.raises(ValueError):
            cg.ContactGuidance(**bad)
    assert cg.resolve(None) is None and cg.resolve(False) is None and cg.resolve(True) == p and cg.resolve(p) is p
    with pytest.raises(ValueError):
        cg.resolve(0.5)
    cg.check_sampling(None, inversion=True), cg.check_sampling(p)
    with pytest.raises(ValueError, match="inversion"):
        cg.check_sampling(p, inversion=True)
    assert cg.describe(cg.CELL | cg.EMPTY) == "CELL|EMPTY" and cg.describe(0) == "ok"
    with pytest.raises(Exception):
        p.weight = 1.0  # frozen


def test_header_binding_and_build_agree():
    import ctypes

    from arreau_amd import _hip, build
    header = open(os.path.join(ROOT, "include", "arreau_hip.h")).read()
    assert {"arreau_sample_loop_guided", "arreau_contact_guidance_step"} <= set(_hip.EXPORTS) and "contact_guide.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "contact_guide.hip"))
    for bit, name in cg.FLAG_NAMES:
        assert re.search(rf"#define ARREAU_GUIDE_{name} {bit}\b", header), name
    body = re.search(r"typedef struct arreau_contact_guidance \{(.*?)\} arreau_contact_guidance;", header, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body)) == [n for n, _ in _hip.ContactGuidanceC._fields_]
    assert ctypes.sizeof(_hip.ContactGuidanceC) == 40
    protos = _hip._prototypes()
    for name, n in (("arreau_sample_loop_guided", 29), ("arreau_contact_guidance_step", 10)):
        proto = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto).split(",")) == len(protos[name]) == n
    assert protos["arreau_sample_loop_guided"][:-2] == protos["arreau_sample_loop_keyed"][:-1]  # the keyed loop plus the struct
    assert "contact guidance" in header and "What this is not" in header


def test_signatures_and_parser_flags():
    from arreau_amd import generate
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    from arreau_amd.engine import HipEngine
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    for fn in (DiffusionLoss.sample, PONITA_DIFFUSION.sample, PONITA_DIFFUSION.encode):
        assert inspect.signature(fn).parameters["contact_guidance"].default is None
    assert inspect.signature(HipEngine.sample_loop).parameters["guidance"].default is None
    assert list(inspect.signature(HipEngine.contact_guidance_step).parameters)[1:] == ["frac", "lattice", "t_crystal", "offsets", "eps", "guidance"]
    ap = generate.build_parser()
    args = ap.parse_args(["--model_path", "m.ckpt"])
    assert args.guide_contacts is False and generate.check_guidance_arguments(args, None) is None
    args = ap.parse_args(["--model_path", "m.ckpt", "--guide_contacts", "--guide_min_distance", "0.7", "--guide_weight", "0.25"])
    assert generate.check_guidance_arguments(args, None) == cg.ContactGuidance(min_distance=0.7, weight=0.25)
    errors = []
    args = ap.parse_args(["--model_path", "m.ckpt", "--guide_contacts", "--guide_weight", "-1"])
    assert generate.check_guidance_arguments(args, errors.append) is None and errors and errors[0].startswith("--guide_contacts: ")


def test_statistics_lines():
    info = {"energy": np.array([0.5, 0.0, 0.25], np.float32), "contacts": np.array([3, 0, 1], np.int32), "flags": np.array([0, cg.CELL, cg.OVERLAP], np.int32)}
    a, b = cg.stats_of(info, 0), cg.stats_of(info, 1)
    assert a["contacts"] == 4 and a["with_contacts"] == 2 and a["flags"] == {"NONFINITE": 0, "CELL": 1, "EMPTY": 0, "OVERLAP": 1}
    assert cg.total_stats([a, a], 0)["crystals"] == 6 and cg.total_stats([a, a], 0)["rank"] == 0
    lines = cg.summary_lines([b, a])
    assert len(lines) == 3 and lines[0].startswith("contact guidance, rank 0: 3 crystals") and "8 contacts" in lines[2] and "CELL 2" in lines[2]


def test_the_keyword_reaches_sample():
    """A bad value is rejected by sample() itself, before any work: no GPU is touched.  (Before the option existed this raised a
    TypeError for the unknown keyword.)"""
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=12, seed=1, num_timesteps=30)
    with pytest.raises(ValueError, match="contact_guidance must be"):
        m.sample(4, 2, contact_guidance=0.5)
    with pytest.raises(ValueError, match="contact_guidance must be"):
        m.diffusion_loss.sample(model=m, z_table=None, num_atoms_per_sample=4, num_samples_in_batch=2, contact_guidance="on")
    crystals = type("C", (), dict(num_atoms=np.array([2]), frac_x=np.zeros((2, 3)), lattice=np.eye(3)[None] * 4, atomic_numbers=np.array([1, 1])))
    with pytest.raises(ValueError, match="inversion"):
        m.encode(crystals, contact_guidance=True)
