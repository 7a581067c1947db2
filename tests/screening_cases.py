"""The inputs the screen's CPU and GPU tests share (test_screening_cpu.py, test_gpu_screening.py): a seeded random set of
triclinic crystals in ragged batches and the hand-made cases, the same bytes for both.  numpy only.

The random set is drawn so that a float32 and a float64 evaluation MUST agree on every integer output: no crystal has its
shortest distance within the derived bound (screening.distance_bound) of search_radius, no contact within twice the bound of
min_distance, no two smallest contacts within twice the bound of each other, no volume within 1e-5 (relative) of min_volume
and no shell quotient q_k = search_radius / h_k within 1e-5 (relative) of an integer or of max_shells.  A crystal that breaks
one of these is drawn again (decided with the float64 restatement alone); `random_set` reports how many were."""
from types import SimpleNamespace

import numpy as np

from arreau_amd.diffusion import screening as sc
from tests.neighbor_reference import cell_from_params

F32 = np.float32
DEG = np.pi / 180
BATCH_SIZES = (1, 7, 16, 24)  # ragged batches: 48 crystals
MASK_TYPE = 5                 # of the random species 0..5


def _draw(rng):
    n = int(rng.randint(1, 65))
    L = cell_from_params(rng.uniform(3.0, 10.0, size=3), rng.uniform(60.0, 120.0, size=3) * DEG)
    return rng.uniform(0.0, 1.0, (n, 3)).astype(F32), L, rng.randint(0, MASK_TYPE + (1 if rng.rand() < 0.15 else 0), n).astype(np.int32)


def offends(frac, L, criteria):
    """True when float32 and float64 need not agree on this crystal's integer outputs (module docstring)."""
    r = sc.screen_reference_f64(frac, [L], [len(frac)], criteria=criteria, details=True)
    if abs(r.volume[0] - criteria.min_volume) <= 1e-5 * criteria.min_volume:
        return True
    q = r.q[0]
    if np.isfinite(q).all():
        marks = np.concatenate([np.arange(1, criteria.max_shells + 1), [criteria.max_shells]])
        if (np.abs(q[:, None] - marks[None, :]) <= 1e-5 * marks[None, :]).any():
            return True
    if r.flags[0] & (sc.CELL | sc.NONFINITE):
        return False
    near, bound = r.nearest[0], r.bound[0]
    if r.near_threshold[0] > 0 or (near.size and abs(near[0] - criteria.search_radius) <= bound):
        return True
    return bool(near.size > 1 and near[1] - near[0] <= 2 * bound)


def random_set(seed=2024, criteria=None, batch_sizes=BATCH_SIZES):
    """(batches, replaced, total): each batch a namespace frac [N,3] float32, lattice [B,3,3] float32, counts [B], types [N]
    int32 (species 0..4, in some crystals also the mask state 5)."""
    criteria = criteria if criteria is not None else sc.ScreenCriteria(mask_type=MASK_TYPE)
    rng = np.random.RandomState(seed)
    batches, replaced, total = [], 0, 0
    for B in batch_sizes:
        crystals = []
        for _ in range(B):
            c = _draw(rng)
            total += 1
            while offends(c[0], c[1], criteria):
                replaced += 1
                c = _draw(rng)
            crystals.append(c)
        batches.append(_batch(f"random_{B}", crystals))
    return batches, replaced, total


def _batch(name, crystals, **extra):
    return SimpleNamespace(name=name, frac=np.concatenate([np.asarray(c[0], dtype=F32).reshape(-1, 3) for c in crystals]),
                           lattice=np.stack([np.asarray(c[1], dtype=F32) for c in crystals]), counts=[len(c[0]) for c in crystals],
                           types=np.concatenate([np.asarray(c[2], dtype=np.int32).reshape(-1) for c in crystals]), **extra)


def cube(a):
    return np.eye(3, dtype=F32) * F32(a)


SKEWED_CELL = np.array([[4, 0, 0], [7.5, 1, 0], [0, 0, 6]], dtype=F32)


def hand_cases():
    """Named single-crystal (or small) batches with what the screen must say about them: expect = dict of flags [B],
    and per case optional pair / min_distance / n_close (exact values, or None where the case does not pin them)."""
    zeros = lambda n: np.zeros(n, np.int32)
    out = []

    def add(name, crystals, **expect):
        out.append(_batch(name, crystals, expect=expect))
    # two atoms 0.3 A apart across the face x = 0 of a 5 A cube: 0.97 and 0.03
    add("across_face", [([[0.97, 0.5, 0.5], [0.03, 0.5, 0.5]], cube(5.0), zeros(2))], flags=[sc.CLOSE], pair=[(0, 1, 1, 0, 0)],
        n_close=[1], approx_distance=[0.3])
    # two atoms on one site: distance exactly 0, reported (the neighbour list would skip the pair)
    add("coincident", [([[0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [0.6, 0.1, 0.3]], cube(6.0), zeros(3))], flags=[sc.CLOSE],
        pair=[(0, 1, 0, 0, 0)], n_close=[1], min_distance=[0.0])
    # one atom in a skewed cell: its nearest image is two cells along a, one back along b -- 2 a - b = (0.5, -1, 0), sqrt(1.25) A --
    # outside the 27 images, whose nearest is a - b at about 3.64 A.  Of the pair of opposite shifts +-(2, -1, 0) the rule counts
    # the one after (0, 0, 0) in lexicographic order.
    add("skewed_self_image", [([[0.3, 0.2, 0.1]], SKEWED_CELL, zeros(1))], flags=[0], pair=[(0, 0, 2, -1, 0)], n_close=[0],
        approx_distance=[np.sqrt(1.25)])
    # a collapsed cell: volume 0.05 A^3 below min_volume
    add("collapsed", [([[0.1, 0.2, 0.3], [0.6, 0.7, 0.8]], np.diag([5.0, 5.0, 0.002]).astype(F32), zeros(2))], flags=[sc.CELL],
        pair=[(-1,) * 5], n_close=[0], nan_distance=True)
    # a flat cell of ordinary volume that would need more than 8 images along c
    add("too_many_shells", [([[0.1, 0.2, 0.3]], np.diag([30.0, 30.0, 0.3]).astype(F32), zeros(1))], flags=[sc.CELL], pair=[(-1,) * 5],
        n_close=[0], nan_distance=True)
    add("nan_coordinate", [([[0.1, np.nan, 0.3], [0.5, 0.5, 0.5]], cube(5.0), [MASK_TYPE, 0])], flags=[sc.NONFINITE], pair=[(-1,) * 5],
        n_close=[0], nan_distance=True, nan_volume=True)
    add("inf_cell", [([[0.1, 0.2, 0.3]], np.array([[5, 0, 0], [0, np.inf, 0], [0, 0, 5]], dtype=F32), zeros(1))], flags=[sc.NONFINITE],
        pair=[(-1,) * 5], n_close=[0], nan_distance=True, nan_volume=True)
    add("masked", [([[0.1, 0.1, 0.1], [0.4, 0.4, 0.4]], cube(4.0), [2, MASK_TYPE])], flags=[sc.MASKED], pair=[(0, 1, 0, 0, 0)], n_close=[0],
        approx_distance=[1.2 * np.sqrt(3.0)])
    # one atom in a 12 A cube: nothing within 3 A; the nearest image is one cell along c (the first of the three equal ones)
    add("sparse", [([[0.5, 0.5, 0.5]], cube(12.0), zeros(1))], flags=[sc.BEYOND], pair=[(0, 0, 0, 0, 1)], n_close=[0], min_distance=[12.0])
    # an exact tie: four atoms on a line, 1 A apart in a 4 A cube (every coordinate exact in float32).  Contacts at exactly
    # 1 A: (0,1), (1,2), (2,3) in the cell and (0,3) through the face.  Smallest i, then smallest j: (0, 1, shift 0).
    add("exact_tie", [([[0, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.75, 0.5, 0.5]], cube(4.0), zeros(4))], flags=[0],
        pair=[(0, 1, 0, 0, 0)], n_close=[0], min_distance=[1.0])
    # ... and a tie in the shift alone: one atom in a 2 A cube meets its images at (0,0,1), (0,1,0), (1,0,0): the earliest shift
    add("tie_in_shift", [([[0.5, 0.5, 0.5]], cube(2.0), zeros(1))], flags=[0], pair=[(0, 0, 0, 0, 1)], n_close=[0], min_distance=[2.0])
    # coordinates far outside [0, 1) and negative: the same crystal as its wrapped copy (0.25 steps are exact).  The third crystal
    # has a coordinate of -1e-9, whose float32 wrap 1 - 1e-9 rounds to exactly 1.0 and so becomes 0; in float64 it stays just below
    # 1 and the same contact is found through the face (shift (1, 0, 0)) -- which is why hand cases are compared with the float64
    # restatement in distance only
    wrapped = [[0.25, 0.5, 0.75], [0.5, 0.5, 0.75], [0.0, 0.25, 0.0]]
    moved = [[-3.75, 17.5, -0.25], [100.5, -7.5, 2.75], [-2.0, -1023.75, 64.0]]
    add("wrap", [(moved, cube(4.0), zeros(3)), (wrapped, cube(4.0), zeros(3)), ([[-1e-9, 0.5, 0.5], [0.25, 0.5, 0.5]], cube(4.0), zeros(2))],
        flags=[0, 0, 0], pair=[(0, 1, 0, 0, 0)] * 3, n_close=[0, 0, 0], min_distance=[1.0, 1.0, 1.0])
    return out


def criteria():
    return sc.ScreenCriteria(mask_type=MASK_TYPE)


def large_crystal(seed=5, n=300):
    """A crystal above the kernel's LDS staging limit (screening.STAGED_ATOMS), jittered off a grid so contacts are distinct."""
    assert n > sc.STAGED_ATOMS
    rng = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(7) / 7.0] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    frac = (g + rng.uniform(-0.03, 0.03, g.shape) + rng.randint(-2, 3, g.shape)).astype(F32)
    L = cell_from_params((14.0, 15.0, 16.0), np.array([80.0, 95.0, 105.0]) * DEG)
    small = _draw(np.random.RandomState(seed + 1))
    return _batch("large", [small, (frac, L, np.zeros(n, np.int32)), _draw(np.random.RandomState(seed + 2))])


def many_crystals(seed=9, B=1024):
    """A batch of 1,024 small crystals (1..24 atoms), every flag likely among them."""
    rng = np.random.RandomState(seed)
    crystals = []
    for _ in range(B):
        f, L, t = _draw(rng)
        n = 1 + len(f) % 24
        crystals.append((f[:n] * F32(3.0) - F32(1.0), L, t[:n]))
    return _batch("many", crystals)
