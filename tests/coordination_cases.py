"""The inputs the coordination search's CPU and GPU tests share (test_coordination_cpu.py, test_gpu_coordination.py): structures
with known coordination numbers, awkward cells, every size at which the kernel takes another path, every flag, and a seeded set
of random crystals, the same bytes for both.  numpy only.

A batch is a namespace frac [N,3] float32, lattice [B,3,3] float32, counts [B], species [N] (atomic numbers), params (the
CoordinationParams it is searched with) and expect: {"cn": per-atom list or None, "flags": per-crystal list or None}.

The random crystals (8..24 atoms, cell lengths 5..9 A, angles 70..110 degrees, one per seed of RANDOM_SEEDS) are all searched;
a crystal is GUARDED -- float32 and float64 must agree on its integers -- when its smallest float64 margin exceeds four times the
derived relative float32 bound of d2 (coordination.d2_relative_bound; the derivation is in that module's docstring), decided by
the float64 restatement alone."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from arreau_amd.diffusion import coordination as co
from tests.neighbor_reference import cell_from_params

F32 = np.float32
DEG = np.pi / 180
RANDOM_SEEDS = tuple(range(3000, 3069))  # 69 crystals; with the 67-atom one they make the 70-crystal ragged batch
DEFAULT = co.CoordinationParams()


def _batch(name, crystals, params=DEFAULT, cn=None, flags=None):
    """crystals: (frac, cell, atomic numbers) each."""
    return SimpleNamespace(name=name, frac=np.concatenate([np.asarray(c[0], dtype=F32).reshape(-1, 3) for c in crystals]),
                           lattice=np.stack([np.asarray(c[1], dtype=F32) for c in crystals]), counts=[len(c[2]) for c in crystals],
                           species=np.concatenate([np.asarray(c[2], dtype=np.int64).reshape(-1) for c in crystals]), params=params,
                           expect={"cn": cn, "flags": flags})


def cube(a):
    return np.eye(3, dtype=F32) * F32(a)


def fcc_primitive(a):
    return (np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=F32) * F32(a / 2)).astype(F32)


FCC_SITES = [[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]]


def known_structures():
    """(name, frac, cell, atomic numbers, coordination number per atom) of textbook structures."""
    shift = lambda sites, d: [[(x + dx) % 1.0 for x, dx in zip(s, d)] for s in sites]
    a_hcp = 3.0
    hexagonal = np.array([[a_hcp, 0, 0], [-a_hcp / 2, a_hcp * np.sqrt(3) / 2, 0], [0, 0, a_hcp * np.sqrt(8 / 3)]], dtype=F32)
    quarter = [[0.25, 0.25, 0.25], [0.75, 0.75, 0.25], [0.75, 0.25, 0.75], [0.25, 0.75, 0.75],
               [0.75, 0.75, 0.75], [0.25, 0.25, 0.75], [0.25, 0.75, 0.25], [0.75, 0.25, 0.25]]
    return [
        ("simple_cubic", [[0.1, 0.2, 0.3]], cube(3.0), [84], [6]),  # every neighbour is an image of the atom itself
        ("bcc_primitive", [[0.3, 0.3, 0.3]], (np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1]], dtype=F32) * F32(2.87 / 2)), [26], [8]),
        ("fcc_primitive", [[0.0, 0.0, 0.0]], fcc_primitive(3.61), [29], [12]),
        ("diamond", [[0, 0, 0], [0.25, 0.25, 0.25]], fcc_primitive(3.567), [6, 6], [4, 4]),
        ("hcp_ideal", [[1 / 3, 2 / 3, 0.25], [2 / 3, 1 / 3, 0.75]], hexagonal, [12, 12], [12, 12]),
        ("rock_salt", FCC_SITES + shift(FCC_SITES, (0.5, 0, 0)), cube(5.64), [11] * 4 + [17] * 4, [6] * 8),
        ("cscl", [[0, 0, 0], [0.5, 0.5, 0.5]], cube(4.11), [55, 17], [8, 8]),
        ("fluorite", FCC_SITES + quarter, cube(5.46), [20] * 4 + [9] * 8, [8] * 4 + [4] * 8),
        ("perovskite", [[0, 0, 0], [0.5, 0.5, 0.5], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]], cube(3.905), [38, 22, 8, 8, 8],
         [12, 6, 2, 2, 2]),
        # a needle cell, 2.2 x 2.2 x 30 A: three shells along a and b; the four images at 2.2 A, the next at 2.2 sqrt(2)
        ("needle", [[0.2, 0.4, 0.1], [0.2, 0.4, 0.6]], np.diag([2.2, 2.2, 30.0]).astype(F32), [3, 3], [4, 4]),
    ]


def known_batch(params=DEFAULT):
    ks = known_structures()
    cn = [c for k in ks for c in k[4]] if params.tol > 0 else None  # (tol = 0 counts bitwise ties only: nothing is pinned)
    return _batch("known", [(f, L, z) for _, f, L, z, _ in ks], params, cn=cn, flags=[0] * len(ks))


SKEWED_CELL = np.array([[4, 0, 0], [7.5, 1, 0], [0, 0, 6]], dtype=F32)
SKEWED = co.CoordinationParams(cutoff=3.0)  # (6 shells along a; at the default cutoff the cell needs 12 and is flagged CELL)


def skewed_batch():
    """One atom in a strongly skewed cell: its nearest images are +-(2 a - b) = +-(0.5, -1, 0), sqrt(1.25) A, outside the 27 nearest
    cells; the stored order is the image order, (-2, 1, 0) first."""
    return _batch("skewed", [([[0.3, 0.2, 0.1]], SKEWED_CELL, [14])], SKEWED, cn=[2], flags=[0])


def draw_random(seed):
    rng = np.random.RandomState(seed)
    n = int(rng.randint(8, 25))
    L = cell_from_params(rng.uniform(5.0, 9.0, size=3), rng.uniform(70.0, 110.0, size=3) * DEG)
    return rng.uniform(-1.0, 2.0, (n, 3)).astype(F32), L, rng.choice([8, 14, 22, 38], n)


def flag_batch():
    """Every flag but OVERFLOW, and the smallest sizes, in one ragged batch (default parameters)."""
    nan = [[0.1, np.nan, 0.3], [0.5, 0.5, 0.5]]
    crystals = [([[0.5, 0.5, 0.5]], cube(4.0), [5]),                                   # n = 1
                (np.zeros((0, 3), F32), cube(5.0), []),                                 # n = 0: EMPTY
                (nan, cube(5.0), [1, 1]),                                               # NONFINITE
                ([[0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [0.6, 0.1, 0.3]], cube(6.0), [7, 7, 8]),  # two coincident atoms: OVERLAP
                ([[0.5, 0.5, 0.5]], cube(20.0), [2]),                                   # alone in a 20 A cell: ISOLATED, nearest 20
                ([[0.1, 0.2, 0.3]], np.diag([30.0, 30.0, 0.3]).astype(F32), [3]),      # 20 shells along c: CELL
                ([[0.1, 0.2, 0.3]], np.array([[5, 0, 0], [0, np.inf, 0], [0, 0, 5]], dtype=F32), [3]),  # NONFINITE (the cell)
                draw_random(RANDOM_SEEDS[0])]
    # the coincident pair: each is the other's only neighbour (thr2 = 0), the third atom keeps its own
    return _batch("flags", crystals, cn=None, flags=[0, co.EMPTY, co.NONFINITE, co.OVERLAP, co.ISOLATED, co.CELL, co.NONFINITE, None])


OVERFLOWING = co.CoordinationParams(max_neighbors=4)


def overflow_batch():
    """fcc with room for four neighbours: OVERFLOW, cn still 12, the list the first four in (j, m) order."""
    return _batch("overflow", [([[0.0, 0.0, 0.0]], fcc_primitive(3.61), [29]), ([[0.1, 0.2, 0.3]], cube(3.0), [84])], OVERFLOWING,
                  cn=[12, 6], flags=[co.OVERFLOW, co.OVERFLOW])


def large_batch(seed=5):
    """A crystal of STAGED_ATOMS + 3 atoms (the path that forms positions from global memory) between two small ones."""
    n = co.cb.STAGED_ATOMS + 3
    rng = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(7) / 7.0] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    frac = (g + rng.uniform(-0.03, 0.03, g.shape) + rng.randint(-2, 3, g.shape)).astype(F32)
    L = cell_from_params((14.0, 15.0, 16.0), np.array([80.0, 95.0, 105.0]) * DEG)
    return _batch("large", [draw_random(seed + 1), (frac, L, np.full(n, 13)), draw_random(seed + 2)])


def ragged_batch():
    """70 crystals: the 69 random ones and, in their middle, one of 67 atoms (16 atoms per wave and a remainder of 3)."""
    rng = np.random.RandomState(67)
    big = (rng.uniform(0.0, 1.0, (67, 3)).astype(F32), cell_from_params((10.0, 11.0, 9.5), np.array([85.0, 95.0, 100.0]) * DEG),
           rng.choice([8, 26], 67))
    crystals = [draw_random(s) for s in RANDOM_SEEDS]
    crystals.insert(33, big)
    return _batch("ragged", crystals)


RAGGED_BIG = 33


def single(batch, b):
    """Crystal b of a batch as a batch of its own."""
    first = int(np.sum(batch.counts[:b]))
    n = batch.counts[b]
    return _batch(f"{batch.name}[{b}]", [(batch.frac[first:first + n], batch.lattice[b], batch.species[first:first + n])], batch.params)


def all_batches():
    """Every batch the kernel is compared on with the float32 restatement; tol = 0 (no crystal guarded: each nearest contact sits
    on its own threshold) among them."""
    return [known_batch(), known_batch(co.CoordinationParams(tol=0.0)), skewed_batch(), flag_batch(), overflow_batch(), large_batch(),
            ragged_batch()]


@lru_cache(maxsize=None)
def references():
    """{batch name (+ ' tol0'): (batch, float32 restatement, float64 restatement)}, computed once and shared; never modified."""
    out = {}
    for bt in all_batches():
        key = bt.name + (" tol0" if bt.params.tol == 0.0 else "")
        out[key] = (bt, co.coordination_reference_f32(bt.frac, bt.lattice, bt.counts, bt.params),
                    co.coordination_reference_f64(bt.frac, bt.lattice, bt.counts, bt.params))
    return out
