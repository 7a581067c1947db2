"""The inputs the powder-pattern CPU and GPU tests share (test_xrd_cpu.py, test_gpu_xrd.py) and the float32 deviation tool measures
on (tools/exp/xrd_f32_deviation.py): the textbook cells, the three invariance pairs (Cu in its cubic and its primitive cell, a
5-atom triclinic crystal under a unimodular change of basis and in its 2 x 1 x 1 supercell), the 70-crystal ragged batch of random
crystals, a crystal past the LDS staging, one crystal per flag, and the invariance crystals again on grids of 2, 257 and 4096
points, with a window one grid point wide, with the window at its cap and with a Debye-Waller factor.  numpy only; the same bytes
for both.

A batch is a namespace name, frac [N,3] float32, lattice [B,3,3] float32, counts [B], species [N] (atomic numbers) and params (the
XrdParams it is built with); its amplitudes are xrd.host_weights(species, params).

The random crystals: 1..24 atoms, 18 A^3 per atom, the cell's lengths within a factor 1.6 of each other and its angles uniform in
60..120 degrees (a draw that is no cell, or a flat one, is drawn again), one per seed."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from arreau_amd.diffusion import xrd
from tests.neighbor_reference import cell_from_params

F32 = np.float32
DEG = np.pi / 180
DEFAULT = xrd.XrdParams()
TEXTBOOK_NAMES = ("simple_cubic", "bcc", "fcc", "diamond", "rock_salt", "cscl")
INVARIANCE_NAMES = ("cu_cubic", "cu_primitive", "triclinic", "triclinic_rebased", "triclinic_doubled")
INVARIANCE_PAIRS = (("cu_cubic", "cu_primitive"), ("triclinic", "triclinic_rebased"), ("triclinic", "triclinic_doubled"))
UNIMODULAR = np.array([[1, 1, 0], [0, 1, 1], [0, 0, 1]])
A_CU, A_FE, A_PO, A_C, A_NACL, A_CSCL = 3.61, 2.87, 3.35, 3.567, 5.64, 4.12
FCC_SITES = [[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]]
RAGGED_SEEDS = tuple(range(70))
RAGGED_MIDDLE = 35


def _batch(name, crystals, params=DEFAULT):
    """crystals: (frac, cell, atomic numbers) each."""
    return SimpleNamespace(name=name, frac=np.concatenate([np.asarray(c[0], dtype=F32).reshape(-1, 3) for c in crystals]),
                           lattice=np.stack([np.asarray(c[1], dtype=F32) for c in crystals]), counts=[len(c[2]) for c in crystals],
                           species=np.concatenate([np.asarray(c[2], dtype=np.int64).reshape(-1) for c in crystals]), params=params)


def cube(a):
    return np.eye(3) * a


def textbook_crystals():
    shift = lambda sites, d: [[(x + dx) % 1.0 for x, dx in zip(s, d)] for s in sites]
    return [([[0.1, 0.2, 0.3]], cube(A_PO), [84]),
            ([[0, 0, 0], [0.5, 0.5, 0.5]], cube(A_FE), [26, 26]),
            (FCC_SITES, cube(A_CU), [29] * 4),
            (FCC_SITES + shift(FCC_SITES, (0.25, 0.25, 0.25)), cube(A_C), [6] * 8),
            (FCC_SITES + shift(FCC_SITES, (0.5, 0.5, 0.5)), cube(A_NACL), [11] * 4 + [17] * 4),
            ([[0, 0, 0], [0.5, 0.5, 0.5]], cube(A_CSCL), [55, 17])]


def triclinic_crystal():
    L = cell_from_params((4.1, 4.9, 5.6), np.array([78.0, 84.0, 102.0]) * DEG).astype(np.float64)
    f = np.array([[0.11, 0.23, 0.37], [0.52, 0.71, 0.08], [0.83, 0.16, 0.64], [0.34, 0.92, 0.55], [0.67, 0.45, 0.81]])
    return f, L, [8, 14, 26, 38, 56]


def invariance_crystals():
    """Float32 holds none of the second descriptions exactly (the rebased rows are rounded sums, the halved coordinates rounded
    products): each pair describes the same crystal to 2^-24, which belongs to what the pairs are compared within."""
    f, L, z = triclinic_crystal()
    M = UNIMODULAR
    rebased = (f @ np.linalg.inv(M), M @ L, z)  # a'_i = sum_j M_ij a_j, f' = f M^-1: the same Cartesian positions
    doubled = (np.concatenate([f * [0.5, 1, 1], f * [0.5, 1, 1] + [0.5, 0, 0]]), L * np.array([[2.0], [1.0], [1.0]]), z + z)
    primitive = np.array([[0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]]) * A_CU
    return [(FCC_SITES, cube(A_CU), [29] * 4), ([[0, 0, 0]], primitive, [29]), (f, L, z), rebased, doubled]


def random_crystal(seed, n=None):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 25)) if n is None else n
    while True:
        L = cell_from_params(rng.uniform(1.0, 1.6, 3), rng.uniform(60.0, 120.0, 3) * DEG).astype(np.float64)
        v = abs(np.linalg.det(L))
        if np.isfinite(L).all() and v > 0.35 * np.prod(np.linalg.norm(L, axis=1)):
            break
    L = L * (18.0 * n / v) ** (1.0 / 3.0)
    return rng.uniform(-0.5, 1.5, (n, 3)), L, rng.integers(1, 84, n).tolist()


def flag_crystals():
    ok = ([[0.2, 0.4, 0.6]], cube(3.0), [13])
    flat = np.array([[3.0, 0, 0], [0, 3.0, 0], [3.0, 3.0, 0]])
    return [([[0.2, np.nan, 0.6]], cube(3.0), [13]), ([[0.2, 0.4, 0.6]], flat, [13]), (np.zeros((0, 3)), cube(3.0), []),
            ([[0.2, 0.4, 0.6]], np.diag([200.0, 3.0, 3.0]), [13]), ok]


FLAGS_EXPECTED = [xrd.NONFINITE, xrd.CELL, xrd.EMPTY, xrd.RANGE, 0]
# one step of the 257-point grid is 0.332 degrees: at fwhm 0.06 the window 12 sigma = 0.306 degrees holds one grid point at most
NARROW = xrd.XrdParams(n_points=257, fwhm=0.06)
WIDE = xrd.XrdParams(n_points=4096, fwhm=3.92)  # 6 sigma = 9.988 of the 10 degrees allowed: 963 grid points in a window
_BUILDERS = {
    "textbook": lambda: _batch("textbook", textbook_crystals()),
    "cscl unit": lambda: _batch("cscl unit", textbook_crystals()[-1:], xrd.XrdParams(scattering="unit")),
    "invariance": lambda: _batch("invariance", invariance_crystals()),
    "ragged": lambda: _batch("ragged", [random_crystal(s) for s in RAGGED_SEEDS]),
    "large": lambda: _batch("large", [random_crystal(500, xrd.cb.STAGED_ATOMS + 1)]),
    "flags": lambda: _batch("flags", flag_crystals()),
    "points 2": lambda: _batch("points 2", invariance_crystals(), xrd.XrdParams(n_points=2, two_theta_min=43.4, two_theta_max=50.5)),
    "points 257": lambda: _batch("points 257", invariance_crystals(), xrd.XrdParams(n_points=257)),
    "points 4096": lambda: _batch("points 4096", invariance_crystals(), xrd.XrdParams(n_points=4096)),
    "narrow": lambda: _batch("narrow", invariance_crystals(), NARROW),
    "wide": lambda: _batch("wide", invariance_crystals(), WIDE),
    "b_iso": lambda: _batch("b_iso", invariance_crystals(), xrd.XrdParams(b_iso=1.5, two_theta_max=150.0, wavelength=0.7093, max_index=127)),
}
BATCHES = tuple(_BUILDERS)


@lru_cache(maxsize=None)
def batch(name):
    return _BUILDERS[name]()


def weights(bt):
    return xrd.host_weights(bt.species, bt.params)


@lru_cache(maxsize=None)
def reference(name):
    """(the batch, its float64 restatement): computed once, shared, never changed."""
    bt = batch(name)
    return bt, xrd.xrd_reference(bt.frac, bt.lattice, bt.counts, weights(bt), bt.params)


def single(bt, b):
    """Crystal b of a batch as a batch of its own."""
    first = int(np.sum(bt.counts[:b]))
    n = bt.counts[b]
    return _batch(f"{bt.name}[{b}]", [(bt.frac[first:first + n], bt.lattice[b], bt.species[first:first + n])], bt.params)


def scale(r):
    """max(P_64) per crystal: what the bound is relative to (NaN for a flagged crystal)."""
    top = np.where(np.isnan(r.pattern), -np.inf, r.pattern).max(axis=1, initial=-np.inf)
    return np.where(np.isinf(top), np.nan, top)
