"""The inputs the uniqueness CPU and GPU tests share (test_uniqueness_cpu.py, test_gpu_uniqueness.py), the same bytes for both,
and their float64 / float32 restatements, computed once per process.  numpy only.

  * `invariance_set`: a perturbed 8-atom two-species cell and its six equivalent variants -- every coordinate, cell entry,
    shift and the rotation (120 degrees about (1, 1, 1): a cyclic permutation of the axes) exact in float32, so the float64
    restatement sees exactly equivalent crystals --, then a CsCl-like polymorph of the same formula and crystals of other
    formulas.
  * `ragged_batch`: 1 to 257 atoms, 1 to 9 species, a skewed triclinic cell, a flat cell, a NaN coordinate, an empty crystal.
    Random members are drawn again while a contact lies within screening.distance_bound of r_cut (float64 restatement).
  * `match_sets`: two pools of 70 small crystals of a few formulas with planted copies, near copies, flagged rows and lone
    formulas; the tests take prefixes of 1, 33 and 70."""
import functools
from types import SimpleNamespace

import numpy as np

from arreau_amd.diffusion import uniqueness as uq

F32 = np.float32
BASE_CELL = np.array([[5.5, 0, 0], [0.25, 5.75, 0], [-0.5, 0.375, 5.625]], dtype=F32)
ROCKSALT = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5], [.5, 0, 0], [0, .5, 0], [0, 0, .5], [.5, .5, .5]])
MATCH_SIZES = (1, 33, 70)


def params():
    return uq.FingerprintParams()


def batch(name, crystals):
    """crystals: (frac [n,3], cell [3,3], species [n]) each."""
    return SimpleNamespace(name=name, frac=np.concatenate([np.asarray(c[0], dtype=F32).reshape(-1, 3) for c in crystals]),
                           lattice=np.stack([np.asarray(c[1], dtype=F32) for c in crystals]), counts=[len(c[2]) for c in crystals],
                           types=np.concatenate([np.asarray(c[2], dtype=np.int32).reshape(-1) for c in crystals]), crystals=list(crystals))


def base_crystal():
    rng = np.random.RandomState(7)
    frac = ROCKSALT + rng.randint(-30, 31, ROCKSALT.shape) / 1024.0  # exact in float32
    return frac.astype(F32), BASE_CELL, np.array([11, 11, 11, 11, 17, 17, 17, 17], np.int32)


VARIANTS = ("base", "permuted", "shifted", "lattice_shifts", "rotated", "basis_change", "supercell")


def invariance_set():
    """The seven equivalent crystals (VARIANTS), then `cscl` (the other AB structure), `ab2`, `a2b` and `other_pair`."""
    f, L, t = base_crystal()
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    shifts = np.array([[1, 0, 0], [0, -2, 0], [0, 0, 3], [-1, 1, 0], [0, 0, 0], [2, 2, -2], [0, -1, 0], [5, 0, -4]], dtype=F32)
    fb = f.copy()
    fb[:, 1] = f[:, 1] - f[:, 0]  # rows (a + b, b, c): f_a (a + b) + (f_b - f_a) b + f_c c
    Lb = np.stack([L[0] + L[1], L[1], L[2]])
    fs = np.concatenate([f * F32([0.5, 1, 1]), f * F32([0.5, 1, 1]) + F32([0.5, 0, 0])])
    out = [(f, L, t), (f[perm], L, t[perm]), (f + F32([0.375, -0.25, 0.0625]), L, t), (f + shifts, L, t), (f, L[:, [2, 0, 1]], t),
           (fb, Lb, t), (fs, L * F32([[2], [1], [1]]), np.concatenate([t, t]))]
    cube = lambda a: np.eye(3, dtype=F32) * F32(a)
    out.append(([[0, 0, 0], [.5, .5, .5]], cube(3.5), [11, 17]))                          # cscl
    out.append(([[0, 0, 0], [.25, .25, .25], [.75, .75, .75]], cube(4.5), [11, 17, 17]))  # ab2
    out.append(([[0, 0, 0], [.25, .25, .25], [.75, .75, .75]], cube(4.5), [17, 11, 11]))  # a2b
    out.append((f, L, np.where(t == 11, 19, 35)))                                         # other_pair
    return batch("invariance", out)


INVARIANCE_NAMES = VARIANTS + ("cscl", "ab2", "a2b", "other_pair")


def _random_crystal(rng, n, n_species, volume_per_atom=18.0, first_species=0):
    a = (n * volume_per_atom) ** (1.0 / 3.0)
    L = (np.eye(3) * a + rng.uniform(-0.1, 0.1, (3, 3)) * a).astype(F32)
    t = np.concatenate([np.arange(n_species), rng.randint(0, n_species, max(0, n - n_species))])[:n] + first_species
    return rng.uniform(0, 1, (n, 3)).astype(F32), L, rng.permutation(t).astype(np.int32)


def _clear_of_cut(draw):
    """Draw until no contact lies within the float32 distance bound of r_cut (decided with the float64 restatement)."""
    while True:
        c = draw()
        r = uq.fingerprint_reference_f64(c[0], [c[1]], [len(c[2])], c[2], params(), details=True)
        if r.near_cut[0] == 0:
            return c


RAGGED_NAMES = ("one_atom", "two_atoms", "seven_three_species", "twenty", "sixty_five_eight_species", "above_staging", "nine_species",
                "skewed", "flat_cell", "nan_coordinate", "empty", "sparse", "twenty_again")


@functools.lru_cache(maxsize=None)
def ragged_batch():
    rng = np.random.RandomState(31)
    big = lambda: _random_crystal(rng, uq.STAGED_ATOMS + 1, 2, volume_per_atom=40.0)
    skew = np.array([[4, 0, 0], [7.5, 3, 0], [1, 2, 9]], dtype=F32)  # shells 3, 3, 1 for r_cut = 6.5
    out = [_clear_of_cut(lambda: _random_crystal(rng, 1, 1, 30.0)), _clear_of_cut(lambda: _random_crystal(rng, 2, 2, 25.0)),
           _clear_of_cut(lambda: _random_crystal(rng, 7, 3)), _clear_of_cut(lambda: _random_crystal(rng, 20, 2)),
           _clear_of_cut(lambda: _random_crystal(rng, 65, 8)), _clear_of_cut(big),
           _random_crystal(rng, 12, 9), _clear_of_cut(lambda: (rng.uniform(0, 1, (3, 3)).astype(F32), skew, np.array([3, 1, 3], np.int32))),
           ([[0.1, 0.2, 0.3]], np.diag([30.0, 30.0, 0.3]).astype(F32), [0]), ([[0.1, np.nan, 0.3], [0.5, 0.5, 0.5]], np.eye(3, dtype=F32) * 5, [0, 1]),
           (np.zeros((0, 3), F32), np.eye(3, dtype=F32) * 5, np.zeros(0, np.int32)),
           _clear_of_cut(lambda: _random_crystal(rng, 2, 1, 500.0)), None]
    out[-1] = out[3]  # the same crystal twice in one batch: the same row
    return batch("ragged", out)


RAGGED_FLAGS = [0, 0, 0, 0, 0, 0, uq.MANY_SPECIES, 0, uq.CELL, uq.NONFINITE, uq.EMPTY, 0, 0]


def _small(rng, kind):
    """A small random crystal of one of a few formulas (species ids are atomic numbers)."""
    species = {"A": [6], "AB": [11, 17], "AB2": [22, 8, 8], "A2B": [22, 22, 8], "ABC": [20, 22, 8], "CD": [12, 8], "lone": [79, 47, 47, 47]}[kind]
    n = len(species)
    a = (n * 20.0) ** (1.0 / 3.0)
    L = (np.eye(3) * a + rng.uniform(-0.15, 0.15, (3, 3)) * a).astype(F32)
    return rng.uniform(0, 1, (n, 3)).astype(F32), L, np.array(species, np.int32)


def _pool(seed, lone_at):
    rng = np.random.RandomState(seed)
    kinds = ["AB", "AB2", "A", "A2B", "ABC", "CD"]
    out = []
    for k in range(70):
        if k == lone_at:
            out.append(_small(rng, "lone"))
        elif k in (9, 40):
            out.append(([[0.1, np.inf, 0.3]], np.eye(3, dtype=F32) * 4, [6]) if k == 9 else (np.zeros((0, 3), F32), np.eye(3, dtype=F32) * 4, np.zeros(0, np.int32)))
        elif k in (12, 20, 35, 50, 69):  # an exact copy of an earlier crystal (12 and 20 copy the same one: the smaller index wins)
            out.append(out[{12: 3, 20: 3, 35: 17, 50: 12, 69: 0}[k]])
        elif k in (25, 61):              # a near copy: atoms moved by about 0.01 A -- inside the tolerance
            f, L, t = out[k - 20]
            out.append(((f + rng.uniform(-1, 1, f.shape) * 0.002).astype(F32), L, t))
        else:
            kind = "AB2" if k in (5, 41) else kinds[rng.randint(len(kinds))]  # (5 and 41 are copied with moved atoms: more than one atom)
            out.append(_clear_of_cut(lambda: _small(rng, kind)))
    return out


@functools.lru_cache(maxsize=None)
def match_sets():
    """(X, Y): two batches of 70; Y holds copies and near copies of X's members among crystals of its own."""
    xs = _pool(101, lone_at=30)
    ys = _pool(202, lone_at=5)
    for k, src in ((2, 0), (16, 7), (17, 7), (33, 31), (48, 61), (65, 3)):  # Y[16] and Y[17] are the same copy: X[7] matches 16
        ys[k] = xs[src]
    return batch("match_x", xs), batch("match_y", ys)


@functools.lru_cache(maxsize=None)
def reference_f64(which):
    """The float64 restatement of a named batch with its details, computed once: 'invariance', 'ragged', 'match_x', 'match_y'."""
    b = {"invariance": invariance_set, "ragged": ragged_batch, "match_x": lambda: match_sets()[0], "match_y": lambda: match_sets()[1]}[which]()
    return uq.fingerprint_reference_f64(b.frac, b.lattice, b.counts, b.types, params(), details=True)


def prefix(ref, B):
    """The first B rows of a fingerprinted set (a namespace) as a dict."""
    return {k: getattr(ref, k)[:B] for k in ("fingerprint", "species", "counts", "flags")}
