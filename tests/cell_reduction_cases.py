"""Crystals with a known primitive cell for the tests of the cell reduction (diffusion/cell_reduction.py, csrc/reduce.hip).
`cases()`: rock salt as supercells of its primitive fcc cell, a P1 crystal, that crystal in skewed bases, a body-centred and a
base-centred cell; at most 16 atoms and 8 translations, so every strided loop of the kernel makes one trip.  `size_cases()` reaches
what lies past that: P1 crystals of 63, 64, 65 atoms (the candidate loop's second block of 64 lanes) and of 257 (the unstaged
path); a face-centred cell (m = 4, three translations that close on each other), a rhombohedrally centred one (m = 3, components of
1/3 and 2/3) and a 3x2x1 supercell (m = 6) of a 2-atom triclinic cell; its 3x3x3 (m = 27: 729 closure pairs, K x K = 841) and
4x4x4 (m = 64, the cap, K = 66) supercells; its 5x4x2 supercell with one atom moved, twice: candidates that only the first block
of 64 atoms rejects, and candidates that only the last one does; and three crystals of two rounds of 256 atoms, supercells of a 65- and a 66-atom P1
crystal (see `_rounds`).  `size_flag_cases()`: 65 translations (one past the cap), three accepted translations that divide n but
do not close, 261 atoms whose 4 translations do not divide them, and a NaN in atom 258 of 260.
Built from hand-written cells, never from the reduction's own output.  Every unflagged case is GUARDED: every decision margin the
float64 restatement reports exceeds ten times its derived float32 bound (asserted here, no case exempt).  Needs numpy alone; the
references are computed once per process and shared."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from arreau_amd.diffusion import cell_reduction as cr
from tests.symmetry_search_cases import cell, supercell

SYMPREC = 0.01  # A
PARAMS = cr.CellReductionParams(symprec=SYMPREC)
A_NACL = 5.64
FCC_PRIMITIVE = np.array([[0, .5, .5], [.5, 0, .5], [.5, .5, 0]]) * A_NACL
# unimodular integer matrices with entries up to +-3 (products of shears): the skewed bases
SKEWS = (np.array([[1, 3, 0], [0, 1, 0], [0, 0, 1]]), np.array([[1, 0, 0], [2, 1, 0], [-3, 1, 1]]),
         np.array([[1, 2, -1], [0, 1, 3], [0, 0, 1]]), np.array([[2, 3, 1], [1, 2, 1], [1, 1, 1]]))


@dataclass
class Case:
    name: str
    frac: np.ndarray     # [n,3] float32
    lattice: np.ndarray  # [3,3] float32
    types: np.ndarray    # [n] int32
    multiplicity: int
    params: cr.CellReductionParams = PARAMS

    @property
    def n(self):
        return int(self.frac.shape[0])


def _case(name, frac, lattice, types, multiplicity, params=PARAMS):
    return Case(name, np.ascontiguousarray(frac, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(lattice, dtype=np.float32),
                np.ascontiguousarray(types, dtype=np.int32), multiplicity, params)


def skewed(frac, lattice, U):
    """The same crystal in the basis U L: positions x U^-1 (row vectors), wrapped."""
    U = np.asarray(U, dtype=np.float64)
    assert abs(abs(np.linalg.det(U)) - 1.0) < 1e-9 and np.abs(U).max() <= 3
    return np.mod(np.asarray(frac, dtype=np.float64) @ np.linalg.inv(U), 1.0), U @ np.asarray(lattice, dtype=np.float64)


def rock_salt(reps):
    return supercell([[0, 0, 0], [.5, .5, .5]], FCC_PRIMITIVE, [11, 17], reps)


@lru_cache(maxsize=None)
def p1_crystal():
    rng = np.random.default_rng(20261018)
    return rng.uniform(0.05, 0.95, (7, 3)), cell(4.1, 5.3, 6.2, 71.3, 83.9, 101.2), np.array([3, 3, 3, 3, 8, 8, 8])


@lru_cache(maxsize=None)
def cases():
    """name -> Case: every family of the issue."""
    out = {}
    for reps, m in (((1, 1, 1), 1), ((2, 1, 1), 2), ((2, 2, 2), 8)):
        out["rock salt %dx%dx%d" % reps] = _case("rock salt %dx%dx%d" % reps, *rock_salt(reps), m)
    f, L, t = p1_crystal()
    out["P1"] = _case("P1", f, L, t, 1)
    for k, U in enumerate(SKEWS):
        fs, Ls = skewed(f, L, U)
        out[f"P1 skew {k}"] = _case(f"P1 skew {k}", fs, Ls, t, 1)
    ortho = cell(3.1, 3.7, 4.3, 81.0, 74.0, 97.0)  # a centring is a translation: the cell's angles are kept generic, no length ties
    x = np.array([[0.1, 0.2, 0.3], [0.4, 0.15, 0.7]])
    out["body-centred"] = _case("body-centred", np.concatenate([x, np.mod(x + 0.5, 1.0)]), ortho, [0, 1, 0, 1], 2)
    out["base-centred"] = _case("base-centred", np.concatenate([x, np.mod(x + (0.5, 0.5, 0.0), 1.0)]), ortho, [0, 1, 0, 1], 2)
    for c in out.values():
        assert_guard(c)
    return out


TWO_ATOM_CELL = cell(3.1, 3.7, 4.3, 81.0, 74.0, 97.0)  # the centred cells' of `cases()`
TWO_ATOM_X = np.array([[0.1, 0.2, 0.3], [0.4, 0.15, 0.7]])
C7 = cell(7.1, 8.3, 9.2, 71.3, 83.9, 101.2)
BIG_CELL = cell(11.5, 16.7, 26.0, 76.1, 72.7, 102.0)  # the match cases' big cell
SIZE_NAMES = ("P1 n63", "P1 n64", "P1 n65", "P1 n257", "face-centred", "R-centred", "2-atom 3x2x1", "2-atom 3x3x3", "2-atom 4x4x4",
              "first block decides", "last block decides", "rounds 260", "rounds 260 permuted", "rounds 264 permuted")
SIZE_FLAG_NAMES = ("65 translations", "open closure", "261 atoms", "nan in atom 258")


def _p1(n, lattice, seed, n_rare=1):
    """n atoms at uniform random positions: n_rare of species 1, the rest split between 4 and 8."""
    rest = n - n_rare
    return (np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)), lattice,
            np.array([1] * n_rare + [4] * (rest // 2) + [8] * (rest - rest // 2)))


def _rounds(prim, reps, fixed, seed):
    """The reps supercell of the primitive crystal `prim`, its atoms reordered: `fixed` maps a primitive atom j to the places its
    translation class (j, j + n, j + 2 n, ...: the supercell is cell-major) takes; every other atom goes to a place drawn with `seed`."""
    f, L, t = supercell(*prim, reps)
    n0, n = len(prim[2]), len(t)
    place = np.full(n, -1)
    for j, where in fixed.items():
        assert len(where) == n // n0
        place[list(where)] = np.arange(j, n, n0)
    free = np.nonzero(place < 0)[0]
    rest = np.setdiff1d(np.arange(n), place[place >= 0])
    place[free] = np.random.default_rng(seed).permutation(rest)
    assert sorted(place) == list(range(n))
    return f[place], L, t[place], place % n0


@lru_cache(maxsize=None)
def size_primitives():
    """name -> Case: the primitive crystal every supercell case of `size_cases()` was built from."""
    two = _case("2-atom", TWO_ATOM_X, TWO_ATOM_CELL, [0, 1], 1)
    out = {}
    # a centred cell's primitive crystal, written by hand: the rows of M are a primitive basis in the centred cell's basis
    for name, M in (("face-centred", np.array([[0, .5, .5], [.5, 0, .5], [.5, .5, 0]])),
                    ("R-centred", np.array([[2, 1, 1], [-1, 1, 1], [-1, -2, 1]]) / 3.0)):
        out[name] = _case(name + " primitive", np.mod(TWO_ATOM_X @ np.linalg.inv(M), 1.0), M @ TWO_ATOM_CELL, [0, 1], 1)
    out.update({k: two for k in ("2-atom 3x2x1", "2-atom 3x3x3", "2-atom 4x4x4")})
    out["rounds 260"] = out["rounds 260 permuted"] = size_cases()["P1 n65"]
    out["rounds 264 permuted"] = _case("P1 n66", *_p1(66, C7, 20261066, n_rare=2), 1)
    return out


@lru_cache(maxsize=None)
def size_cases():
    """name -> Case (SIZE_NAMES): the sizes, kinds of translation group and translation counts `cases()` does not reach."""
    out = {}
    for n, L, seed in ((63, C7, 20261063), (64, C7, 20261064), (65, C7, 20261065), (257, BIG_CELL, 20261257)):
        out[f"P1 n{n}"] = _case(f"P1 n{n}", *_p1(n, L, seed), 1)
    x, types = TWO_ATOM_X, [0, 1]
    centred = lambda ts: np.concatenate([np.mod(x + t, 1.0) for t in ts])
    out["face-centred"] = _case("face-centred", centred([(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)]), TWO_ATOM_CELL, types * 4, 4)
    third = 1.0 / 3.0
    out["R-centred"] = _case("R-centred", centred([(0, 0, 0), (2 * third, third, third), (third, 2 * third, 2 * third)]), TWO_ATOM_CELL,
                             types * 3, 3)
    for reps in ((3, 2, 1), (3, 3, 3), (4, 4, 4)):
        out["2-atom %dx%dx%d" % reps] = _case("2-atom %dx%dx%d" % reps, *supercell(x, TWO_ATOM_CELL, types, reps), int(np.prod(reps)))
    # 80 atoms, 5x4x2, one atom moved by 3 symprec: no translation is left (m = 1), and a candidate misses by 3 symprec at that atom
    # and at the atom it sends to that atom's place, nowhere else.  Atom 2 moved: for some candidates both lie in the first block of
    # 64 atoms and the block of atoms 64..79 fits exactly, so the first trip's rejection has to stand after the second.  Atom 70
    # moved: for some both lie in 64..79 and the first block fits exactly, so only the second trip rejects them.
    for name, moved, failing, fitting in (("first block decides", 2, slice(0, 64), slice(64, 80)),
                                          ("last block decides", 70, slice(64, 80), slice(0, 64))):
        f, L, t = supercell(x, TWO_ATOM_CELL, types, (5, 4, 2))
        f[moved] += np.linalg.solve(L.T, np.array([3.0 * SYMPREC, 0.0, 0.0]))
        c = out[name] = _case(name, f, L, t, 1)
        w, rare = c.frac.astype(np.float64), np.nonzero(c.types == 0)[0]
        only_there = 0
        for q in rare[1:]:
            d = cr.min_image_distance((w[:, None, :] + (w[q] - w[rare[0]])) - w[None, :, :], c.lattice.astype(np.float64))
            d[c.types[:, None] != c.types[None, :]] = np.inf
            only_there += d.min(axis=1)[failing].max() > 2.0 * SYMPREC and d.min(axis=1)[fitting].max() < 0.5 * SYMPREC
        assert only_there >= 4, (name, only_there)
    # two rounds of 256 atoms: 2x2x1 supercells, m = 4.  Unpermuted, the rarest species sits at 0, 65, 130, 195 and every class has
    # its first atom below 65.  Permuted, 260 atoms: the rarest species IS the class at 256..259 (an atom at 256 or more is the lowest
    # of its class only when the whole class is, and 260 atoms leave four such places: the rarest species cannot also sit in round
    # 0), so round 0 has no candidate and the last kept atom is 256.  Permuted, 264 atoms (two atoms of the rarest species in the
    # primitive cell): the class of p0 at 3, 100, 257, 262, so translations are accepted in both rounds and the count is carried;
    # the other class of that species at 261, 263 and two drawn places (candidates that are rejected); a class of species 4 at 256,
    # 258, 259, 260, so the last kept atom is 256 with kept atoms carried from round 0.
    p65 = out["P1 n65"]
    prim65 = (p65.frac.astype(np.float64), C7, p65.types)
    out["rounds 260"] = _case("rounds 260", *supercell(*prim65, (2, 2, 1)), 4)
    f, L, t, _ = _rounds(prim65, (2, 2, 1), {0: (256, 257, 258, 259)}, 20261260)
    out["rounds 260 permuted"] = _case("rounds 260 permuted", f, L, t, 4)
    f, L, t, cls = _rounds(_p1(66, C7, 20261066, n_rare=2), (2, 2, 1), {0: (3, 100, 257, 262), 2: (256, 258, 259, 260)}, 20261264)
    rare = np.nonzero(t == 1)[0]
    first_class = np.nonzero(cls == cls[rare[0]])[0]
    assert first_class.min() < 256 <= first_class.max(), "the class of p0 does not sit in both rounds"
    assert (rare < 256).sum() >= 2 and (rare >= 256).sum() >= 2
    out["rounds 264 permuted"] = _case("rounds 264 permuted", f, L, t, 4)
    assert tuple(out) == SIZE_NAMES
    for c in out.values():
        assert_guard(c)
    for name in ("rounds 260 permuted", "rounds 264 permuted"):
        c, ref = out[name], reference(out[name])
        assert np.nonzero(c.types == 1)[0].max() >= 256 and int(ref.keep[int(ref.n_out[0]) - 1]) >= 256, name
    return out


@dataclass
class FlagCase:
    case: Case
    flags: int
    n_translations: int


@lru_cache(maxsize=None)
def size_flag_cases():
    """name -> FlagCase (SIZE_FLAG_NAMES): crystals the reduction copies through, with the flags and the number of accepted
    translations the rules give.  Not guarded as a whole (a flagged crystal takes few decisions); the decisions that flag them are
    0.3 symprec or more from their thresholds by construction."""
    out = {}
    x, types = TWO_ATOM_X, [0, 1]
    out["65 translations"] = FlagCase(_case("65 translations", *supercell(x, TWO_ATOM_CELL, types, (13, 5, 1)), 1), cr.AMBIGUOUS, 65)
    # copy k of a 4x1x1 supercell moved along Cartesian x by (0, 0.35, 0.7, 0.35) symprec: the translations by 1/4 and 3/4 leave
    # residuals of at most 0.7 symprec, the one by 1/2 leaves 1.4: three are accepted, 3 divides 12, 1/4 + 1/4 has no partner
    f, L, t = p1_crystal()
    fs, Ls, ts = supercell(f[:3], L, [3, 8, 8], (4, 1, 1))
    fs = fs + np.repeat([0.0, 0.35, 0.7, 0.35], 3)[:, None] * np.linalg.solve(Ls.T, np.array([SYMPREC, 0.0, 0.0]))[None, :]
    out["open closure"] = FlagCase(_case("open closure", fs, Ls, ts, 1), cr.AMBIGUOUS, 3)
    # a 261st atom of species 8, 0.3 symprec beside an existing one: the 4 translations are still accepted and do not divide 261
    big = size_cases()["rounds 260 permuted"]
    f64, L64 = big.frac.astype(np.float64), big.lattice.astype(np.float64)
    beside = int(np.nonzero(big.types == 8)[0][0])
    extra = f64[beside] + np.linalg.solve(L64.T, np.array([0.3 * SYMPREC, 0.0, 0.0]))
    out["261 atoms"] = FlagCase(_case("261 atoms", np.concatenate([f64, extra[None, :]]), big.lattice, np.concatenate([big.types, [8]]), 1),
                                cr.AMBIGUOUS, 4)
    nan = big.frac.copy()
    nan[258, 1] = np.nan
    out["nan in atom 258"] = FlagCase(_case("nan in atom 258", nan, big.lattice, big.types, 1), cr.NONFINITE, 0)
    assert tuple(out) == SIZE_FLAG_NAMES
    closure = out["open closure"]
    assert closure.case.n % int(reference(closure.case).n_translations[0]) == 0  # not the exit `cases()` already reaches
    return out


def skewed_rock_salt(k=0, reps=(2, 1, 1)):
    """Rock salt in a skewed basis, for the cross-instrument checks.  NOT guarded: a skewed cubic cell's equal lengths and zero
    scalars are no longer exact in float32, so which of the equal vectors the reduction takes may differ from the restatement's;
    every choice is a primitive fcc cell."""
    f, L, t = rock_salt(reps)
    fs, Ls = skewed(f, L, SKEWS[k])
    return _case("rock salt %dx%dx%d skew %d" % (*reps, k), fs, Ls, t, int(np.prod(reps)))


_REFERENCES = {}


def reference(case):
    """The float64 restatement of one case, computed once per process."""
    key = (case.name, case.params)
    if key not in _REFERENCES:
        _REFERENCES[key] = cr.reduce_reference_f64(case.frac, case.lattice[None], [case.n], case.types, case.params)
    return _REFERENCES[key]


def assert_guard(case):
    """Every decision margin of the restatement exceeds ten times its float32 bound."""
    mg = reference(case).margins[0]
    for kind, pairs in mg.items():
        for margin, bound in pairs:
            assert margin > cr.GUARD * bound, f"{case.name}: a {kind} margin {margin:.3e} within {cr.GUARD} x its bound {bound:.3e}"


def batch_of(cs):
    """(frac [N,3], lattice [B,3,3], counts [B], types [N]) of a list of cases, float32 / int32."""
    return (np.concatenate([c.frac for c in cs]).astype(np.float32).reshape(-1, 3), np.stack([c.lattice for c in cs]).astype(np.float32),
            [c.n for c in cs], np.concatenate([c.types for c in cs]).astype(np.int32))


def lengths_angles(L):
    """Sorted lengths and the sorted |cosines| between the rows of a cell: equal for two bases that differ by order and sign."""
    L = np.asarray(L, dtype=np.float64)
    ln = np.linalg.norm(L, axis=1)
    cos = [abs(float(L[i] @ L[j]) / (ln[i] * ln[j])) for i, j in ((0, 1), (0, 2), (1, 2))]
    return np.sort(ln), np.sort(cos)
