"""Crystals with a known primitive cell for the tests of the cell reduction (diffusion/cell_reduction.py, csrc/reduce.hip): rock
salt as supercells of its primitive fcc cell, a P1 crystal, that crystal in skewed bases, a body-centred and a base-centred cell.
Built from hand-written cells, never from the reduction's own output.  Every case is GUARDED: every decision margin the float64
restatement reports exceeds ten times its derived float32 bound (asserted here, no case exempt).  Needs numpy alone; the
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
