"""Crystals with a known symmetry for the tests of the symmetry search (diffusion/symmetry_search.py, csrc/symfind.hip): built
from generators closed with symmetry.close_group and from hand-written cells, never from a search's own output.  Every case
is GUARDED: with the float64 restatement, the deviation of every lattice candidate of rule 2 and the residual of every (W, t)
rule 4 evaluates is at most symprec / 2 or at least 2 symprec (asserted here, no case exempt), so float32 and float64 agree on
every discrete output.  Needs numpy alone; the references are computed once per process and shared."""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

from arreau_amd.diffusion import symmetry_search as ss
from arreau_amd.diffusion.symmetry import close_group

SYMPREC = 0.01  # A
PARAMS = ss.SymmetrySearchParams(symprec=SYMPREC, max_ops=192)
NOISE = 2.0e-5  # sigma of the displaced versions, fractional: about 1e-4 A, residuals far below symprec / 2


@dataclass
class Case:
    name: str
    frac: np.ndarray       # [n,3] float32
    lattice: np.ndarray    # [3,3] float32
    types: np.ndarray      # [n] int32
    n_ops: int
    n_translations: int
    point_group: str
    ops: Optional[list] = None  # the closed group [(R, t)] the found operations must equal as a set
    params: ss.SymmetrySearchParams = field(default_factory=lambda: PARAMS)
    flags: int = 0

    @property
    def n(self):
        return int(self.frac.shape[0])


def cell(a, b, c, alpha=90.0, beta=90.0, gamma=90.0):
    """Rows a, b, c [3,3] float64 of a cell from lengths (A) and angles (degrees): a along x, b in the xy plane."""
    ca, cb, cg = np.cos(np.deg2rad([alpha, beta, gamma]))
    sg = np.sin(np.deg2rad(gamma))
    cx, cy = cb, (ca - cb * cg) / sg
    return np.array([[a, 0.0, 0.0], [b * cg, b * sg, 0.0], [c * cx, c * cy, c * np.sqrt(1.0 - cx * cx - cy * cy)]])


def orbits(generators, seeds, seed_types):
    """(closed group, positions [n,3], types [n]): the images of every seed point under the closed group, duplicates (modulo 1)
    dropped, in the order they appear."""
    group = close_group(generators)
    pos, ty = [], []
    for x, s in zip(seeds, seed_types):
        mine = []
        for R, t in group:
            y = np.mod(R @ np.asarray(x, dtype=np.float64) + t, 1.0)
            if not any(np.abs((y - z) - np.rint(y - z)).max() < 1e-6 for z in mine):
                mine.append(y)
        pos += mine
        ty += [s] * len(mine)
    return group, np.array(pos), np.array(ty, dtype=np.int32)


def supercell(frac, lattice, types, reps):
    """The reps = (n_a, n_b, n_c) supercell: cell-major order."""
    reps = np.asarray(reps)
    shifts = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), -1).reshape(-1, 3)
    f = ((np.asarray(frac, dtype=np.float64)[None, :, :] + shifts[:, None, :]) / reps[None, None, :]).reshape(-1, 3)
    return f, np.asarray(lattice, dtype=np.float64) * reps[:, None], np.tile(np.asarray(types), len(shifts))


def _case(name, frac, lattice, types, n_ops, n_translations, point_group, ops=None, params=PARAMS, flags=0):
    return Case(name, np.ascontiguousarray(frac, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(lattice, dtype=np.float32),
                np.ascontiguousarray(types, dtype=np.int32), n_ops, n_translations, point_group, ops, params, flags)


def _noisy(case, rng, name=None):
    f = case.frac.astype(np.float64) + rng.normal(0.0, NOISE, case.frac.shape)
    return _case(name or case.name + " displaced", f, case.lattice, case.types, case.n_ops, case.n_translations, case.point_group,
                 case.ops, case.params, case.flags)


FCC = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]], dtype=np.float64)
PM3M = ("-y,x,z", "z,x,y", "-x,-y,-z")
FM3M = PM3M + ("x,y+1/2,z+1/2", "x+1/2,y,z+1/2")


@lru_cache(maxsize=None)
def base_cases():
    """The table of the issue, their displaced versions and the broken inversion: a tuple of Case."""
    rng = np.random.default_rng(20261018)
    tri = cell(4.1, 5.3, 6.2, 71.3, 83.9, 101.2)
    out = []
    x = rng.uniform(0.05, 0.95, (6, 3))
    out.append(_case("triclinic", x, tri, np.zeros(6), 1, 1, "1", close_group(["x,y,z"])))
    inv = _case("triclinic with inversion", np.concatenate([x, 1.0 - x]), tri, np.zeros(12), 2, 1, "-1", close_group(["-x,-y,-z"]))
    out.append(inv)
    g, f, t = orbits(("-x,y+1/2,-z+1/2", "-x,-y,-z"), [(0.11, 0.23, 0.37), (0.42, 0.08, 0.19)], [1, 4])
    out.append(_case("P2_1/c", f, cell(5.1, 6.3, 7.2, beta=103.7), t, 4, 1, "2/m", g))
    g, f, t = orbits(("-x+1/2,-y,z+1/2", "-x,y+1/2,-z", "-x,-y,-z"), [(0.13, 0.21, 0.34), (0.41, 0.07, 0.18)], [3, 1])
    out.append(_case("Pnma", f, cell(5.4, 6.1, 7.3), t, 8, 1, "mmm", g))
    g, f, t = orbits(("-y,x,z", "-x,y,-z", "-x,-y,-z"), [(0.12, 0.27, 0.36)], [2])
    out.append(_case("P4/mmm", f, cell(4.2, 4.2, 5.9), t, 16, 1, "4/mmm", g))
    g = close_group(("x-y,x,z+1/2", "y,x,-z", "-x,-y,-z"))  # P6_3/mmc
    out.append(_case("hcp", [[1 / 3, 2 / 3, 0.25], [2 / 3, 1 / 3, 0.75]], cell(3.2, 3.2, 5.2, gamma=120.0), [0, 0], 24, 1, "6/mmm", g))
    g = close_group(PM3M)
    out.append(_case("CsCl", [[0, 0, 0], [.5, .5, .5]], cell(4.1, 4.1, 4.1), [5, 2], 48, 1, "m-3m", g))
    out.append(_case("NaCl", np.concatenate([FCC, np.mod(FCC + 0.5, 1.0)]), cell(5.64, 5.64, 5.64), [0] * 4 + [1] * 4, 192, 4, "m-3m",
                     close_group(FM3M)))
    g = close_group(("z,x,y", "-y,-x,-z", "-x,-y,-z"))  # R-3m in rhombohedral axes
    u = 0.237
    out.append(_case("R-3m rhombohedral axes", [[0, 0, 0], [u, u, u], [1 - u, 1 - u, 1 - u]], cell(4.5, 4.5, 4.5, 77.3, 77.3, 77.3),
                     [0, 1, 1], 12, 1, "-3m", g))
    out.append(_case("one atom, cubic", [[0.3, 0.6, 0.1]], cell(3.0, 3.0, 3.0), [7], 48, 1, "m-3m"))
    # the rarest species (3: one atom, as species 5 has -- the smaller id wins) is neither first nor species 0
    out.append(_case("perovskite", [[.5, .5, 0], [.5, 0, .5], [0, .5, .5], [0, 0, 0], [.5, .5, .5]], cell(3.9, 3.9, 3.9), [2, 2, 2, 5, 3], 48, 1,
                     "m-3m", close_group(PM3M)))
    out += [_noisy(c, rng) for c in list(out) if c.n > 1]
    broken = inv.frac.astype(np.float64).copy()
    broken[7] += (0.05, -0.04, 0.06)  # about 0.4 A: far beyond symprec
    out.append(_case("triclinic with inversion, one atom moved away", broken, tri, np.zeros(12), 1, 1, "1", close_group(["x,y,z"])))
    for c in out:
        assert_guard(c)
    return tuple(out)


@lru_cache(maxsize=None)
def shape_cases():
    """Atom counts where the kernel can go wrong -- 1, 2, 63, 64, 65 and one more than the 256 atoms it stages in LDS --, each a
    supercell with a known answer; max_ops holds every operation.  A dict name -> Case."""
    big = ss.SymmetrySearchParams(symprec=SYMPREC, max_ops=1536)
    one = ([[0.0, 0.0, 0.0]], cell(3.0, 3.0, 3.0), [7])
    base = {c.name: c for c in base_cases()}
    out = {"n1": base["one atom, cubic"], "n2": base["CsCl"]}
    f, L, t = supercell(*one, (3, 3, 7))      # a tetragonal lattice of 63 points: 16 rotations x 63 translations
    out["n63"] = _case("63 atoms", f, L, t, 1008, 63, "4/mmm", params=big)
    nacl = base["NaCl"]
    f, L, t = supercell(nacl.frac, nacl.lattice, nacl.types, (2, 2, 2))
    out["n64"] = _case("64 atoms, NaCl 2x2x2", f, L, t, 1536, 32, "m-3m", params=big)
    f, L, t = supercell(*one, (5, 13, 1))     # an orthorhombic lattice of 65 points
    out["n65"] = _case("65 atoms", f, L, t, 520, 65, "mmm", params=big)
    # 256 atoms of an fcc 4x4x4 supercell and, last, one atom of another species in an octahedral hole: its site symmetry
    # m-3m is all that is left, and the rarest species is neither first nor species 0
    f, L, t = supercell(FCC, cell(4.0, 4.0, 4.0), [7] * 4, (4, 4, 4))
    out["n257"] = _case("257 atoms", np.concatenate([f, [[0.125, 0.125, 0.125]]]), L, np.concatenate([t, [3]]), 48, 1, "m-3m")
    assert out["n257"].n == ss.STAGED_ATOMS + 1
    for c in out.values():
        assert_guard(c)
    return out


def overflow_case():
    """The 64-atom NaCl supercell with the default max_ops = 192: 1536 operations, OVERFLOW, the first 192 stored."""
    c = shape_cases()["n64"]
    return _case(c.name + " (overflow)", c.frac, c.lattice, c.types, 1536, 32, "m-3m", params=PARAMS, flags=ss.OVERFLOW)


_REFERENCES = {}


def reference(case):
    """The float64 restatement of one case (with details), computed once per process."""
    key = (case.name, case.params)
    if key not in _REFERENCES:
        _REFERENCES[key] = ss.symmetry_reference_f64(case.frac, case.lattice[None], [case.n], case.types, case.params, details=True)
    return _REFERENCES[key]


def assert_guard(case):
    """Every lattice deviation and every residual the search evaluates is <= symprec / 2 or >= 2 symprec."""
    ref = reference(case)
    s = float(np.float32(case.params.symprec))
    for what, v in (("lattice deviation", ref.lattice_dev[0]), ("residual", ref.all_residuals[0])):
        grey = (v > s / 2) & (v < 2 * s)
        assert not grey.any(), f"{case.name}: {what} {v[grey][:4]} between symprec / 2 and 2 symprec ({s})"


def batch_of(cases):
    """(frac [N,3], lattice [B,3,3], counts [B], types [N]) of a list of cases, float32 / int32."""
    return (np.concatenate([c.frac for c in cases]).astype(np.float32).reshape(-1, 3), np.stack([c.lattice for c in cases]).astype(np.float32),
            [c.n for c in cases], np.concatenate([c.types for c in cases]).astype(np.int32))
