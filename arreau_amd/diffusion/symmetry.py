"""Space-group symmetry: sample crystals whose atoms sit in the Wyckoff orbits of a chosen group (an extension; rules in
include/arreau_hip.h, "space-group symmetry").

A space-group operation acts on fractional coordinates as the exact affine map x -> R x + t with an integer R (det +-1) and a
translation whose components are multiples of 1/12 (denominators 1, 2, 3, 4 or 6), taken modulo 1.  Groups are given by
generators in the CIF `_symmetry_equiv_pos_as_xyz` form ("-x+1/2,y,-z+1/2") and closed here (`close_group`), so no tables are
needed.  Closure is exact: translations are kept as integers in units of 1/12.

`SymmetrySpec` holds the group, its lattice system (one of lattice_systems.SYSTEMS, whose cells the group's rotations must
preserve) and the orbit layout of one crystal: every atom j has a leader l (the lowest atom index of its orbit) and the index k(j)
of an operation with g_k(x_l) = x_j (mod 1); every leader has its stabilizer H_l, the operations that fix it mod 1.  Build it from
a template (`from_template`: the template's Wyckoff structure) or as general positions (`general_positions`).

On the device the orbit is kept at every step: the network's position noise is pulled back to the leader and averaged, the leader
takes the VE reverse update with its own draw, is projected onto its site (the average over H_l of the affine images), and the
members are the images of the new leader.  Species: the leader draws from the orbit's mean logits, the members copy it.
`project_leader`, `expand`, `step_positions` and `step_species` restate that in float64; the GPU tests compare the kernels against them."""
import re
from fractions import Fraction
from typing import List, Optional, Sequence

import numpy as np

from .lattice_systems import SYSTEMS

MAX_ORDER = 192  # the largest space group in a conventional cell (Fm-3m and its kin)
_DEN = 12        # translations are exact multiples of 1/12
_AXES = "xyz"


def parse_symop(text: str):
    """(R int64 [3,3], t float64 [3]) of one operation in xyz form, e.g. "-x+1/2,y,-z+1/2" or "x-y,x,z+1/6".  Translations are
    exact rationals with denominator 1, 2, 3, 4 or 6, reduced to [0, 1).  Raises ValueError for anything else, including an R
    whose determinant is not +-1."""
    R, t12 = _parse(text)
    return R, t12 / _DEN


def _parse(text):
    if not isinstance(text, str):
        raise ValueError(f"symmetry operation must be a string, not {type(text).__name__}")
    parts = text.replace(" ", "").lower().strip("'\"").split(",")
    if len(parts) != 3:
        raise ValueError(f"symmetry operation {text!r}: three comma-separated components expected")
    R = np.zeros((3, 3), dtype=np.int64)
    t12 = np.zeros(3, dtype=np.int64)
    for i, expr in enumerate(parts):
        terms = re.findall(r"[+-]?[^+-]+", expr)
        if not expr or "".join(terms) != expr:
            raise ValueError(f"symmetry operation {text!r}: cannot read component {expr!r}")
        seen_const = False
        for term in terms:
            sign = -1 if term[0] == "-" else 1
            body = term.lstrip("+-")
            if body in ("x", "y", "z"):
                a = _AXES.index(body)
                if R[i, a] != 0:
                    raise ValueError(f"symmetry operation {text!r}: {body} appears twice in component {expr!r}")
                R[i, a] = sign
                continue
            if not re.fullmatch(r"\d+(/\d+)?", body) or seen_const:
                raise ValueError(f"symmetry operation {text!r}: cannot read term {term!r}")
            seen_const = True
            q = Fraction(body)
            if q.denominator not in (1, 2, 3, 4, 6):
                raise ValueError(f"symmetry operation {text!r}: translation {body} is not a multiple of 1/2, 1/3, 1/4 or 1/6")
            t12[i] = (t12[i] + sign * int(q * _DEN)) % _DEN
    det = int(round(np.linalg.det(R)))
    if det not in (1, -1):
        raise ValueError(f"symmetry operation {text!r}: det R = {det}, not +-1")
    return R, t12


def format_symop(R, t) -> str:
    """The xyz form of (R, t): the inverse of parse_symop."""
    t12 = np.rint(np.asarray(t, dtype=np.float64) * _DEN).astype(np.int64) % _DEN
    out = []
    for i in range(3):
        s = ""
        for a in range(3):
            c = int(R[i][a])
            if c:
                s += ("-" if c < 0 else ("+" if s else "")) + ("" if abs(c) == 1 else str(abs(c))) + _AXES[a]
        if t12[i]:
            s += "+" + str(Fraction(int(t12[i]), _DEN))
        out.append(s or "0")
    return ",".join(out)


def _as_exact(op):
    """(R, t12) of an operation given as a string or as (R, t) with t a multiple of 1/12."""
    if isinstance(op, str):
        return _parse(op)
    R, t = op
    R = np.asarray(R)
    if R.shape != (3, 3) or not np.array_equal(R, np.rint(R)):
        raise ValueError("a symmetry operation's R must be an integer 3 x 3 matrix")
    R = np.rint(R).astype(np.int64)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    t12f = t * _DEN
    if not np.all(np.abs(t12f - np.rint(t12f)) < 1e-9):
        raise ValueError(f"symmetry operation translation {t.tolist()} is not a multiple of 1/12")
    if int(round(np.linalg.det(R))) not in (1, -1):
        raise ValueError(f"symmetry operation {format_symop(R, t)}: det R is not +-1")
    return R, np.rint(t12f).astype(np.int64) % _DEN


def close_group(ops) -> list:
    """The group the operations generate, modulo integer translations: a list of (R int64 [3,3], t float64 [3]) with the
    identity first, then in order of discovery (deterministic).  `ops`: strings in xyz form or (R, t) pairs.  Raises ValueError
    when the group has more than 192 elements (no space group has, in a conventional cell)."""
    gens = [_as_exact(op) for op in ops]
    key = lambda R, t12: (tuple(R.reshape(-1).tolist()), tuple(t12.tolist()))
    ident = (np.eye(3, dtype=np.int64), np.zeros(3, dtype=np.int64))
    elems = [ident]
    index = {key(*ident)}
    i = 0
    while i < len(elems):
        R1, t1 = elems[i]
        for R2, t2 in gens:  # g1 . g2 and g2 . g1 for every element reached: x -> R1 (R2 x + t2) + t1
            for (Ra, ta), (Rb, tb) in (((R1, t1), (R2, t2)), ((R2, t2), (R1, t1))):
                R = Ra @ Rb
                t12 = (Ra @ tb + ta) % _DEN
                k = key(R, t12)
                if k not in index:
                    index.add(k)
                    elems.append((R, t12))
                    if len(elems) > MAX_ORDER:
                        raise ValueError(f"the operations generate more than {MAX_ORDER} elements (modulo integer "
                                         "translations): not a space group in a conventional cell")
        i += 1
    return [(R, t12 / _DEN) for R, t12 in elems]


def _wrap(d):
    """The wrapped difference of fractional coordinates, in [-0.5, 0.5)."""
    return d - np.floor(d + 0.5)


def _remainder(x):
    return np.mod(x, 1.0)


def _metric(system: str):
    """A metric tensor of the cells `lattice_systems` draws for `system`: generic lengths and angles that obey its ties and
    angles (monoclinic b-unique, hexagonal gamma = 120 degrees between a and b, rhombohedral axes)."""
    lengths = {"cubic": (3.7, 3.7, 3.7), "tetragonal": (3.7, 3.7, 5.3), "hexagonal": (3.7, 3.7, 5.3),
               "rhombohedral": (3.7, 3.7, 3.7)}.get(system, (3.7, 4.9, 5.3))
    angles = {"hexagonal": (90.0, 90.0, 120.0), "rhombohedral": (77.3, 77.3, 77.3), "monoclinic": (90.0, 103.7, 90.0),
              "triclinic": (71.3, 83.9, 101.2)}.get(system, (90.0, 90.0, 90.0))
    a, b, c = lengths
    ca, cb, cg = np.cos(np.deg2rad(angles))
    return np.array([[a * a, a * b * cg, a * c * cb], [a * b * cg, b * b, b * c * ca], [a * c * cb, b * c * ca, c * c]])


def check_metric(ops, system: str):
    """Raise ValueError unless every R of the group preserves the metric of `system`'s cells: R^T M R = M."""
    if system not in SYSTEMS:
        raise ValueError(f"unknown lattice system {system!r}: one of " + ", ".join(SYSTEMS))
    M = _metric(system)
    for R, t in ops:
        if not np.allclose(R.T @ M @ R, M, rtol=1e-9, atol=1e-9):
            raise ValueError(f"symmetry operation {format_symop(R, t)} does not preserve the metric of a {system} cell (the "
                             "group does not belong to that lattice system in the axes lattice_systems draws)")


class SymmetrySpec:
    """A space group, its lattice system and the orbit layout of one crystal of n_atoms atoms (see the module docstring).

    Attributes: ops (list of (R, t)), R int64 [G,3,3], R_inv int64 [G,3,3], t float64 [G,3], lattice_system, n_atoms,
    leader int64 [n] (local), op int64 [n] (k(j)), orbits (list of int64 arrays, the member atoms in ascending order),
    stabilizers (list of int64 arrays of op indices, one per orbit), anchors float64 [n_orbits,3] (the template's leader
    positions; None for general positions)."""

    def __init__(self, ops, lattice_system, leader, op, orbits, stabilizers, anchors):
        self.ops = ops
        self.R = np.stack([R for R, _ in ops]).astype(np.int64)
        self.t = np.stack([t for _, t in ops]).astype(np.float64)
        self.R_inv = np.rint(np.linalg.inv(self.R)).astype(np.int64)
        self.lattice_system = lattice_system
        self.leader = np.asarray(leader, dtype=np.int64)
        self.op = np.asarray(op, dtype=np.int64)
        self.orbits = [np.asarray(o, dtype=np.int64) for o in orbits]
        self.stabilizers = [np.asarray(h, dtype=np.int64) for h in stabilizers]
        self.anchors = None if anchors is None else np.asarray(anchors, dtype=np.float64).reshape(-1, 3)
        self.n_atoms = int(self.leader.shape[0])
        G = len(ops)
        for o, h in zip(self.orbits, self.stabilizers):
            if len(o) * len(h) != G:
                raise ValueError(f"orbit of atom {int(o[0])}: |orbit| {len(o)} x |stabilizer| {len(h)} != |G| {G}")

    @property
    def order(self) -> int:
        return len(self.ops)

    @property
    def leaders(self) -> np.ndarray:
        return np.array([int(o[0]) for o in self.orbits], dtype=np.int64)

    def __repr__(self):
        return (f"SymmetrySpec(|G|={self.order}, {self.lattice_system}, {self.n_atoms} atoms in {len(self.orbits)} orbits "
                f"of sizes {[len(o) for o in self.orbits]})")

    @classmethod
    def from_template(cls, frac, ops, lattice_system: str, tol: float = 1e-4) -> "SymmetrySpec":
        """The Wyckoff structure of a template crystal (fractional coordinates [n,3]) under the group `ops` generate.  Every
        image g(x_j) must match a template atom within `tol` (max-abs component of the wrapped difference).  The template's
        species are not used."""
        group = close_group(ops)
        check_metric(group, lattice_system)
        x = np.asarray(frac, dtype=np.float64).reshape(-1, 3)
        n = x.shape[0]
        if n < 1:
            raise ValueError("the symmetry template holds no atoms")
        # image[m, j]: the template atom g_m(x_j) lands on
        image = np.empty((len(group), n), dtype=np.int64)
        for m, (R, t) in enumerate(group):
            gx = x @ R.T + t
            d = np.abs(_wrap(gx[:, None, :] - x[None, :, :])).max(axis=2)  # [j, p]
            p = d.argmin(axis=1)
            bad = np.nonzero(d[np.arange(n), p] > tol)[0]
            if bad.size:
                j = int(bad[0])
                raise ValueError(f"symmetry template: the image of atom {j} under operation {m} ({format_symop(R, t)}) matches "
                                 f"no template atom within {tol} (nearest: atom {int(p[j])}, {d[j, p[j]]:.3g} away)")
            image[m] = p
        leader = np.full(n, -1, dtype=np.int64)
        op = np.zeros(n, dtype=np.int64)
        orbits, stabs, anchors = [], [], []
        for l in range(n):
            if leader[l] >= 0:
                continue
            members = sorted(set(image[:, l].tolist()))
            for j in members:
                if leader[j] >= 0:
                    raise ValueError(f"symmetry template: atom {j} lies in the orbits of atoms {int(leader[j])} and {l}")
                leader[j] = l
                op[j] = int(np.nonzero(image[:, l] == j)[0][0])  # the first operation taking the leader there
            orbits.append(members)
            stabs.append(np.nonzero(image[:, l] == l)[0])
            anchors.append(x[l])
        return cls(group, lattice_system, leader, op, orbits, stabs, np.array(anchors))

    @classmethod
    def general_positions(cls, ops, n_orbits: int, lattice_system: str) -> "SymmetrySpec":
        """n_orbits orbits of general positions: N = n_orbits |G| atoms, atom o |G| + m is g_m of leader o |G|, every
        stabilizer is the identity alone."""
        group = close_group(ops)
        check_metric(group, lattice_system)
        n_orbits = int(n_orbits)
        if n_orbits < 1:
            raise ValueError("general_positions needs at least one orbit")
        G = len(group)
        leader = np.repeat(np.arange(n_orbits) * G, G)
        op = np.tile(np.arange(G), n_orbits)
        orbits = [np.arange(o * G, (o + 1) * G) for o in range(n_orbits)]
        return cls(group, lattice_system, leader, op, orbits, [np.zeros(1, dtype=np.int64)] * n_orbits, None)

    # ---- float64 restatements of the device rules ------------------------------------------------------------------------
    def project_leader(self, o: int, y, anchor, wrap: bool = True):
        """Rule 3: the leader of orbit o onto its site, (1/|H|) sum_h (R_h y + t_h + n_h) with n_h = rint(a - R_h a - t_h) for
        the on-site anchor a; wrapped to [0, 1) unless wrap=False.  A general position (|H| = 1) is y itself."""
        y = np.asarray(y, dtype=np.float64)
        a = np.asarray(anchor, dtype=np.float64)
        H = self.stabilizers[o]
        if len(H) == 1:
            p = y.copy()
        else:
            acc = np.zeros(3)
            for h in H:
                n = np.rint(a - self.R[h] @ a - self.t[h])
                acc += self.R[h] @ y + self.t[h] + n
            p = acc / len(H)
        return _remainder(p) if wrap else p

    def expand(self, x_leaders, wrap: bool = True):
        """Rule 4: the crystal's positions [n,3] from its leaders' ([n_orbits,3], orbit order): x_j = R_k(j) x_l + t_k(j),
        wrapped unless wrap=False; the leaders themselves are copied."""
        xl = np.asarray(x_leaders, dtype=np.float64).reshape(-1, 3)
        out = np.empty((self.n_atoms, 3))
        for o, members in enumerate(self.orbits):
            l = int(members[0])
            for j in members:
                j = int(j)
                out[j] = xl[o] if j == l else self.R[self.op[j]] @ xl[o] + self.t[self.op[j]]
                if wrap and j != l:
                    out[j] = _remainder(out[j])
        return out

    def initial_positions(self, frac):
        """The initial state of a crystal of this spec from today's draw `frac` [n,3]: each leader projected onto its site
        (rule 3, anchored at the template's leader position; no wrap), the members expanded from it (rule 4, no wrap)."""
        x = np.asarray(frac, dtype=np.float64).reshape(-1, 3)
        xl = np.stack([self.project_leader(o, x[int(m[0])], self.anchors[o] if self.anchors is not None else x[int(m[0])],
                                           wrap=False) for o, m in enumerate(self.orbits)])
        return self.expand(xl, wrap=False)

    def step_positions(self, x, eps, z, sigma_t: float, sigma_s: float, wrap: bool = True):
        """The position part of one symmetric step of this crystal, in float64: x [n,3] the current (on-site) positions, eps
        [n,3] the network's position noise, z [n,3] the step's draws (only the leaders' rows are used), sigma_t / sigma_s the VE
        sigmas of the timesteps t and s.  Rules 1-4.  wrap=False leaves the leaders and their images unwrapped (which shows
        the leaders that left the cell, where the anchoring of rule 3 matters)."""
        x, eps, z = (np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (x, eps, z))
        s2, sp2 = float(sigma_t) ** 2, float(sigma_s) ** 2
        std = np.sqrt(sp2 * (s2 - sp2) / s2)
        xl = np.empty((len(self.orbits), 3))
        for o, members in enumerate(self.orbits):
            l = int(members[0])
            ebar = sum(self.R_inv[self.op[j]] @ eps[j] for j in members) / len(members)
            y = x[l] - ebar * (s2 - sp2) + std * z[l]
            xl[o] = self.project_leader(o, y, x[l], wrap=wrap)
        return self.expand(xl, wrap=wrap)

    def step_species(self, logits, types, u, t: int, s: int, q_one_step_transposed, q_mats):
        """The species part of one symmetric step of this crystal from timestep t to s, in float64 (rule 5): logits [n,S] the
        network's x0 logits, types [n] the current classes (only the leaders' are used), u [n,S] the step's uniforms (only the
        leaders' rows are used), q_one_step_transposed [T,S,S] and q_mats [T,S,S] the D3PM tables.  Per orbit: the mean logits
        over the members in member order; the posterior of the D3PM reverse with the leader's class as x_t -- the raw logits at
        t = 1, else log(fact1 + 1e-6) + log(fact2 + 1e-6) with fact1 row x_t of q_one_step_transposed[t-1] at stride 1 and column
        x_t of q_mats[t-s-1] on a strided step, fact2 = softmax . q_mats[s-1]; plus the Gumbel noise of the leader's uniforms
        clipped to [1e-6, 1], scaled by 0.2 at t = 1; the first arg-max, which every member takes.  Returns (classes int64 [n],
        margins float64 [n_orbits]: the distance between the two best values)."""
        lg = np.asarray(logits, dtype=np.float64)
        ty = np.asarray(types).reshape(-1).astype(np.int64)
        un = np.asarray(u, dtype=np.float64)
        q1t, qm = np.asarray(q_one_step_transposed, dtype=np.float64), np.asarray(q_mats, dtype=np.float64)
        t, s = int(t), int(s)
        out = np.empty(self.n_atoms, dtype=np.int64)
        margins = np.empty(len(self.orbits))
        for o, members in enumerate(self.orbits):
            l = int(members[0])
            mean = np.zeros(lg.shape[1])
            for j in members:
                mean += lg[int(j)]
            mean /= len(members)
            if t == 1:
                post = mean
            else:
                xt = int(ty[l])
                fact1 = q1t[t - 1, xt, :] if s == t - 1 else qm[t - s - 1][:, xt]
                p = np.exp(mean - mean.max())
                fact2 = (p / p.sum()) @ qm[s - 1]
                post = np.log(fact1 + 1e-6) + np.log(fact2 + 1e-6)
            val = post - np.log(-np.log(np.clip(un[l], 1e-6, 1.0))) * (0.2 if t == 1 else 1.0)
            best = int(np.argmax(val))  # (the first of equal values)
            out[members] = best
            margins[o] = val[best] - np.delete(val, best).max() if val.shape[0] > 1 else np.inf
        return out, margins

    def check_species(self, types, what="constant species"):
        """Raise ValueError unless the species [n] are constant on every orbit."""
        ty = np.asarray(types).reshape(-1)
        for members in self.orbits:
            v = ty[members]
            if not np.all(v == v[0]):
                raise ValueError(f"{what} differ within the orbit of atom {int(members[0])}: a space-group orbit shares "
                                 "one species")


def read_symops(path: str) -> List[str]:
    """The operations of a file with one operation per line in xyz form; `#` starts a comment, blank lines are skipped."""
    ops = []
    with open(path) as fh:
        for line in fh:
            line = line.split("#", 1)[0].strip()
            if line:
                parse_symop(line)  # (raises with the line's text)
                ops.append(line)
    if not ops:
        raise ValueError(f"{path}: no symmetry operations")
    return ops


def resolve(symmetry, B: Optional[int]):
    """The spec of every crystal (a list, None for an unconstrained crystal), or None when no crystal has one (the sampler as
    it was).  `symmetry`: one SymmetrySpec for every crystal of the batch (B needed), or a sequence with one entry per crystal."""
    if symmetry is None:
        return None
    if isinstance(symmetry, SymmetrySpec):
        if B is None:
            raise ValueError("symmetry: one spec for the batch needs num_samples_in_batch")
        specs = [symmetry] * int(B)
    else:
        try:
            specs = list(symmetry)
        except TypeError:
            raise ValueError("symmetry must be None, a SymmetrySpec, or a sequence with one (or None) per crystal") from None
        if B is not None and len(specs) != int(B):
            raise ValueError(f"symmetry holds {len(specs)} entries for a batch of {B} crystals")
        for s in specs:
            if s is not None and not isinstance(s, SymmetrySpec):
                raise ValueError("symmetry entries must be SymmetrySpec or None")
    return specs if any(s is not None for s in specs) else None


def batch_layout(specs, num_atoms_per_sample, lattice_system):
    """(atom counts [B], lattice systems [B]) of a batch whose crystals `specs` (from `resolve`) constrain: a spec decides its
    crystal's count and system; `num_atoms_per_sample` / `lattice_system`, if given, must agree there and give the others."""
    B = len(specs)
    if num_atoms_per_sample is None:
        counts = [None] * B
    elif isinstance(num_atoms_per_sample, (int, np.integer)):
        counts = [int(num_atoms_per_sample)] * B
    else:
        counts = [int(v) for v in num_atoms_per_sample]
        if len(counts) != B:
            raise ValueError(f"num_atoms_per_sample holds {len(counts)} counts for a batch of {B} crystals")
    if lattice_system is None or isinstance(lattice_system, str):
        names = [lattice_system] * B
    else:
        names = list(lattice_system)
        if len(names) != B:
            raise ValueError(f"lattice_system holds {len(names)} names for a batch of {B} crystals")
    for b, s in enumerate(specs):
        if s is None:
            if counts[b] is None:
                raise ValueError(f"crystal {b} has no symmetry spec: num_atoms_per_sample must give its atom count")
            continue
        if counts[b] is not None and counts[b] != s.n_atoms:
            raise ValueError(f"crystal {b}: num_atoms_per_sample says {counts[b]} atoms, its symmetry spec {s.n_atoms}")
        if names[b] is not None and names[b] != s.lattice_system:
            raise ValueError(f"crystal {b}: lattice_system {names[b]!r} disagrees with its symmetry spec's "
                             f"{s.lattice_system!r}")
        counts[b], names[b] = s.n_atoms, s.lattice_system
    return counts, names


def device_arrays(specs: Sequence[Optional[SymmetrySpec]], offsets, device) -> dict:
    """The device tables of a batch (arreau_symmetry, include/arreau_hip.h): per atom the global leader (-1: unconstrained
    crystal), the op from the leader and the global orbit (-1 likewise); the orbits' members and stabilizer ops as CSR; the
    operations' R, R^-1 and t as float32 (a spec object used by several crystals shares its rows).  `offsets`: the crystals'
    atom offsets [B+1]."""
    import torch
    off = np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets, dtype=np.int64).reshape(-1)
    N = int(off[-1])
    leader = np.full(N, -1, dtype=np.int32)
    op = np.zeros(N, dtype=np.int32)
    orbit = np.full(N, -1, dtype=np.int32)
    orbit_ptr, orbit_atoms, stab_ptr, stab_ops = [0], [], [0], []
    rot, rinv, trans = [], [], []
    op_base = {}
    for b, s in enumerate(specs):
        if s is None:
            continue
        first = int(off[b])
        if int(off[b + 1]) - first != s.n_atoms:
            raise ValueError(f"crystal {b} holds {int(off[b + 1]) - first} atoms, its symmetry spec {s.n_atoms}")
        if id(s) not in op_base:
            op_base[id(s)] = len(rot)
            rot.extend(s.R.reshape(-1, 9))
            rinv.extend(s.R_inv.reshape(-1, 9))
            trans.extend(s.t)
        base = op_base[id(s)]
        leader[first:first + s.n_atoms] = first + s.leader
        op[first:first + s.n_atoms] = base + s.op
        for members, H in zip(s.orbits, s.stabilizers):
            orbit[first + members] = len(orbit_ptr) - 1
            orbit_atoms.extend((first + members).tolist())
            orbit_ptr.append(len(orbit_atoms))
            stab_ops.extend((base + H).tolist())
            stab_ptr.append(len(stab_ops))
    i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32), device=device).contiguous()
    f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=device).contiguous()
    return {"leader": i32(leader), "op": i32(op), "orbit": i32(orbit), "orbit_ptr": i32(orbit_ptr), "orbit_atoms": i32(orbit_atoms),
            "stab_ptr": i32(stab_ptr), "stab_ops": i32(stab_ops), "rot": f32(np.reshape(rot, (-1, 9))),
            "rot_inv": f32(np.reshape(rinv, (-1, 9))), "trans": f32(np.reshape(trans, (-1, 3)))}
