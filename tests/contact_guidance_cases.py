"""The crystals the contact-guidance tests share (tests/test_contact_guidance_cpu.py, tests/test_gpu_contact_guidance.py).  Every
contact of a case has d >= MIN_D and every pair and image a margin |d - d0| >= MIN_MARGIN, except where a case says otherwise
(`overlap`: the coincident pair); the CPU test checks this, so a case that misses it cannot pass silently.  Inputs are float32: the
kernel's own; the float64 restatement reads the same values."""
import functools

import numpy as np

from arreau_amd.diffusion.contact_guidance import CELL, EMPTY, NONFINITE, OVERLAP, ContactGuidance

T = 100  # the timesteps of the tests' synthetic models (tests/sampling_helpers.py)
MIN_D, MIN_MARGIN = 0.05, 1e-3
F32 = np.float32
DEFAULT = ContactGuidance()  # d0 = 0.5, w = 0.5, max_shells = 8


class GuidanceCase:
    """One batch: frac [N,3] and lattice [B,3,3] float32, counts [B], the crystals' timesteps t [B], params, and what the rule
    says of it: the flags per crystal and the unordered contacts per crystal (None: not stated, the restatement's)."""

    def __init__(self, name, frac, lattice, counts, params=DEFAULT, t=None, flags=None, contacts=None):
        self.name, self.params = name, params
        self.frac = np.ascontiguousarray(np.asarray(frac, dtype=np.float64).reshape(-1, 3).astype(F32))
        self.lattice = np.ascontiguousarray(np.asarray(lattice, dtype=np.float64).reshape(-1, 3, 3).astype(F32))
        self.counts = [int(n) for n in counts]
        assert sum(self.counts) == self.frac.shape[0] and len(self.counts) == self.lattice.shape[0]
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.t = np.asarray(t if t is not None else [T // 2] * len(self.counts), dtype=np.int32)
        self.flags = flags if flags is not None else [0] * len(self.counts)
        self.contacts = contacts

    @property
    def B(self):
        return len(self.counts)

    def crystal(self, b):
        a, e = self.offsets[b], self.offsets[b + 1]
        return GuidanceCase(f"{self.name}[{b}]", self.frac[a:e], self.lattice[b:b + 1], [self.counts[b]], self.params, self.t[b:b + 1],
                            [self.flags[b]], None if self.contacts is None else [self.contacts[b]])


def batch_of(name, cases, order=None):
    """The crystals of `cases` (one params) as one batch, in `order` (indices into the concatenation)."""
    crystals = [c.crystal(b) for c in cases for b in range(c.B)]
    assert all(c.params == crystals[0].params for c in crystals)
    crystals = [crystals[i] for i in (order if order is not None else range(len(crystals)))]
    return GuidanceCase(name, np.concatenate([c.frac for c in crystals]), np.concatenate([c.lattice for c in crystals]),
                        [c.counts[0] for c in crystals], crystals[0].params, np.concatenate([c.t for c in crystals]),
                        [c.flags[0] for c in crystals], None if any(c.contacts is None for c in crystals) else [c.contacts[0] for c in crystals])


def cell_from_params(lengths, angles_deg):
    """Rows a, b, c of a cell with the given lengths and angles (alpha between b and c, beta a and c, gamma a and b)."""
    a, b, c = lengths
    al, be, ga = np.deg2rad(angles_deg)
    cx = c * np.cos(be)
    cy = c * (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    return np.array([[a, 0, 0], [b * np.cos(ga), b * np.sin(ga), 0], [cx, cy, np.sqrt(c * c - cx * cx - cy * cy)]])


CUBE4 = 4.0 * np.eye(3)


def pair_case():
    """Two atoms 0.3 A apart along (1, 2, 2) / 3 in a 4 A cube."""
    return GuidanceCase("pair", [[0.3, 0.3, 0.3], np.array([0.3, 0.3, 0.3]) + 0.3 * np.array([1, 2, 2]) / 3 / 4], CUBE4, [2], contacts=[1])


def face_case():
    """A pair across the cell face: fractions 0.02 and 0.97 along x, 0.2 A apart through the boundary."""
    return GuidanceCase("face", [[0.02, 0.5, 0.5], [0.97, 0.5, 0.5]], CUBE4, [2], contacts=[1])


def triclinic_case():
    """60 / 70 / 80 degrees with a 2 A axis and d0 = 2.5: two shells along that axis, several images of one j in contact."""
    return GuidanceCase("triclinic", [[0.10, 0.20, 0.30], [0.45, 0.52, 0.41], [0.80, 0.15, 0.85]], cell_from_params((2.0, 5.5, 6.0), (60, 70, 80)),
                        [3], ContactGuidance(min_distance=2.5, weight=0.25))


def single_case():
    """n = 1 in a 0.45 A cube: the atom's own images lie inside d0 and are left out, so nothing is in contact."""
    return GuidanceCase("single", [[0.4, 0.6, 0.1]], 0.45 * np.eye(3), [1], contacts=[0])


def empty_case():
    return GuidanceCase("empty", np.zeros((0, 3)), CUBE4, [0], flags=[EMPTY], contacts=[0])


def overlap_case():
    """Atoms 0 and 1 coincide (skipped, OVERLAP); atom 2 sits 0.3 A from both: two real contacts."""
    return GuidanceCase("overlap", [[0.25, 0.5, 0.5], [0.25, 0.5, 0.5], [0.325, 0.5, 0.5]], CUBE4, [3], flags=[OVERLAP], contacts=[2])


def nan_case():
    return GuidanceCase("nan", [[0.1, 0.1, 0.1], [0.15, np.nan, 0.1]], CUBE4, [2], flags=[NONFINITE], contacts=[0])


def flat_case():
    """A 0.2 A thick cell: 2.5 images across it for d0 = 0.5, more than max_shells = 1 allows."""
    return GuidanceCase("flat", [[0.1, 0.1, 0.1], [0.15, 0.1, 0.1]], np.diag([4.0, 4.0, 0.2]), [2], ContactGuidance(max_shells=1), flags=[CELL],
                        contacts=[0])


def ragged_case(seed=15):
    """Crystals of 1, 2, 7, 20 and 65 atoms (65 crosses a wave in the j stride) at timesteps 1, 2, T/2, T-1, T; random positions
    in random triclinic cells, d0 = 0.9 so that the larger ones hold many contacts."""
    rng = np.random.RandomState(seed)
    counts = [1, 2, 7, 20, 65]
    cells = [cell_from_params(rng.uniform(4.5, 6.5, 3), rng.uniform(70, 110, 3)) for _ in counts]
    frac = rng.uniform(0, 1, (sum(counts), 3))
    frac[1:3] = [[0.2, 0.3, 0.4], [0.2, 0.3, 0.5]]  # the two-atom crystal holds a contact
    return GuidanceCase("ragged", frac, cells, counts, ContactGuidance(min_distance=0.9, weight=0.5), t=[1, 2, T // 2, T - 1, T])


BIG_CELL = ((11.5, 16.7, 26.0), (76.1, 72.7, 102.0))  # the big cell of the match and reduction cases
LOOP_PARAMS = ContactGuidance(min_distance=2.0, weight=0.3)  # the loop tests' parameters
LARGE_N = 257  # one atom more than the kernel stages in LDS (CRYSTAL_LDS_ATOMS = 256)


def large_case(seed=257, n=LARGE_N):
    """257 atoms in the big cell, d0 = 2.0: atoms 0..255 uniform with the third fraction squeezed into [0.05, 0.70], atom 256 alone
    at (0.5, 0.5, 0.875), farther than d0 from every atom and image.  n = 256 is the same crystal without its last atom: the
    largest the kernel stages in LDS, with the same cell and so the same image count M."""
    rng = np.random.RandomState(seed)
    frac = rng.uniform(0, 1, (LARGE_N - 1, 3))
    frac[:, 2] = 0.05 + 0.65 * frac[:, 2]
    frac = np.concatenate([frac, [[0.5, 0.5, 0.875]]])[:n]
    return GuidanceCase("large" if n == LARGE_N else f"large{n}", frac, cell_from_params(*BIG_CELL), [n], LOOP_PARAMS)


def large_between_small():
    """`large` between two small crystals of the same parameters: the block in front and the block behind must not matter."""
    frac = [[0.10, 0.20, 0.30], [0.30, 0.30, 0.40], [0.80, 0.15, 0.85]]  # 0.98 A between the first two
    small = [GuidanceCase(f"small{k}", frac, CUBE4, [3], LOOP_PARAMS) for k in range(2)]
    return batch_of("large", [small[0], large_case(), small[1]])


def eight_shells_case():
    """Three atoms in diag(4, 4, 0.26) with d0 = 2.0: 2.0 / 0.26 = 7.7, eight images along c, accepted at max_shells = 8.  Its twin in
    diag(4, 4, 0.24) needs nine and is CELL.  One batch: an accepted 17-image axis next to a rejected one."""
    frac = [[0.10, 0.20, 0.10], [0.40, 0.30, 0.45], [0.70, 0.62, 0.80]]
    return GuidanceCase("eight shells", frac + frac, [np.diag([4.0, 4.0, 0.26]), np.diag([4.0, 4.0, 0.24])], [3, 3], LOOP_PARAMS, flags=[0, CELL])


SEVENTY_COUNTS = [1, 2, 7, 20, 65] * 14


@functools.lru_cache(maxsize=None)
def seventy_case(seed=70):
    """70 crystals, counts cycling through 1, 2, 7, 20, 65, at timesteps spread evenly over 1..T (both ends included); cells and
    parameters as `ragged`.  Among some 10^6 pairs and images a random draw holds one within 1e-3 A of d0, so every crystal is
    drawn again (from the same generator) until it keeps MIN_D and MIN_MARGIN: a condition on the float64 restatement alone."""
    from arreau_amd.diffusion.contact_guidance import reference
    rng = np.random.RandomState(seed)
    params = ContactGuidance(min_distance=0.9, weight=0.5)
    crystals = []
    for b, n in enumerate(SEVENTY_COUNTS):
        for _ in range(1000):
            one = GuidanceCase(f"seventy[{b}]", rng.uniform(0, 1, (n, 3)), cell_from_params(rng.uniform(4.5, 6.5, 3), rng.uniform(70, 110, 3)), [n],
                               params, t=[1 + (b * (T - 1)) // (len(SEVENTY_COUNTS) - 1)])
            r = reference(one.frac, one.lattice, one.offsets, params)
            if r.flags[0] == 0 and (r.margin[0].size == 0 or r.margin[0].min() >= 2 * MIN_MARGIN) and (r.d[0].size == 0 or r.d[0].min() >= 2 * MIN_D):
                break
        else:
            raise AssertionError(f"no draw of crystal {b} keeps the margins")
        crystals.append(one)
    return batch_of("seventy", crystals)


BAD_T = [0, -3, T + 1, 5, T]  # `ragged` at timesteps outside 1..T: clamped to [1, 1, T, 5, T] and flagged


def launch_cases():
    """The cases only the launch tests and the precondition test run (too large for the finite-difference tests)."""
    return [large_between_small(), eight_shells_case(), seventy_case()]


def all_cases():
    return [pair_case(), face_case(), triclinic_case(), single_case(), empty_case(), overlap_case(), nan_case(), flat_case(), ragged_case()]


def mixed_batch(order=None):
    """The default-parameter cases as one batch: flagged crystals (EMPTY, OVERLAP, NONFINITE) between guided ones."""
    return batch_of("mixed", [pair_case(), nan_case(), face_case(), empty_case(), overlap_case(), single_case()], order)
