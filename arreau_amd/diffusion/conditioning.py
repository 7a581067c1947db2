"""Conditioned sampling (structure completion): known positions, species and cells held to a template while the sampler
generates the rest.  RePaint-style replacement without resampling jumps, applied inside the update kernels
(arreau_sample_loop_conditioned; the rules are stated in include/arreau_hip.h).  The reference's `constant_atoms`
(diffusion/diffusion_loss.py:289, 311-312, 345-346) is the case "every species known".

This module is host-side: the condition is described and validated here, in numpy, without a GPU; `device_arrays` uploads
it in the form the library takes."""
from dataclasses import dataclass, replace
from typing import Optional, Union

import numpy as np

from .lattice_helpers import matrix_to_params
from .tools.atomic_number_table import AtomicNumberTable

MaskLike = Union[bool, np.ndarray, list, None]


def _mask(value: MaskLike, n: int, what: str) -> np.ndarray:
    """bool -> all / none of n; an array -> a bool mask of n entries."""
    if value is None or isinstance(value, (bool, np.bool_)):
        return np.full(n, bool(value))
    m = np.asarray(value)
    if m.shape != (n,):
        raise ValueError(f"{what} must hold {n} entries, got shape {m.shape}")
    return m.astype(bool)


@dataclass
class SampleCondition:
    """What is known of each crystal of a batch.  num_atoms [B] defines the batch; frac_x [N,3] with position_mask [N],
    atomic_numbers [N] (Z, not class indices) with species_mask [N], lattice [B,3,3] (rows a, b, c) with lattice_mask [B].
    Unmasked entries are not read.  An absent array means "nothing of that kind is known"."""
    num_atoms: np.ndarray
    frac_x: Optional[np.ndarray] = None
    position_mask: Optional[np.ndarray] = None
    atomic_numbers: Optional[np.ndarray] = None
    species_mask: Optional[np.ndarray] = None
    lattice: Optional[np.ndarray] = None
    lattice_mask: Optional[np.ndarray] = None

    def __post_init__(self):
        self.num_atoms = np.asarray(self.num_atoms, dtype=np.int64).reshape(-1)

    @property
    def B(self) -> int:
        return int(self.num_atoms.shape[0])

    @property
    def N(self) -> int:
        return int(self.num_atoms.sum())

    @classmethod
    def from_sample_result(cls, result, fix_positions: MaskLike = False, fix_species: MaskLike = False,
                           fix_lattice: MaskLike = False) -> "SampleCondition":
        """A SampleResult (generated, or loaded from the crystals.npz / .h5 wire format) as a template.  Each fix_* is a bool
        (all / none) or a mask: per atom for positions and species, per crystal for the lattice."""
        num_atoms = np.asarray(result.num_atoms, dtype=np.int64).reshape(-1)
        B, N = int(num_atoms.shape[0]), int(num_atoms.sum())
        return cls(num_atoms=num_atoms,
                   frac_x=np.asarray(result.frac_x, dtype=np.float64), position_mask=_mask(fix_positions, N, "fix_positions"),
                   atomic_numbers=np.asarray(result.atomic_numbers), species_mask=_mask(fix_species, N, "fix_species"),
                   lattice=np.asarray(result.lattice, dtype=np.float64), lattice_mask=_mask(fix_lattice, B, "fix_lattice"))

    # ---- masks ------------------------------------------------------------------------------------------------
    def _m(self, name, n):
        m = getattr(self, name)
        return np.zeros(n, dtype=bool) if m is None else np.asarray(m).astype(bool).reshape(-1)

    def positions_known(self) -> np.ndarray:
        return self._m("position_mask", self.N)

    def species_known(self) -> np.ndarray:
        return self._m("species_mask", self.N)

    def lattice_known(self) -> np.ndarray:
        return self._m("lattice_mask", self.B)

    # ---- validation -------------------------------------------------------------------------------------------
    def validate(self, z_table: AtomicNumberTable) -> None:
        """Raise ValueError unless the condition is well formed for a model with this z-table."""
        B, N = self.B, self.N
        if B < 1 or (self.num_atoms < 1).any():
            raise ValueError("condition: num_atoms must hold one positive count per crystal")
        for name, data, mask, n, shape in (("position", "frac_x", "position_mask", N, (N, 3)),
                                           ("species", "atomic_numbers", "species_mask", N, (N,)),
                                           ("lattice", "lattice", "lattice_mask", B, (B, 3, 3))):
            m, v = getattr(self, mask), getattr(self, data)
            if m is not None and np.asarray(m).shape != (n,):
                raise ValueError(f"condition: {mask} must have shape ({n},), got {np.asarray(m).shape}")
            if v is not None and np.asarray(v).shape != shape:
                raise ValueError(f"condition: {data} must have shape {shape}, got {np.asarray(v).shape}")
            if m is not None and np.asarray(m).astype(bool).any() and v is None:
                raise ValueError(f"condition: a {name} mask needs {data} of shape {shape}")
        pm, sm, lm = self.positions_known(), self.species_known(), self.lattice_known()
        if pm.any() and not np.isfinite(np.asarray(self.frac_x, dtype=np.float64)[pm]).all():
            raise ValueError("condition: known fractional coordinates must be finite")
        if sm.any():
            z = np.asarray(self.atomic_numbers)[sm]
            if not np.isfinite(z.astype(np.float64)).all() or (z != np.round(z)).any():
                raise ValueError("condition: known atomic numbers must be integers")
            zs = set(int(v) for v in z_table.zs)
            bad = sorted(set(int(v) for v in z) - zs)
            if bad:
                raise ValueError(f"condition: atomic numbers {bad} are not in the model's z-table")
            if (z == AtomicNumberTable.MASK_ATOMIC_NUMBER).any():
                raise ValueError(f"condition: the mask state {AtomicNumberTable.MASK_ATOMIC_NUMBER} cannot be a known species")
        if lm.any():
            lat = np.asarray(self.lattice, dtype=np.float64)[lm]
            if not np.isfinite(lat).all():
                raise ValueError("condition: known cells must be finite")
            if not (np.sqrt((lat ** 2).sum(-1)) > 0).all():
                raise ValueError("condition: known cells must have positive lengths")

    def resolve_batch(self, num_atoms_per_sample=None, num_samples_in_batch=None):
        """(num_atoms [B] list, B): the condition defines the batch; given values must agree with it."""
        counts = [int(v) for v in self.num_atoms]
        if num_samples_in_batch is not None and int(num_samples_in_batch) != self.B:
            raise ValueError(f"num_samples_in_batch={num_samples_in_batch} disagrees with the condition's {self.B} crystals")
        if num_atoms_per_sample is not None:
            if isinstance(num_atoms_per_sample, (int, np.integer)):
                given = [int(num_atoms_per_sample)] * self.B
            else:
                given = [int(v) for v in num_atoms_per_sample]
            if given != counts:
                raise ValueError("num_atoms_per_sample disagrees with the condition's atom counts")
        return counts, self.B

    def check_sampling(self, z_table, *, noise: str, fixed_cell: bool, constant_species: bool) -> None:
        """validate() plus the combinations the sampler refuses."""
        if noise != "philox":
            raise ValueError("conditioned sampling needs noise='philox' (the replacement draws are in-kernel Philox draws)")
        self.validate(z_table)
        if fixed_cell and self.lattice_known().any():
            raise ValueError("a lattice mask and fixed_cell=True both fix the cell; give one of them")
        if constant_species and self.species_known().any():
            raise ValueError("use_constant_atomic_symbols / constant_atoms and a species mask both fix the species; give one of them")

    # ---- batch plumbing -----------------------------------------------------------------------------------------
    def slice(self, start: int, stop: int) -> "SampleCondition":
        """The condition of crystals [start, stop)."""
        first = np.concatenate([[0], np.cumsum(self.num_atoms)])
        a0, a1 = int(first[start]), int(first[stop])
        per_atom = lambda v: None if v is None else np.asarray(v)[a0:a1]
        per_crystal = lambda v: None if v is None else np.asarray(v)[start:stop]
        return SampleCondition(num_atoms=self.num_atoms[start:stop].copy(), frac_x=per_atom(self.frac_x),
                               position_mask=per_atom(self.position_mask), atomic_numbers=per_atom(self.atomic_numbers),
                               species_mask=per_atom(self.species_mask), lattice=per_crystal(self.lattice),
                               lattice_mask=per_crystal(self.lattice_mask))

    def tile(self, k: int) -> "SampleCondition":
        """The whole set of templates repeated k times (crystal order t0, t1, ..., t0, t1, ...)."""
        if int(k) < 1:
            raise ValueError("samples per template must be positive")
        rep = lambda v: None if v is None else np.concatenate([np.asarray(v)] * int(k), axis=0)
        return replace(self, num_atoms=np.tile(self.num_atoms, int(k)), frac_x=rep(self.frac_x),
                       position_mask=rep(self.position_mask), atomic_numbers=rep(self.atomic_numbers),
                       species_mask=rep(self.species_mask), lattice=rep(self.lattice),
                       lattice_mask=rep(self.lattice_mask))

    # ---- what the library takes -----------------------------------------------------------------------------------
    def known_angles(self) -> np.ndarray:
        """[B,3] angles (radians) of the template cells; rows of unknown cells are zero."""
        g0 = np.zeros((self.B, 3))
        lm = self.lattice_known()
        if lm.any():
            g0[lm] = matrix_to_params(np.asarray(self.lattice, dtype=np.float64)[lm])[1]
        return g0

    def device_arrays(self, z_table: AtomicNumberTable, device) -> dict:
        """The arreau_sample_condition arrays on `device`: x0 [N,3] f32, pos_mask [N] u8, a0 [N] i32, type_mask [N] u8,
        l0 [B,3] f32, len_mask [B] u8; a kind with nothing known is None."""
        import torch
        out = dict(x0=None, pos_mask=None, a0=None, type_mask=None, l0=None, len_mask=None)
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt).contiguous()
        pm, sm, lm = self.positions_known(), self.species_known(), self.lattice_known()
        if pm.any():
            x0 = np.where(pm[:, None], np.asarray(self.frac_x, dtype=np.float64), 0.0)
            out.update(x0=up(x0, torch.float32), pos_mask=up(pm.astype(np.uint8), torch.uint8))
        if sm.any():
            lut = {int(z): i for i, z in enumerate(z_table.zs)}
            a0 = np.array([lut[int(z)] if k else 0 for z, k in zip(np.asarray(self.atomic_numbers), sm)], dtype=np.int32)
            out.update(a0=up(a0, torch.int32), type_mask=up(sm.astype(np.uint8), torch.uint8))
        if lm.any():
            l0 = np.zeros((self.B, 3))
            l0[lm] = matrix_to_params(np.asarray(self.lattice, dtype=np.float64)[lm])[0]
            out.update(l0=up(l0, torch.float32), len_mask=up(lm.astype(np.uint8), torch.uint8))
        return out
