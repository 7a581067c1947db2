"""Lattice systems: sample crystals of a chosen lattice system (an extension; rules in include/arreau_hip.h, "lattice systems").

A system fixes the cell's angles and ties some of its lengths:

    system         angles (degrees, the reference's prior)   tie code   tied axes
    cubic          90, 90, 90                                2          a = b = c
    tetragonal     90, 90, 90                                1          a = b
    orthorhombic   90, 90, 90                                0          none
    hexagonal      90, 90, 120                               1          a = b
    rhombohedral   alpha = beta = gamma ~ U(60, 120)         2          a = b = c
    monoclinic     90, U(90, 180), 90                        0          none
    triclinic      three draws from U(60, 120)               0          none

The angles come from `sample_bravais_angles` (reference diffusion_helpers.py:739-774), which returns DEGREES, and are passed to
the device in radians (`np.deg2rad`): `lattice_from_params` takes radians, and training sees radians (`matrix_to_params`
returns acos values).  gamma is the angle between a and b in `lattice_from_params`, so the tied pair is axes 0 and 1.

`lattice_system=None` is the sampler as it was, bit for bit: monoclinic angles in degrees, read by the device as radians -- the
reference's own behaviour (its deg2rad lines are commented out), under which an angle the prior calls "90" acts as about 116.6
degrees.  `None` and `"monoclinic"` therefore differ: the latter gives a cell with the angles its prior names.

Angles are never diffused.  Lengths are, per axis; the tie is kept on the device at every step (update and RePaint jump) and on
the host for the initial state (`tie_lengths`).  The float64 restatements `tied_update` / `tied_jump` are what the GPU tests
compare the kernels against."""
from typing import Optional, Sequence, Union

import numpy as np

# tie code per system: 0 none, 1 a = b, 2 a = b = c
TIE_CODES = {"cubic": 2, "tetragonal": 1, "orthorhombic": 0, "hexagonal": 1, "rhombohedral": 2, "monoclinic": 0,
             "triclinic": 0}
SYSTEMS = tuple(TIE_CODES)

LatticeSystemArg = Union[None, str, Sequence[Optional[str]]]


def check(lattice_system: LatticeSystemArg, B: int, lattice_known=None) -> Optional[list]:
    """The system of every crystal (a list of B names, None for a crystal without one), or None without any system.  Raises
    ValueError for an unknown name, a sequence of the wrong length, or a system on a crystal whose cell a condition knows
    (`lattice_known`: bool [B], SampleCondition.lattice_known(); the template's cell and angles already decide it).  Draws
    nothing."""
    if lattice_system is None:
        return None
    if isinstance(lattice_system, str):
        names = [lattice_system] * B
    else:
        try:
            names = list(lattice_system)
        except TypeError:
            raise ValueError("lattice_system must be None, one of " + ", ".join(SYSTEMS) + ", or one per crystal") from None
        if len(names) != B:
            raise ValueError(f"lattice_system holds {len(names)} names for a batch of {B} crystals")
    for name in names:
        if name is not None and name not in TIE_CODES:
            raise ValueError(f"unknown lattice system {name!r}: one of " + ", ".join(SYSTEMS))
    if lattice_known is not None:
        known = np.asarray(lattice_known, dtype=bool).reshape(-1)
        bad = [b for b, name in enumerate(names) if name is not None and known[b]]
        if bad:
            raise ValueError(f"lattice_system on crystals whose cell the condition knows (crystals {bad[:8]}): the template's "
                             "cell and angles decide it")
    return names


def resolve(lattice_system: LatticeSystemArg, B: int, lattice_known=None, uniforms=None):
    """(angles [B,3] float64, tie codes int32 [B] or None).  Validates first (`check`), then draws the angles per crystal in
    order from `sample_bravais_angles` on numpy's global generator: radians for a named system, and for None (the whole
    argument, or one crystal's entry) today's monoclinic draw in degrees, unconverted, with code 0.
    `uniforms` (keyed sampling): one uniform(low, high) source per crystal (keyed.angle_uniforms), used instead of numpy's
    generator, which is then not touched."""
    from .diffusion_helpers import sample_bravais_angles  # (needs torch; the names and tie codes above do not)
    names = check(lattice_system, B, lattice_known)
    src = (lambda b: None) if uniforms is None else (lambda b: uniforms[b])
    if names is None:
        return np.array([sample_bravais_angles("monoclinic", src(b)) for b in range(B)]), None
    angles = np.empty((B, 3), dtype=np.float64)
    for b, name in enumerate(names):
        angles[b] = sample_bravais_angles("monoclinic", src(b)) if name is None else np.deg2rad(sample_bravais_angles(name, src(b)))
    codes = np.array([0 if name is None else TIE_CODES[name] for name in names], dtype=np.int32)
    return angles, codes


def tied_axes(code: int) -> slice:
    """The tied group G of a code as a slice of the three axes (empty for code 0)."""
    return slice(0, int(code) + 1) if code > 0 else slice(0, 0)


def tie_lengths(lengths, codes):
    """The host tie of initial (or fixed) lengths, in place: lengths[b, G] = lengths[b, 0].  Works on torch tensors and numpy
    arrays [B,3]; returns `lengths`."""
    for b, code in enumerate(np.asarray(codes).reshape(-1)):
        if code > 0:
            lengths[b, 1:int(code) + 1] = lengths[b, 0]
    return lengths


def _tie_code(code, known):
    code = int(code)
    code = code if 0 <= code <= 2 else 0  # rule 5: outside 0..2 counts as 0 (the device flags it)
    return 0 if known else code          # rule 4: a known cell is not tied


def tied_update(xt, x0, z, t, s, alpha_bars, betas, codes, clipmax=0.999, len_mask=None):
    """Rule 1 in float64: the length update of every crystal b from t[b] to s[b] (VP_lattice.reverse_given_x0 with t - 1 replaced
    by s; the stride-1 step takes betas[t]) with the tie of codes[b].  xt [B,3] current lengths, x0 [B,3] the network's x0
    (pred_lengths_0 * num_atoms), z [B,3] the step's draws; for the axes of G x_t is the leader's, x0 the group's mean (summed in
    axis order) and z the leader's draw.  `len_mask`: crystals left untied (rule 4)."""
    xt, x0, z = (np.asarray(a, dtype=np.float64) for a in (xt, x0, z))
    ab, bt = np.asarray(alpha_bars, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    out = np.empty_like(xt)
    for b in range(xt.shape[0]):
        tb, sb = int(t[b]), int(s[b])
        ab_t, ab_p = ab[tb], ab[sb]
        beta = bt[tb] if sb == tb - 1 else min(1.0 - ab_t / ab_p, clipmax)
        denom = 1.0 - ab_t
        c0 = np.sqrt(ab_p) * beta
        c1 = np.sqrt(1.0 - beta) * (1.0 - ab_p)
        var = (1.0 - ab_p) * beta / denom
        code = _tie_code(codes[b], len_mask is not None and bool(len_mask[b]))
        g = tied_axes(code)
        n_g = g.stop - g.start
        for i in range(3):
            tied = n_g > 0 and i < g.stop
            x0_i = sum(x0[b, j] for j in range(n_g)) / n_g if tied else x0[b, i]
            xt_i, z_i = (xt[b, 0], z[b, 0]) if tied else (xt[b, i], z[b, i])
            zz = z_i if tb > 1 else 0.0
            out[b, i] = (c0 * x0_i + c1 * xt_i) / denom + var * zz
    return out


def tied_jump(lengths, z, s, t, alpha_bars, codes, len_mask=None):
    """Rule 2 in float64: the RePaint jump of the lengths of every crystal b from s[b] up to t[b] (VP_lattice.forward composed,
    abar_0 = 1) with the tie of codes[b]: the axes of G jump from the leader's length with the leader's draw."""
    lengths, z = np.asarray(lengths, dtype=np.float64), np.asarray(z, dtype=np.float64)
    ab = np.asarray(alpha_bars, dtype=np.float64)
    out = np.empty_like(lengths)
    for b in range(lengths.shape[0]):
        sb, tb = int(s[b]), int(t[b])
        ratio = ab[tb] / ab[sb] if sb > 0 else ab[tb]
        g = tied_axes(_tie_code(codes[b], len_mask is not None and bool(len_mask[b])))
        for i in range(3):
            j = 0 if g.start < g.stop and i < g.stop else i
            out[b, i] = np.sqrt(ratio) * lengths[b, j] + np.sqrt(1.0 - ratio) * z[b, j]
    return out
