"""The sampling-step entry points at the corners the 4-to-6-crystal step tests do not reach (cases and their reach:
tests/sampling_corner_cases.py; guards: test_sampling_corners_cpu.py): 67 ragged crystals that each hold their own pair of
timesteps, S = 124 / 2 / 12 classes and T = 2.  One launch per case against the float64 restatements gathered per crystal, with
the bounds of each entry point's own restatement test and every class equal; bitwise against the constant-pair launches, the
untied step and the P1 symmetric step; the eta, inversion and conditioned resampled loops on the same batch bitwise against
their steps and events in both loop forms, and one conditioned step in value.  Last, the contract of the loop's graph key on the
same batch (section 6: 7 tests of three-step loops, 2.8 s together on an MI355X).  Needs an MI355X: `-m gpu`.

Measured on an MI355X (74 tests in 5.1 s; the slowest 0.5 s, the first loop of the module; every other at most 0.2 s).  Largest
error, positions wrapped / lengths / cell, per model; the bounds are 1e-5 for positions and 1e-5 max(1, magnitude) for lengths and
cell, the magnitude being about 7 (S12-T2: about 115, the 130-atom crystal's x0 at T = 2).  No class differed in any case.

    entry point         S12                        S124                       S2                         S12-T2
    reverse_step        1.9e-7 / 3.5e-7 / 6.2e-7   2.2e-7 / 4.0e-7 / 5.4e-7   2.1e-7 / 6.0e-7 / 6.0e-7   2.2e-7 / 1.0e-5 / 9.0e-6
    reverse_step_to     1.7e-7 / 2.5e-6 / 2.0e-6   1.7e-7 / 2.4e-6 / 2.1e-6   2.2e-7 / 3.0e-6 / 2.5e-6   2.0e-7 / 6.1e-6 / 6.9e-6
    reverse_step_tied   1.7e-7 / 2.2e-6 / 1.9e-6   1.7e-7 / 1.8e-6 / 1.8e-6   2.2e-7 / 2.4e-6 / 2.1e-6   2.0e-7 / 6.1e-6 / 6.9e-6
    eta 0               1.3e-7 / 3.8e-7 / 6.0e-7   1.3e-7 / 2.5e-7 / 7.9e-7   1.3e-7 / 6.0e-7 / 6.7e-7   1.2e-7 / 6.9e-6 / 1.2e-5
    eta 0.5             2.0e-7 / 2.8e-7 / 5.9e-7   2.3e-7 / 4.4e-7 / 7.0e-7   2.2e-7 / 4.6e-7 / 7.3e-7   1.9e-7 / 5.1e-6 / 5.8e-6
    eta 0, tied         1.3e-7 / 3.4e-7 / 5.5e-7   1.3e-7 / 5.4e-7 / 7.0e-7   1.3e-7 / 6.0e-7 / 8.2e-7   1.2e-7 / 6.9e-6 / 1.2e-5
    eta 0.5, tied       2.0e-7 / 3.7e-7 / 6.5e-7   2.3e-7 / 5.4e-7 / 7.0e-7   2.2e-7 / 4.2e-7 / 1.0e-6   1.9e-7 / 5.1e-6 / 5.8e-6
    invert_step         4.6e-8 / 0.12 of bound     4.7e-8 / 0.14 of bound     5.8e-8 / 0.13 of bound     5.9e-8 / 0.06 of bound
    resample_jump       2.6e-7 / 4.2e-7            2.1e-7 / 3.5e-7            2.0e-7 / 3.5e-7            2.3e-7 / 1.2e-7     (positions: 1e-6)
    jump, tied          2.6e-7 / 3.5e-7            2.1e-7 / 3.5e-7            2.0e-7 / 3.5e-7            2.3e-7 / 1.1e-7
    corrector_step      3.8e-7, masked 1.2e-7      2.2e-7, masked 2.2e-7      2.4e-7, masked 2.2e-7      3.1e-7, masked 3.2e-7

P1 against the scheduled step: positions differ by 0 on all four models.  One conditioned step (S12, S124): positions 6.0e-8 (0.6 % of
their bound), lengths 1.4e-6 of 7.6, cell 1.4e-6, replaced positions 6.0e-8 (bound 1e-6), no class differs.  The smallest float64
margins are printed by test_sampling_corners_cpu.py (between 1.1e-3, S124 reverse, and 0.12).

What the module sees, measured once with two deliberately wrong builds of the library (never committed; both only read other
in-range entries).  reverse_one_atom's crystal search cut to its first level (right up to 64 crystals): the 64 restatement tests of
the respaced, eta, lattice-system, inversion and resampling modules pass; here all 28 reverse-step cases and the 4 P1 cases fail.
The TIE instance's `lead` taken from lanes 0-31 (right for crystals 0-7 of a wave): the same 64 pass; here the 12 tied step cases
and the no-prep S12 eta loop fail."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from arreau_amd import _hip
from arreau_amd.diffusion import inversion as iv
from arreau_amd.diffusion import resampling as rs
from arreau_amd.diffusion import respacing
from oracle import geometry as OG
from oracle import sampler as OS
from tests import sampling_corner_cases as C
from tests.helpers import oracle_from_module, random_state
from tests.sampling_helpers import assert_same_bits, dev  # noqa: F401

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the project's bound for an fp32 step against its float64 restatement
CLIP, SNR, B, N = C.CLIP, C.SNR, C.B, C.N


_BUILT = {}


def _model(dev, name):
    """(name, S, module on the device, oracle model) of a model of the cases, built once."""
    if name not in _BUILT:
        from arreau_amd.checkpoint import make_synthetic_model
        m = make_synthetic_model(seed=C.MODEL_SEED, **C.MODELS[name]).to(dev)
        _BUILT[name] = (name, C.MODELS[name]["S"], m, oracle_from_module(m, torch.float32))
    return _BUILT[name]


@pytest.fixture(scope="module", params=sorted(C.MODELS))
def corner_model(dev, request):
    return _model(dev, request.param)


@pytest.fixture(scope="module", params=["S12", "S124"])
def loop_model(dev, request):
    return _model(dev, request.param)


def _set_loop_form(monkeypatch, loop_prep):
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev).contiguous()


def _offsets(dev):
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    return crystal_offsets(torch.tensor(C.COUNTS), dev)


def _on_device(v, dev):
    """A namespace of the inputs' tensors on the device, with the offsets and a factory of fresh states (x_t as the species)."""
    d = lambda a: a.to(dev).contiguous()
    w = SimpleNamespace(**{k: d(getattr(v, k)) for k in ("eps", "logits", "len0", "z_l", "z_f", "u")}, an=d(v.angles), off=_offsets(dev))
    w.fresh = lambda: (d(v.frac.clone()), d(v.x_t.to(torch.int32)), d(v.lengths.clone()), torch.zeros(B, 3, 3, device=dev))
    return w


def _rows(b):
    return slice(int(C.FIRST[b]), int(C.FIRST[b + 1]))


def assert_tied(lengths, what):
    """Tied axes bitwise equal: a = b for code 1, a = b = c for code 2."""
    le = lengths.detach().cpu()
    for b, code in enumerate(C.CODES):
        if code > 0:
            assert torch.equal(le[b, :code + 1], le[b, :1].expand(code + 1)), (what, b, le[b])


def _assert_crystals_equal_constant_launches(model, kind, got, launch, what):
    """Blind spot 1, bitwise: the launch with per-crystal pairs against one launch per distinct pair with that pair for every
    crystal -- the rows of the crystals that hold the pair are the same bits."""
    idx = C.pair_index(model, kind)
    for p, pair in enumerate(C.pair_list(model, kind)):
        if C.pair_list(model, kind).index(pair) != p:
            continue
        const = launch(np.full(B, pair[0]), np.full(B, pair[1]))
        for b in np.flatnonzero([C.pair_list(model, kind)[i] == pair for i in idx]):
            rows = _rows(b)
            for g, c in zip(got, const):
                part = (lambda x: x[rows]) if g.shape[0] == N else (lambda x: x[b:b + 1])
                assert_same_bits((part(g),), (part(c),), (what, "crystal", int(b), "pair", pair))


# -------------------------------------------------------------------------------------------------------------- 1
VARIANTS = {  # id -> (kind of pairs, restatement variant, eta, tied)
    "plain": ("plain", "plain", None, False), "to": ("reverse", "sched", None, False), "tied": ("reverse", "sched", None, True),
    "eta0": ("reverse", "eta", 0.0, False), "eta0.5": ("reverse", "eta", 0.5, False),
    "eta0-tied": ("reverse", "eta", 0.0, True), "eta0.5-tied": ("reverse", "eta", 0.5, True)}


def _reverse_launch(eng, w, dev, variant, t, s, tie=None, sym=None):
    """One launch of a reverse entry point with the per-crystal arrays t, s; returns the new (frac, types, lengths, lattice)."""
    _, _, eta, _ = VARIANTS[variant]
    f, ty, le, lat = w.fresh()
    t_c, s_c = _i32(t, dev), _i32(s, dev)
    noise = (w.z_l, w.z_f, w.u)
    if sym is not None:
        eng.reverse_step_sym(f, ty, le, w.an, t_c, s_c, w.off, w.eps, w.logits, w.len0, *noise, lat, tie, sym, CLIP)
    elif variant == "plain":
        eng.reverse_step(f, ty, le, w.an, t_c, w.off, w.eps, w.logits, w.len0, *noise, lat)
    elif eta is not None:
        eng.reverse_step_eta(f, ty, le, w.an, t_c, s_c, w.off, w.eps, w.logits, w.len0, *noise, lat, eta, tie, CLIP)
    elif tie is not None:
        eng.reverse_step_tied(f, ty, le, w.an, t_c, s_c, w.off, w.eps, w.logits, w.len0, *noise, lat, tie, CLIP)
    else:
        eng.reverse_step_to(f, ty, le, w.an, t_c, s_c, w.off, w.eps, w.logits, w.len0, *noise, lat, CLIP)
    return f, ty, le, lat


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_reverse_steps_with_a_pair_per_crystal(dev, corner_model, variant):
    """arreau_reverse_step / _to / _tied / _eta (plain, SCHED, SCHED+TIE, ETA, ETA+TIE instances), one launch on the 67-crystal batch.
    Blind spot 1 (every crystal of every step test held the same (t, s)): each crystal holds its own pair, and positions and
    classes are compared with the float64 restatement at that crystal's pair -- a wrong crystal index from the 64-ary search
    gives another sigma, Qbar row or t == 1 branch, which test_sampling_corners_cpu.py shows the comparison sees; the launch is
    also bitwise the constant-pair launches, crystal by crystal.
    Blind spot 2 (B <= 6): lengths, cells and exact ties of all 67 crystals -- waves 1-3 and the second workgroup of the lattice
    part, the shuffles of the TIE instances past lane 23, the partly live last group of four.
    Blind spot 3 (S = 12): at S = 124 every class equal, with changed atoms on both sides of class 64 (guarded on the CPU).
    Bounds: those of test_gpu_respaced_sampling.py / test_gpu_ddim_sampling.py (positions 1e-5 wrapped, lengths and cell 1e-5 of
    max(1, magnitude)) and, for the tied step, test_gpu_lattice_systems.py's per-crystal one; no class may differ."""
    model, S, m, om = corner_model
    eng = m.engine()
    kind, restated, eta, tied = VARIANTS[variant]
    v = C.inputs(model, kind)
    w = _on_device(v, dev)
    t, s = C.pairs_per_crystal(model, kind)
    codes = C.CODES if tied else None
    tie = _i32(C.CODES, dev) if tied else None
    eng.status(reset=True)
    f, ty, le, lat = got = _reverse_launch(eng, w, dev, variant, t, s, tie)
    ref = C.gather(C.per_pair(model, kind, lambda a, b: C.reverse_at(om, v, a, b, restated, eta, codes)), model, kind)
    cell = C.cell_of(ref["lengths"], v.angles)
    e_f = float(C.wrapped(f.cpu().numpy(), ref["frac"]).max())
    e_l = np.abs(le.cpu().double().numpy() - ref["lengths"])
    e_c = float(np.abs(lat.cpu().double().numpy() - cell).max())
    wrong = int((ty.cpu().numpy() != ref["types"]).sum())
    print(f"{model} {variant}: frac {e_f:.3g} (bound {TOL:g})  lengths {e_l.max():.3g} of {np.abs(ref['lengths']).max():.3g}  "
          f"cell {e_c:.3g} of {np.abs(cell).max():.3g}  classes that differ {wrong}  smallest float64 margin {ref['margin'].min():.3g}")
    assert e_f <= TOL
    if variant == "tied":
        x0 = v.len0.double().numpy() * np.asarray(C.COUNTS)[:, None]
        scale = np.maximum(1.0, np.abs(np.concatenate([ref["lengths"], v.lengths.double().numpy(), x0], axis=1)).max(axis=1, keepdims=True))
        assert np.all(e_l <= TOL * scale)
    else:
        assert e_l.max() <= TOL * max(1.0, float(np.abs(ref["lengths"]).max()))
    assert e_c <= TOL * max(1.0, float(np.abs(cell).max()))
    assert ref["margin"].min() >= C.MARGIN and wrong == 0
    eng.check_status()
    _assert_crystals_equal_constant_launches(model, kind, got, lambda a, b: _reverse_launch(eng, w, dev, variant, a, b, tie), variant)
    if tied:  # code-0 crystals, and positions and species of every crystal, are the untied step's
        assert_tied(le, variant)
        free = _reverse_launch(eng, w, dev, variant, t, s, None)
        assert_same_bits((f, ty), free[:2], "positions and species are the untied step's")
        for b, code in enumerate(C.CODES):
            if code == 0:
                assert_same_bits((le[b], lat[b]), (free[2][b], free[3][b]), f"code-0 crystal {b}")
        assert not torch.equal(le, free[2])
    if variant == "plain":  # s = t - 1 through the scheduled entry point: the same bits
        assert_same_bits(got, _reverse_launch(eng, w, dev, "to", t, s), "arreau_reverse_step_to at stride 1")
    eng.check_status()


def test_p1_symmetric_step_is_the_scheduled_step(dev, corner_model):
    """The argument of test_gpu_symmetry.py::test_p1_spec_is_the_plain_step at 67 crystals with a pair per crystal: with a P1
    table (orbits of one atom) arreau_reverse_step_sym gives the species and cells of arreau_reverse_step_to bit for bit, and
    its positions within 2^-22 wrapped (the same fp32 expression in two inlined copies).  Blind spots 1 and 3: d3pm_reverse_class
    and sym_atom_crystal are separate copies of the species half and the crystal search; this pins them to reverse_one_atom's at
    mixed pairs and S = 124."""
    from arreau_amd.diffusion import symmetry as sy
    from tests.symmetry_cases import GENS
    model, S, m, om = corner_model
    eng = m.engine()
    v = C.inputs(model, "reverse")
    w = _on_device(v, dev)
    t, s = C.pairs_per_crystal(model, "reverse")
    by_count = {n: sy.SymmetrySpec.general_positions(GENS["P1"], n, "triclinic") for n in sorted(set(C.COUNTS))}
    tables = sy.device_arrays([by_count[n] for n in C.COUNTS], w.off, dev)
    eng.status(reset=True)
    want = _reverse_launch(eng, w, dev, "to", t, s)
    got = _reverse_launch(eng, w, dev, "to", t, s, None, tables)
    assert_same_bits(got[1:], want[1:], "P1: species and cells")
    err = float(C.wrapped(got[0].cpu().numpy(), want[0].cpu().numpy()).max())
    print(f"{model}: P1 against the scheduled step, largest wrapped difference {err:.3g}")
    assert err <= 2.0 ** -22
    assert not torch.equal(want[0], w.fresh()[0]) and not torch.equal(want[1], w.fresh()[1])
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("held", [False, True], ids=["free", "fixed-lengths"])
def test_invert_step_with_a_climb_per_crystal(dev, corner_model, held):
    """arreau_invert_step (the INVERT instance; its atom part is invert_atoms_body through sym_atom_crystal), every crystal on its
    own climb s -> t.  Blind spots 1 and 2 as in the reverse steps: positions against inversion.invert_positions at the crystal's
    own pair (1e-5 wrapped), lengths against invert_lengths within the derived length_error_bound, the cell within 1e-5, for all
    67 crystals; bitwise the constant-pair launches; species untouched; fixed lengths held bitwise with the free positions."""
    model, S, m, om = corner_model
    eng = m.engine()
    v = C.inputs(model, "invert")
    w = _on_device(v, dev)
    s, t = C.pairs_per_crystal(model, "invert")
    fixed = v.lengths.to(dev).contiguous() if held else None

    def launch(a, b):
        f, ty, le, lat = w.fresh()
        eng.invert_step(f, ty, le, w.an, _i32(a, dev), _i32(b, dev), w.off, w.eps, w.len0, lat, fixed_lengths=fixed)
        return f, ty, le, lat

    eng.status(reset=True)
    f, ty, le, lat = got = launch(s, t)
    ref = C.gather(C.per_pair(model, "invert", lambda a, b: C.invert_at(om, v, a, b)), model, "invert")
    e_f = float(C.wrapped(f.cpu().numpy(), ref["frac"]).max())
    assert e_f <= TOL
    assert_same_bits((ty,), (w.fresh()[1],), "the species were written")
    assert bool(((f >= 0) & (f <= 1)).all())
    if held:
        assert_same_bits((le,), (fixed,), "fixed lengths")
        want_l = v.lengths.double().numpy()
        print(f"{model} invert, fixed lengths: frac {e_f:.3g} (bound {TOL:g})")
    else:
        want_l = ref["lengths"]
        e_l = np.abs(le.cpu().double().numpy() - want_l)
        print(f"{model} invert: frac {e_f:.3g} (bound {TOL:g})  lengths {e_l.max():.3g}, largest share of its bound "
              f"{(e_l / ref['bound']).max():.3g} (bounds {ref['bound'].min():.3g} .. {ref['bound'].max():.3g})")
        assert (e_l <= ref["bound"]).all()
    cell = C.cell_of(want_l, v.angles)
    assert float(np.abs(lat.cpu().double().numpy() - cell).max()) <= TOL * max(1.0, float(np.abs(cell).max()))
    _assert_crystals_equal_constant_launches(model, "invert", got, launch, "invert")
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_jump_with_a_pair_per_crystal(dev, corner_model, tied):
    """arreau_resample_jump(_tied) (jump<false / true>), every crystal on its own jump s -> t, s = 0 included.  Blind spot 1: the
    jump kernel's own copy of the crystal search -- positions (1e-6 wrapped) and classes (equal) against resampling.jump at the
    crystal's pair, bitwise the constant-pair launches.  Blind spot 3: at S = 124 the class loop's second trip and its
    cross-lane first-index rule.  Blind spot 2: lengths of 67 crystals (test_gpu_resampled_sampling.py's allclose; tied:
    lattice_systems.tied_jump within 1e-5 of max(1, |l|), exact ties, code-0 crystals and all positions and species the untied
    jump's)."""
    from tests.test_gpu_resampled_sampling import _cell
    model, S, m, om = corner_model
    eng = m.engine()
    v = C.inputs(model, "jump")
    w = _on_device(v, dev)
    s, t = C.pairs_per_crystal(model, "jump")
    tie = _i32(C.CODES, dev) if tied else None

    def launch(a, b, tie=tie):
        f, ty, le, lat = w.fresh()
        eng.resample_jump(f, ty, le, w.an, _i32(a, dev), _i32(b, dev), w.off, w.z_f, w.z_l, w.u, lat, length_tie=tie)
        return f, ty, le, lat

    eng.status(reset=True)
    f, ty, le, lat = got = launch(s, t)
    eng.check_status()
    ref = C.gather(C.per_pair(model, "jump", lambda a, b: C.jump_at(om, v, a, b, C.CODES if tied else None)), model, "jump")
    e_f = float(C.wrapped(f.cpu().numpy(), ref["frac"]).max())
    got_l = le.cpu().double().numpy()
    wrong = int((ty.cpu().numpy() != ref["types"]).sum())
    print(f"{model} jump tied={tied}: frac {e_f:.3g} (bound 1e-06)  lengths {np.abs(got_l - ref['lengths']).max():.3g} of "
          f"{np.abs(ref['lengths']).max():.3g}  classes that differ {wrong}  smallest float64 margin {ref['margin'].min():.3g}")
    assert e_f <= 1e-6
    if tied:
        assert np.all(np.abs(got_l - ref["lengths"]) <= TOL * np.maximum(1.0, np.abs(ref["lengths"])))
        assert_tied(le, "jump")
    else:
        assert np.allclose(got_l, ref["lengths"], rtol=1e-5, atol=1e-6)
    assert ref["margin"].min() >= C.MARGIN and wrong == 0
    assert torch.allclose(lat, _cell(le, w.an), rtol=1e-6, atol=1e-6)
    assert bool(((f >= 0) & (f <= 1)).all())
    _assert_crystals_equal_constant_launches(model, "jump", got, launch, ("jump", tied))
    if tied:
        free = launch(s, t, None)
        assert_same_bits((f, ty), free[:2], "positions and species are the untied jump's")
        for b, code in enumerate(C.CODES):
            if code == 0:
                assert_same_bits((le[b], lat[b]), (free[2][b], free[3][b]), f"code-0 crystal {b}")
        assert not torch.equal(le, free[2])
    eng.check_status()


def test_noise_state_is_the_jump_from_zero(dev, corner_model):
    """arreau_noise_state on the 67-crystal batch against arreau_resample_jump (0 -> t) on arreau_philox_fill_word's draws of kinds
    6 / 7 / 8: bit for bit, free and with the lattice-system tie (the jump itself is pinned to its restatement above)."""
    model, S, m, om = corner_model
    eng = m.engine()
    v = C.inputs(model, "jump")
    w = _on_device(v, dev)
    t, seed = (50 if C.MODELS[model]["num_timesteps"] > 2 else 2), 2718281828
    z_f = eng.philox_fill_word(seed, t, 6, 0, 3 * N).view(N, 3)
    z_l = eng.philox_fill_word(seed, t, 7, 0, 3 * B).view(B, 3)
    u_t = eng.philox_fill_word(seed, t, 8, 0, N * S).view(N, S)
    eng.status(reset=True)
    for tie in (None, _i32(C.CODES, dev)):
        got, want = w.fresh(), w.fresh()
        eng.noise_state(*got[:3], w.an, w.off, t, seed, got[3], length_tie=tie)
        eng.resample_jump(*want[:3], w.an, _i32(np.zeros(B), dev), _i32(np.full(B, t), dev), w.off, z_f, z_l, u_t, want[3], length_tie=tie)
        assert_same_bits(got, want, ("noise_state", tie is not None))
        assert not torch.equal(got[0], w.fresh()[0]) and not torch.equal(got[2], w.fresh()[2])
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("masked", [False, True], ids=["all-free", "masked"])
def test_corrector_step_with_a_timestep_per_crystal(dev, corner_model, masked):
    """arreau_corrector_step (corrector<false / true>) with every crystal at its own timestep.  Blind spots 1 and 2: the move of
    each of the 67 crystals against corrector.corrector_move at the crystal's own sigma (1e-5 wrapped) and bitwise the
    constant-timestep launches; known positions (40 % of the atoms, all of crystal 64) and the zero-eps crystal 65 unmoved."""
    model, S, m, om = corner_model
    eng = m.engine()
    v = C.inputs(model, "corrector")
    w = _on_device(v, dev)
    t, _ = C.pairs_per_crystal(model, "corrector")
    cond = None
    if masked:
        x0 = torch.where(v.known[:, None], v.frac, torch.zeros_like(v.frac))
        cond = {"x0": x0.to(dev).contiguous(), "pos_mask": v.known.to(torch.uint8).to(dev).contiguous()}

    def launch(a, _):
        f = w.fresh()[0]
        eng.corrector_step(f, _i32(a, dev), w.off, w.eps, w.z_f, SNR, condition=cond)
        return (f,)

    eng.status(reset=True)
    got = launch(t, t)[0].cpu()
    ref = C.gather(C.per_pair(model, "corrector", lambda a, _: C.corrector_at(om, v, a, masked)), model, "corrector")
    e_f = float(C.wrapped(got.numpy(), ref["frac"]).max())
    print(f"{model} corrector masked={masked}: frac {e_f:.3g} (bound {TOL:g})")
    assert e_f <= TOL
    unmoved = torch.as_tensor(C.CRYSTAL == 65)
    if masked:
        unmoved = unmoved | v.known
    assert torch.equal(got[unmoved], v.frac[unmoved])
    assert not torch.equal(got[~unmoved], v.frac[~unmoved])
    assert bool(((got >= 0) & (got <= 1)).all())
    _assert_crystals_equal_constant_launches(model, "corrector", (got.to(dev),), launch, ("corrector", masked))
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 5
class LoopCase:
    """The 67-crystal batch as a loop's start: physical cells (4-8 A, angles in radians), positions in the cell, every third
    atom on the mask class."""

    def __init__(self, dev, S, seed):
        self.frac, self.types, self.lengths, self.angles, self.na = random_state(S, C.COUNTS, seed, sampler_like=False)
        self.dev, self.S, self.off = dev, S, _offsets(dev)
        self.an = self.angles.to(dev).contiguous()

    def fresh(self):
        d = lambda a: a.to(self.dev).contiguous()
        return d(self.frac.clone()), d(self.types.to(torch.int32)), d(self.lengths.clone()), torch.zeros(B, 3, 3, device=self.dev)


def _full(v, dev):
    return torch.full((B,), int(v), device=dev, dtype=torch.int32)


SCHED = [99, 98, 80, 61, 40, 39, 12]  # six steps, the seventh entry their last target


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_tied_eta_loop_is_its_steps_one_by_one(dev, loop_model, loop_prep, monkeypatch):
    """A scheduled, tied eta loop of six steps on the 67-crystal batch, bitwise against predict_scores + arreau_reverse_step_eta on
    arreau_philox_fill's draws (the replay of test_gpu_ddim_sampling.py::test_eta_loop_is_its_steps_one_by_one).  Blind spot 2:
    with ARREAU_LOOP_PREP=1 the loop runs reverse_lattice_body's ETA+TIE instance on 67 crystals; without it the per-crystal
    workgroups.  The loop hands the kernel batch[i] where the step searches the offsets, so blind spot 1's search is checked
    against an independent crystal index on every atom; S = 124 for blind spot 3."""
    _set_loop_form(monkeypatch, loop_prep)
    model, S, m, _ = loop_model
    eng = m.engine()
    case, seed, eta = LoopCase(dev, S, 17), 1122334455, 0.5
    tie = _i32(C.CODES, dev)
    nxt = respacing.next_table(C.T, SCHED).to(dev)
    eng.status(reset=True)
    f, ty, le, lat = case.fresh()
    for t, s in zip(SCHED[:-1], SCHED[1:]):
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, _full(t, dev), case.off)
        eng.reverse_step_eta(f, ty, le, case.an, _full(t, dev), _full(s, dev), case.off, eps, logits, len0,
                             eng.philox_fill(seed, t, 0, 3 * B).view(B, 3), eng.philox_fill(seed, t, 1, 3 * N).view(N, 3),
                             eng.philox_fill(seed, t, 2, N * S).view(N, S), lat, eta, tie, CLIP)
    for use_graph in (False, True):
        got = case.fresh()
        eng.sample_loop(*got[:3], case.an, case.off, SCHED[0], len(SCHED) - 1, seed, None, got[3], use_graph=use_graph, next_table=nxt,
                        lattice_clipmax=CLIP, eta=eta, length_tie=tie)
        assert_same_bits(got, (f, ty, le, lat), ("eta loop", model, use_graph))
    assert_tied(le, "loop")
    assert not torch.equal(ty, case.fresh()[1]) and not torch.equal(le, case.fresh()[2])
    eng.check_status()


LEVELS = [1, 3, 10, 50, 99]  # four climbs


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_invert_loop_is_its_steps_one_by_one(dev, loop_model, loop_prep, monkeypatch):
    """An inversion loop of four levels on the 67-crystal batch, bitwise against predict_scores + arreau_invert_step level by level
    (the replay of test_gpu_inversion.py::test_invert_loop_is_its_steps_one_by_one), free cells and fixed ones (an untrained
    network's x0 of a 130-atom cell is far from any cell; the fixed run keeps the network's input physical over all four levels).
    Blind spots 1 and 2: the INVERT instance's lattice part in both loop forms on 67 crystals, and invert_atoms_body's crystal
    search against the loop's batch[i]."""
    _set_loop_form(monkeypatch, loop_prep)
    model, S, m, _ = loop_model
    eng = m.engine()
    case = LoopCase(dev, S, 19)
    up = torch.as_tensor(iv.ascending_table(C.T, LEVELS)).to(dev)
    eng.status(reset=True)
    for fixed in (case.fresh()[2], None):
        f, ty, le, lat = case.fresh()
        for s, t in zip(LEVELS, LEVELS[1:]):
            eps, _, len0 = eng.predict_scores(f, ty, le, case.an, _full(s, dev), case.off)
            eng.invert_step(f, ty, le, case.an, _full(s, dev), _full(t, dev), case.off, eps, len0, lat, fixed_lengths=fixed)
        for use_graph in (False, True):
            got = case.fresh()
            eng.invert_loop(*got[:3], case.an, case.off, LEVELS[0], len(LEVELS) - 1, up, got[3], use_graph=use_graph, fixed_lengths=fixed)
            assert_same_bits(got, (f, ty, le, lat), ("invert loop", model, use_graph, fixed is not None), nan_ok=fixed is None)
        assert not torch.equal(f, case.fresh()[0])
        if fixed is not None:
            assert_same_bits((le,), (fixed,), "fixed lengths")
            eng.check_status()
    assert not eng.status(reset=True)["flags"] & (_hip.STATUS_BAD_TIMESTEP | _hip.STATUS_BAD_TYPE)


def _loop_condition(case, seed=4):
    """Masks that alternate over the crystals: positions known on 60 % of the atoms of the even crystals, species on every third
    crystal, the lengths of the even crystals (64 and the 130-atom crystal 66 among them: its cell is held to the template)."""
    rng = np.random.RandomState(seed)
    pm = (C.CRYSTAL % 2 == 0) & (rng.rand(N) < 0.6)
    tm = C.CRYSTAL % 3 == 0
    lm = np.arange(B) % 2 == 0
    assert pm[C.CRYSTAL >= 64].any() and tm[C.CRYSTAL >= 64].any() and lm[64:].any() and not lm[65]
    host = SimpleNamespace(N=N, B=B, pm=pm, tm=tm, lm=lm, x0=rng.uniform(-0.5, 1.5, (N, 3)).astype(np.float32) * pm[:, None],
                           a0=rng.randint(0, case.S - 1, N).astype(np.int32), l0=rng.uniform(4, 8, (B, 3)).astype(np.float32))
    d = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=case.dev, dtype=dt).contiguous()
    cond = dict(x0=d(host.x0, torch.float32), pos_mask=d(pm.astype(np.uint8), torch.uint8), a0=d(host.a0, torch.int32),
                type_mask=d(tm.astype(np.uint8), torch.uint8), l0=d(host.l0, torch.float32), len_mask=d(lm.astype(np.uint8), torch.uint8))
    return host, cond


def _events_one_by_one(eng, case, seed, steps, succ, R, J, cond, om, state):
    """resampling.plan at stride 1, run with predict_scores / reverse_step / resample_jump on philox_fill_word's draws and the
    replacement rules restated on the host (test_gpu_resampled_sampling.py's replay, for any number of classes)."""
    from tests.test_gpu_resampled_sampling import _replace
    S, dev = case.S, case.dev
    f, ty, le, lat = state
    for ev in rs.plan(steps, succ, R, J):
        if ev.kind == "jump":
            eng.resample_jump(f, ty, le, case.an, _full(ev.s, dev), _full(ev.t, dev), case.off,
                              eng.philox_fill_word(seed, ev.t, 6, ev.r, 3 * N).view(N, 3), eng.philox_fill_word(seed, ev.t, 7, ev.r, 3 * B).view(B, 3),
                              eng.philox_fill_word(seed, ev.t, 8, ev.r, N * S).view(N, S), lat, condition=cond)
            continue
        t, w3 = ev.t, 256 * ev.r
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, _full(t, dev), case.off)
        eng.reverse_step(f, ty, le, case.an, _full(t, dev), case.off, eps, logits, len0, eng.philox_fill_word(seed, t, 0, w3, 3 * B).view(B, 3),
                         eng.philox_fill_word(seed, t, 1, w3, 3 * N).view(N, 3), eng.philox_fill_word(seed, t, 2, w3, N * S).view(N, S), lat)
        _replace(eng, om, cond, seed, t, ev.s, ev.r, f, ty, le, case.an, lat)
    return f, ty, le, lat


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_conditioned_resampled_loop_is_its_events(dev, loop_model, loop_prep, monkeypatch):
    """A conditioned resampled loop (2 passes, jump length 2, 4 steps) on the 67-crystal batch, block by block bitwise against its
    events with the replacement rules restated on the host (test_gpu_resampled_sampling.py::
    test_conditioned_resampled_loop_is_its_events).  Blind spot 2: the COND+RESAMPLE instances' lattice part and the jump on 67
    crystals with masks that alternate over the crystals, crystals 64 and 66 among the known ones; S = 124 for blind spot 3."""
    _set_loop_form(monkeypatch, loop_prep)
    model, S, m, om = loop_model
    eng = m.engine()
    case, seed, R, J = LoopCase(dev, S, 43), 31415, 2, 2
    host, cond = _loop_condition(case)
    steps = [60, 59, 58, 57]
    pm, tm, lm = (torch.as_tensor(a).to(dev) for a in (host.pm, host.tm, host.lm))
    loop = case.fresh()
    eng.status(reset=True)
    eng.condition_initial_state(*loop[:3], steps[0], seed, cond)
    for lo in range(0, len(steps), J):
        start = tuple(x.clone() for x in loop)
        eng.sample_loop(*loop[:3], case.an, case.off, steps[lo], J, seed, None, loop[3], use_graph=True, condition=cond, resampling=(R, J))
        f, ty, le, lat = _events_one_by_one(eng, case, seed, steps[lo:lo + J], steps[lo] - J, R, J, cond, om, tuple(x.clone() for x in start))
        assert torch.equal(loop[1][tm], cond["a0"][tm]), steps[lo]
        assert_same_bits(loop[:3], (f, ty, le), (model, steps[lo]))
        assert torch.allclose(loop[3], lat, rtol=1e-6, atol=1e-6), steps[lo]  # (the cell: another kernel's evaluation of it)
        assert not torch.equal(loop[0], start[0]) and not torch.equal(loop[2][~lm], start[2][~lm])
    assert not eng.status(reset=True)["flags"] & (_hip.STATUS_BAD_TIMESTEP | _hip.STATUS_BAD_TYPE)


def test_one_conditioned_step_in_value(dev, loop_model):
    """sample_loop(..., 1, condition=cond) on the 67-crystal batch against the float64 step and replacement rules of
    test_gpu_conditioned_sampling.py::test_conditioned_steps_against_a_cpu_restatement, with its bounds, on the device's own
    predict_scores and arreau_philox_fill's draws: the loop's COND instance in value, where the bitwise tests above compare it
    with other launches."""
    from tests.test_gpu_conditioned_sampling import _rules_cpu
    model, S, m, om = loop_model
    eng = m.engine()
    case, seed, t = LoopCase(dev, S, 47), 1357911, 60
    host, cond = _loop_condition(case)
    f, ty, le, lat = case.fresh()
    eng.status(reset=True)
    eng.condition_initial_state(f, ty, le, t, seed, cond)
    frac, types, lengths = f.cpu(), ty.cpu().long(), le.cpu()
    scores = tuple(x.cpu() for x in eng.predict_scores(f, ty, le, case.an, _full(t, dev), case.off))
    noise = OS.StepNoise(*(eng.philox_fill(seed, t, k, n).view(*shp).cpu() for k, n, shp in ((0, 3 * B, (B, 3)), (1, 3 * N, (N, 3)), (2, N * S, (N, S)))))
    d = lambda a: a.double()
    f_o, ty_o, le_o, _ = OS.reverse_step(C.in_float64(om), d(frac), types, d(lengths), d(case.angles), case.na, tuple(d(a) for a in scores), t,
                                         OS.StepNoise(*(d(a) for a in (noise.z_lattice, noise.z_frac, noise.u_types))))
    host64 = SimpleNamespace(**{**vars(host), "x0": host.x0.astype(np.float64), "l0": host.l0.astype(np.float64)})  # (the rules in float64 too)
    f_o, ty_o, le_o = _rules_cpu(om, eng, seed, t, host64, f_o, ty_o, le_o)
    lat_o = OG.lattice_from_params(le_o, d(case.angles))
    eng.sample_loop(f, ty, le, case.an, case.off, t, 1, seed, None, lat, condition=cond)
    s2, sp2 = float(om.ve_sigmas[t]) ** 2, float(om.ve_sigmas[t - 1]) ** 2
    pre = d(frac) - d(scores[0]) * (s2 - sp2)
    bound = TOL * pre.abs().clamp(min=1.0) + TOL * max(1.0, float(scores[0].abs().max())) * (s2 - sp2)
    dd = torch.as_tensor(C.wrapped(f.cpu().numpy(), f_o.numpy()))
    e_l, e_c = float((d(le.cpu()) - le_o).abs().max()), float((d(lat.cpu()) - lat_o).abs().max())
    pm, tm = torch.as_tensor(host.pm), torch.as_tensor(host.tm)
    wrong = int((ty.cpu().long() != ty_o).sum())
    print(f"{model} conditioned step: frac {float(dd.max()):.3g} (largest share of its bound {float((dd / bound).max()):.3g})  lengths {e_l:.3g} "
          f"of {float(le_o.abs().max()):.3g}  cell {e_c:.3g}  replaced positions {float(dd[pm].max()):.3g} (bound 1e-06)  classes that differ {wrong}")
    assert (dd <= bound).all()
    assert e_l <= TOL * max(1.0, float(le_o.abs().max())) and e_c <= TOL * max(1.0, float(lat_o.abs().max()))
    assert float(dd[pm].max()) <= 1e-6
    assert torch.equal(ty.cpu().long()[tm], ty_o[tm])
    assert wrong <= 1  # the network's own logits: a Gumbel arg-max within rounding of a tie may go either way
    eng.check_status()


# -------------------------------------------------------------------------------------------------------------- 6
def _key_rows(case, dev):
    """name -> (options A, options B, poison, check): a replay call with A, then poison() (what a stale replay would read or write
    is changed under it), then a replay call with B on the same buffers; check() after it.  Only the named option differs."""
    from arreau_amd.diffusion import contact_guidance as cg
    from arreau_amd.diffusion import keyed
    from arreau_amd.diffusion import species as sp
    nothing = lambda: None
    allowed = np.ones((B, case.S), dtype=bool)
    allowed[::2, 5:] = False  # the even crystals: classes 0..4 only
    rows_a, rows_b = sp.device_rows(allowed, dev), sp.device_rows(allowed, dev)
    seeds = torch.from_numpy(keyed.stream_seeds(99, np.arange(B)).view(np.int64).copy())
    seeds_a, seeds_b = seeds.to(dev).contiguous(), seeds.to(dev).contiguous()
    tie_a, tie_b = _i32(C.CODES, dev), _i32(C.CODES, dev)
    guide, info = cg.ContactGuidance(min_distance=2.0, weight=0.3), cg.allocate_info(B, dev)
    sched = dict(t_start=99, next_table=respacing.next_table(C.T, [99, 80, 61, 40]).to(dev))

    def clear_info():
        assert any(bool(info[q].any()) for q in cg.INFO_KEYS), "the guided run wrote no diagnostics: the row would see nothing"
        for q in cg.INFO_KEYS:
            info[q].zero_()

    def info_untouched():
        assert not any(bool(info[q].any()) for q in cg.INFO_KEYS), "a replay wrote the diagnostics of a call that named none"

    return {
        "lattice_clipmax": (dict(sched, lattice_clipmax=0.999), dict(sched, lattice_clipmax=0.05), nothing, nothing),
        "species-rows-pointer": (dict(species=(rows_a, 1.0)), dict(species=(rows_b, 1.0)), lambda: rows_a.fill_(-1), nothing),
        "crystal-seeds-pointer": (dict(crystal_seeds=seeds_a), dict(crystal_seeds=seeds_b), lambda: seeds_a.add_(1), nothing),
        "tie-pointer": (dict(length_tie=tie_a), dict(length_tie=tie_b), lambda: tie_a.zero_(), nothing),
        "guidance-info-absent": (dict(guidance=(guide, info)), dict(guidance=guide), clear_info, info_untouched),
    }


KEY_ROWS = ["lattice_clipmax", "species-rows-pointer", "crystal-seeds-pointer", "tie-pointer", "guidance-info-absent"]


@pytest.mark.parametrize("row", KEY_ROWS)
def test_graph_key_holds_every_option(dev, row):
    """The contract of the graph key (internal.h: SampleGraphKey holds the call's SampleOptions whole): a replay loop with option
    value A, the state restored into the same buffers, a replay loop with value B -- the result is the eager loop's with B bit for
    bit, so the graph captured for A was not replayed.  Three steps per call (the fewest that replay), the 67-crystal batch, S12.
    A value row also shows that A and B give different states; a pointer row (two tables of the same contents) overwrites table A
    before the second call, so a stale replay would read other values, and shows that the overwritten table gives another state;
    the info row shows the first call wrote the diagnostics and the second, which names none, left them alone.
    The rows other tests hold already, in the same form: eta 0.0 -> 0.5 and none (test_gpu_ddim_sampling.py::
    test_eta_loop_without_a_schedule_and_another_eta_is_captured_anew), the corrector's snr and its steps 1 -> 2
    (test_gpu_corrector_sampling.py::test_changed_corrector_never_replays_a_stale_graph), the species temperature
    (test_gpu_species_sampling.py, "another temperature, other rows on the same buffers"), the guidance's weight, its min_distance
    and another set of info arrays (test_gpu_contact_guidance.py::test_another_weight_on_the_same_buffers_is_not_a_stale_replay),
    the resampling's passes and jump length (test_gpu_resampled_sampling.py::test_changed_resampling_never_replays_a_stale_graph),
    the multistep history pointers (test_gpu_multistep_sampling.py::test_loop_without_a_schedule_and_the_graph_key) and the
    direction (test_gpu_inversion.py, the invert loop on a sampling loop's buffers)."""
    _, S, m, _ = _model(dev, "S12")
    eng = m.engine()
    case, seed, n = LoopCase(dev, S, 53), 24681357, 3
    opt_a, opt_b, poison, check = _key_rows(case, dev)[row]

    def run(bufs, use_graph, t_start=60, **opt):
        eng.sample_loop(*bufs[:3], case.an, case.off, t_start, n, seed, None, bufs[3], use_graph=use_graph, **opt)
        return bufs

    eng.status(reset=True)
    bufs = run(case.fresh(), True, **opt_a)
    first = tuple(x.clone() for x in bufs)
    assert_same_bits(first, run(case.fresh(), False, **opt_a), (row, "A: replay against eager"))
    poison()
    for x, x0 in zip(bufs, case.fresh()):
        x.copy_(x0)
    run(bufs, True, **opt_b)
    check()
    assert_same_bits(bufs, run(case.fresh(), False, **opt_b), (row, "B on A's buffers: replay against eager"))
    if row == "lattice_clipmax":
        assert not torch.equal(bufs[2], first[2]), "the two clips give the same lengths: the row would see nothing"
    elif row.endswith("pointer"):
        assert_same_bits(bufs, first, (row, "the same contents give the same state"))
        spoiled = run(case.fresh(), False, **opt_a)
        assert any(not torch.equal(a, b) for a, b in zip(spoiled, first)), "the overwritten table gives the same state: the row would see nothing"
    eng.check_status()


@pytest.mark.parametrize("pair", ["corrector", "guidance"])
def test_graph_key_does_not_split_an_absent_option(dev, pair):
    """What the key must not split: corrector None and (0, snr), guidance None and weight 0 are the same options (internal.h:
    SampleOptions), so on the same buffers the second call of each pair replays the graph the first one left.  The library has
    no way to observe a replay, so the assertion is equality only: both calls, and the eager loop, give the same bits."""
    from arreau_amd.diffusion import contact_guidance as cg
    _, S, m, _ = _model(dev, "S12")
    eng = m.engine()
    case, seed, n = LoopCase(dev, S, 59), 97531, 3
    absent, present = {"corrector": (dict(corrector=None), dict(corrector=(0, SNR))),
                       "guidance": (dict(species=(None, 1.0), guidance=None), dict(species=(None, 1.0), guidance=cg.ContactGuidance(2.0, 0.0)))}[pair]
    eng.status(reset=True)
    want = case.fresh()
    eng.sample_loop(*want[:3], case.an, case.off, 60, n, seed, None, want[3], use_graph=False, **absent)
    bufs = case.fresh()
    for opt in (absent, present, absent):
        for x, x0 in zip(bufs, case.fresh()):
            x.copy_(x0)
        eng.sample_loop(*bufs[:3], case.an, case.off, 60, n, seed, None, bufs[3], use_graph=True, **opt)
        assert_same_bits(bufs, want, (pair, opt))
    assert not torch.equal(want[0], case.fresh()[0])
    eng.check_status()
