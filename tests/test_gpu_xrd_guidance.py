"""XRD guidance on the GPU (rules in include/arreau_hip.h, "XRD guidance"; diffusion/xrd_guidance.py): the guidance launch against
the float64 restatement within the measured float32 bound, its distance against the xrd launch's pattern on the same state (the
walk is shared), every flag, its reproducibility, and the guided loop against evaluate, guide and step bit for bit in both loop
forms, eager and with graph replay.  The cases (tests/xrd_guidance_cases.py) reach 256 atoms in one crystal, 70 crystals, five and
sixty rounds of box entries, windows of one and of 963 grid points."""
import ctypes

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import contact_guidance as cg, inversion, xrd, xrd_guidance as xg
from arreau_amd.diffusion.lattice_helpers import lattice_from_params
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable
from tests import xrd_guidance_cases as cases
from tests.sampling_helpers import Case, S, T, assert_same_bits, dev, full_i32, fused_model, model_seed  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SEED = 20250612
SNR = 0.16
WEIGHT = 2.0
LOOP_PARAMS = xrd.XrdParams(n_points=512, fwhm=0.6)
CONTACTS = cg.ContactGuidance(min_distance=2.0, weight=0.3)

assert cases.T == T


class Batch(Case):
    COUNTS = [4, 8, 5]


def _sigmas(m):
    return m.diffusion_loss.pos_diffusion.sigmas.detach().cpu().to(torch.float32).numpy().astype(np.float64)


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _launch(eng, bt, dev, eps, t=None, weight=WEIGHT, by_class=None, target=None):
    """One launch on a copy of eps [N,3] (numpy float32) with the batch's atom weights, or (by_class = (types, table)) class
    weights: (eps', g, the info arrays) as numpy."""
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    B, N = len(bt.counts), bt.frac.shape[0]
    info = xg.allocate_info(B, dev)
    t = cases.timesteps(B) if t is None else t
    kw = dict(atom_weights=d(bt.weights)) if by_class is None else dict(class_weights=d(by_class[1]))
    types = None if by_class is None else d(np.asarray(by_class[0], dtype=np.int32))
    guide = xg.DeviceGuidance(bt.params, weight, d(bt.target if target is None else target), info=info, **kw)
    out, grad = d(eps).clone(), torch.full((N, 3), 7.0, device=dev)
    eng.xrd_guidance_step(d(bt.frac), types, d(bt.lattice), d(t), d(cases.offsets(bt)), out, guide, gradient=grad)
    return out.cpu().numpy(), grad.cpu().numpy(), xg.info_to_numpy(info)


def _distance_window(want):
    """The float32 values a float64 distance within 1e-12 of `want` may round to."""
    return np.float32(want - 1e-12), np.float32(want + 1e-12)


# ------------------------------------------------------------------------------------------- the launch against the restatement
@pytest.mark.parametrize("name", cases.BATCHES)
def test_step_matches_the_restatement(dev, fused_model, name):
    """g (d_gradient) within G_F32_BOUND of the crystal's scale, eps' within eps_bound = k (bound + 4 u |g|) + 2 u |eps'|, the
    reflections equal, no flag; d_distance is the float32 of a value within 1e-12 of xrd.distance of the pattern arreau_crystal_xrd
    returns on the same state (float64 sums of at most 4096 float32 terms in another order: the walk is shared); a second launch
    gives the same bits."""
    m, _ = fused_model
    eng = m.engine()
    bt, ref = cases.reference(name)
    B, off = len(bt.counts), cases.offsets(bt)
    sig, t = _sigmas(m), cases.timesteps(B)
    k = xg.sigma_coefficient(sig, t, WEIGHT)
    eps = np.random.RandomState(7).normal(size=bt.frac.shape).astype(np.float32)
    got, g, info = _launch(eng, bt, dev, eps)
    again, g2, info2 = _launch(eng, bt, dev, eps)
    assert _same_bytes(got, again) and _same_bytes(g, g2) and all(_same_bytes(info[q], info2[q]) for q in xg.INFO_KEYS)
    want = xg.guided_eps(eps, ref, bt.counts, sig, t, WEIGHT)
    assert not info["flags"].any() and not ref.flags.any()
    assert list(info["reflections"]) == list(ref.reflections)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    pattern = xrd.xrd(d(bt.frac), d(bt.lattice), d(off), d(bt.weights), xrd.for_weights(bt.params))["pattern"].cpu().numpy()
    for b in range(B):
        a, e = off[b], off[b + 1]
        gb = xg.g_bound(ref.g[a:e], ref.g_terms[a:e])
        g_err = np.abs(g[a:e].astype(np.float64) - ref.g[a:e]).max()
        tol = xg.eps_bound(k[b], gb, ref.g[a:e], want[a:e])
        err = np.abs(got[a:e].astype(np.float64) - want[a:e])
        lo, hi = _distance_window(xrd.distance(pattern[b], bt.target[b]))
        print(f"{name}[{b}]: n {e - a}, distance {ref.distance[b]:.6g} (device {info['distance'][b]:.9g}), largest |g| {np.abs(ref.g[a:e]).max():.3g}, "
              f"g error {g_err:.3g} of bound {gb:.3g}, eps' error / bound {np.max(err / tol):.3g}")
        assert ref.distance[b] >= xg.MIN_TEST_DISTANCE
        assert g_err <= gb and (err <= tol).all()
        assert lo <= info["distance"][b] <= hi, (b, lo, info["distance"][b], hi)
    eng.check_status()


def test_every_flag_keeps_eps(dev, fused_model):
    """One crystal per flag: NONFINITE, CELL, EMPTY, RANGE, LARGE (257 atoms), NO_TARGET (a zero row), and a range in which
    nothing scatters (DARK).  A flagged crystal keeps its eps bit for bit, its g is 0, its distance NaN, its reflections 0; the
    last crystal of the batch is guided."""
    m, _ = fused_model
    eng = m.engine()
    for bt, expected in ((cases.flags_batch(), cases.FLAGS_EXPECTED), (cases.dark_batch(), [xg.DARK])):
        off = cases.offsets(bt)
        eps = np.random.RandomState(8).normal(size=bt.frac.shape).astype(np.float32)
        got, g, info = _launch(eng, bt, dev, eps)
        ref = xg.reference(bt.frac, bt.lattice, bt.counts, bt.weights, bt.target, bt.params)
        assert list(info["flags"]) == expected == list(ref.flags)
        for b, flag in enumerate(expected):
            a, e = off[b], off[b + 1]
            if flag:
                assert _same_bytes(got[a:e], eps[a:e]) and not g[a:e].any() and np.isnan(info["distance"][b]) and info["reflections"][b] == 0
            else:
                assert not _same_bytes(got[a:e], eps[a:e]) and info["reflections"][b] == ref.reflections[b] > 0
                assert np.abs(g[a:e] - ref.g[a:e]).max() <= xg.g_bound(ref.g[a:e], ref.g_terms[a:e])
    for bad in (np.nan, np.inf, -1.0):  # a target entry that is not finite, or negative
        bt = cases.single(cases.batch("triclinic"), 0)
        row = bt.target.copy()
        row[0, 100] = bad
        eps = np.ones_like(bt.frac)
        got, g, info = _launch(eng, bt, dev, eps, target=row)
        assert list(info["flags"]) == [xg.NO_TARGET] and _same_bytes(got, eps)
    eng.check_status()


def test_a_crystal_gives_the_same_bits_wherever_it_sits_in_the_batch(dev, fused_model):
    """The first, the middle and the last crystal of the 70-crystal ragged batch launched alone (each at its own timestep) against
    their rows of the whole launch: eps', g and the three diagnostics."""
    m, _ = fused_model
    eng = m.engine()
    bt = cases.batch("ragged")
    off, t = cases.offsets(bt), cases.timesteps(len(bt.counts))
    eps = np.random.RandomState(9).normal(size=bt.frac.shape).astype(np.float32)
    got, g, info = _launch(eng, bt, dev, eps)
    for b in (0, cases.xc.RAGGED_MIDDLE, len(bt.counts) - 1):
        a, e = off[b], off[b + 1]
        alone, g_1, info_1 = _launch(eng, cases.single(bt, b), dev, eps[a:e], t=t[b:b + 1])
        assert _same_bytes(alone, got[a:e]) and _same_bytes(g_1, g[a:e]), b
        for q in xg.INFO_KEYS:
            assert info_1[q].tobytes() == info[q][b:b + 1].tobytes(), (b, q)
    assert not _same_bytes(got, eps)


def test_weight_zero_launches_and_changes_nothing(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    bt = cases.batch("textbook")
    eps = np.random.RandomState(10).normal(size=bt.frac.shape).astype(np.float32)
    got, g, info = _launch(eng, bt, dev, eps)
    zero, g0, info0 = _launch(eng, bt, dev, eps, weight=0.0)
    assert np.array_equal(zero, eps) and _same_bytes(g0, g) and all(_same_bytes(info[q], info0[q]) for q in xg.INFO_KEYS)
    assert not np.array_equal(got, eps)


def test_class_weights_are_the_atom_weights_of_the_current_classes(dev, fused_model):
    """The textbook batch with its seven elements as classes 0..6 of a 12-class table: the same bits as with the atoms' own
    amplitudes.  Then two atoms of rock salt in the mask class (weight 0) and one in a class outside the table: they get g = 0, and
    the others get what the crystal without those atoms gets, within the bound (the empty sites add zeros to every sum)."""
    m, _ = fused_model
    eng = m.engine()
    bt = cases.batch("textbook")
    zs = sorted(set(bt.species.tolist()))
    table = np.zeros(S, np.float32)
    table[:len(zs)] = zs
    types = np.array([zs.index(z) for z in bt.species.tolist()], dtype=np.int32)
    assert len(zs) < S and np.array_equal(xg.atom_weights(types, table), bt.weights)
    eps = np.random.RandomState(11).normal(size=bt.frac.shape).astype(np.float32)
    by_atom, by_class = _launch(eng, bt, dev, eps), _launch(eng, bt, dev, eps, by_class=(types, table))
    assert _same_bytes(by_atom[0], by_class[0]) and _same_bytes(by_atom[1], by_class[1])
    assert all(_same_bytes(by_atom[2][q], by_class[2][q]) for q in xg.INFO_KEYS)
    salt = cases.single(bt, 4)
    t8 = np.array([zs.index(z) for z in salt.species.tolist()], dtype=np.int32)
    t8[[1, 6]], t8[3] = S - 1, S + 5
    masked = np.isin(np.arange(8), [1, 3, 6])
    w = xg.atom_weights(t8, table)
    assert not w[masked].any() and w[~masked].all()
    _, g, info = _launch(eng, salt, dev, np.zeros_like(salt.frac), by_class=(t8, table))
    ref = xg.reference(salt.frac, salt.lattice, salt.counts, w, salt.target, salt.params)
    assert info["flags"][0] == 0 and not g[masked].any() and g[~masked].any()
    assert np.abs(g - ref.g).max() <= xg.g_bound(ref.g, ref.g_terms)
    eng.check_status()


def test_rejections_leave_eps_untouched(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    lib = _hip.lib()
    bt = cases.batch("triclinic")
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    frac, lattice, off, t, w, q = d(bt.frac), d(bt.lattice), d(cases.offsets(bt)), d(cases.timesteps(1)), d(bt.weights), d(bt.target)
    eps = torch.randn(bt.frac.shape[0], 3, device=dev)
    before = eps.clone()
    p = bt.params
    ok = (p.wavelength, p.two_theta_min, p.two_theta_max, p.fwhm, p.b_iso, p.n_points, p.max_index)
    P = lambda **kw: _hip.XrdParamsC(*[kw.get(k, v) for k, v in zip(("wavelength", "two_theta_min", "two_theta_max", "fwhm", "b_iso", "n_points", "max_index"), ok)])
    ptr = lambda x: _hip.ptr(x).value
    bad = [_hip.XrdGuidanceC(P(wavelength=0.0), 2.0, ptr(q), None, ptr(w), None, None, None),
           _hip.XrdGuidanceC(P(n_points=1), 2.0, ptr(q), None, ptr(w), None, None, None),
           _hip.XrdGuidanceC(P(fwhm=10.0), 2.0, ptr(q), None, ptr(w), None, None, None),
           _hip.XrdGuidanceC(P(max_index=128), 2.0, ptr(q), None, ptr(w), None, None, None),
           _hip.XrdGuidanceC(P(), float("nan"), ptr(q), None, ptr(w), None, None, None),
           _hip.XrdGuidanceC(P(), -1.0, ptr(q), None, ptr(w), None, None, None),
           _hip.XrdGuidanceC(P(), 2.0, None, None, ptr(w), None, None, None),
           _hip.XrdGuidanceC(P(), 2.0, ptr(q), None, None, None, None, None),
           _hip.XrdGuidanceC(P(), 2.0, ptr(q), ptr(w), ptr(w), None, None, None)]
    for g in bad:
        rc = lib.arreau_xrd_guidance_step(eng._handle, _hip.ptr(frac), None, _hip.ptr(lattice), _hip.ptr(t), _hip.ptr(off), 1, bt.frac.shape[0],
                                          _hip.ptr(eps), ctypes.byref(g), None, _hip.stream_ptr(dev))
        assert rc == -1 and b"xrd guidance" in lib.arreau_last_error()
    rc = lib.arreau_xrd_guidance_step(eng._handle, _hip.ptr(frac), None, _hip.ptr(lattice), _hip.ptr(t), _hip.ptr(off), 1, bt.frac.shape[0],
                                      _hip.ptr(eps), None, None, _hip.stream_ptr(dev))
    assert rc == -1
    # a loop takes class weights: atom weights are rejected there, before any work
    case = Batch(dev, seed=59, sampler_like=False)
    got = case.fresh()
    start = [x.clone() for x in got]
    ws = eng.workspace(case.N, case.B)
    ctl = _hip.SpeciesControlC(None, 1.0)
    rows = d(np.ones((case.B, p.n_points), np.float32))
    atoms = _hip.XrdGuidanceC(P(), 2.0, ptr(rows), None, ptr(torch.ones(case.N, device=dev)), None, None, None)
    rc = lib.arreau_sample_loop_xrd_guided(
        eng._handle, _hip.ptr(got[0]), _hip.ptr(got[1]), _hip.ptr(got[2]), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N, 30, 3, SEED,
        None, None, _hip.ptr(got[3]), _hip.ptr(ws), ws.numel(), 0, None, None, None, None, None, None, None, None, ctypes.byref(ctl),
        None, None, ctypes.byref(atoms), _hip.stream_ptr(dev))
    assert rc == -1 and b"class weights" in lib.arreau_last_error()
    torch.cuda.synchronize(dev)
    assert torch.equal(eps, before)
    assert_same_bits(got, start, "rejected loop")
    eng.check_status()


# ------------------------------------------------------------------------------------------- the loop against its steps
def _class_table(m, params=LOOP_PARAMS):
    return xg.class_weights(AtomicNumberTable(m.z_table_zs.tolist()), params)


def _loop_guidance(eng, m, case, dev, weight=WEIGHT, seed=99):
    """A DeviceGuidance for `case`: the targets are the patterns of other positions and species in the case's starting cells."""
    other = Batch(dev, seed=seed, sampler_like=False)
    table = torch.as_tensor(_class_table(m), device=dev)
    f, ty, le, _ = case.fresh()
    w = table[other.types.to(dev).long()].contiguous()
    rows = xrd.xrd(other.frac.to(dev).contiguous(), lattice_from_params(le, case.an), case.off, w, xrd.for_weights(LOOP_PARAMS))["pattern"]
    assert bool(torch.isfinite(rows).all()) and bool((rows.sum(1) > 0).all())
    return xg.DeviceGuidance(LOOP_PARAMS, weight, rows.contiguous(), class_weights=table, info=xg.allocate_info(case.B, dev))


def _chain(eng, case, guide, steps, form, seed=SEED):
    """predict_scores -> (contact_guidance_step ->) xrd_guidance_step -> (corrector_step -> the same evaluation ->) reverse_step
    for every step, from a copy of the case's start; a fixed cell and held species are put back after every step, as the loop
    re-imposes them.  Returns the state."""
    f, ty, le, lat = state = case.fresh()
    B, N, dev = case.B, case.N, eng.device
    fixed, held = le.clone(), ty.clone()
    contact = (CONTACTS, cg.allocate_info(B, dev)) if form == "contacts" else None

    def evaluate(t_c):
        eps, logits, len0 = eng.predict_scores(f, ty, le, case.an, t_c, case.off)
        cell = lattice_from_params(le, case.an)
        if contact is not None:
            eng.contact_guidance_step(f, cell, t_c, case.off, eps, contact)
        eng.xrd_guidance_step(f, ty, cell, t_c, case.off, eps, guide)
        return eps, logits, len0
    for t in steps:
        t_c = full_i32(B, t, dev)
        scores = evaluate(t_c)
        if form == "corrector":
            eng.corrector_step(f, t_c, case.off, scores[0], eng.philox_fill_word(seed, t, 5, 0, 3 * N).view(N, 3), SNR)
            scores = evaluate(t_c)
        z_l, z_f, u_t = (eng.philox_fill(seed, t, 0, 3 * B).view(B, 3), eng.philox_fill(seed, t, 1, 3 * N).view(N, 3),
                         eng.philox_fill(seed, t, 2, N * S).view(N, S))
        eng.reverse_step(f, ty, le, case.an, t_c, case.off, *scores, z_l, z_f, u_t, lat)
        if form == "fixed cell":
            le.copy_(fixed)
        if form == "constant species":
            ty.copy_(held)
    return state, contact


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
@pytest.mark.parametrize("form", ["plain", "corrector", "contacts", "fixed cell", "constant species"])
def test_guided_loop_is_its_steps_bit_for_bit(dev, fused_model, form, loop_prep, monkeypatch):
    """Three steps of Engine.sample_loop(xrd_guidance=...) against evaluate, guide and step, eager and with graph replay: the state
    and the diagnostics of the last evaluation.  With contact guidance in the same call the order is rule 7's.  The guidance is
    not idle: the loop without it ends elsewhere.  (A fixed cell: positions, species and lengths; the loop writes its cell output
    from the held lengths in another kernel.)"""
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = fused_model
    eng = m.engine()
    case = Batch(dev, seed=41, sampler_like=False)
    steps = [60, 59, 58]
    want_guide = _loop_guidance(eng, m, case, dev)
    want, want_contact = _chain(eng, case, want_guide, steps, form)
    held = case.fresh()
    kw = {"corrector": dict(corrector=(1, SNR)), "fixed cell": dict(fixed_lengths=held[2].clone())}.get(form, {})
    const = held[1].clone() if form == "constant species" else None
    compared = slice(0, 3) if form == "fixed cell" else slice(0, 4)
    for use_graph in (False, True):
        got = case.fresh()
        guide = _loop_guidance(eng, m, case, dev)
        contact = (CONTACTS, cg.allocate_info(case.B, dev)) if form == "contacts" else None
        eng.sample_loop(*got[:3], case.an, case.off, steps[0], len(steps), SEED, const, got[3], use_graph=use_graph, guidance=contact,
                        xrd_guidance=guide, **kw)
        assert_same_bits(got[compared], want[compared], (form, loop_prep, use_graph))
        assert_same_bits([guide.info[q] for q in xg.INFO_KEYS], [want_guide.info[q] for q in xg.INFO_KEYS], (form, "info", use_graph), nan_ok=True)
        if contact is not None:
            assert_same_bits([contact[1][q] for q in cg.INFO_KEYS], [want_contact[1][q] for q in cg.INFO_KEYS], (form, "contact info"))
    assert bool((want_guide.info["flags"] == 0).any())
    plain = case.fresh()
    eng.sample_loop(*plain[:3], case.an, case.off, steps[0], len(steps), SEED, const, plain[3],
                    guidance=(CONTACTS, cg.allocate_info(case.B, dev)) if form == "contacts" else None, **kw)
    assert not torch.equal(plain[0], want[0])
    eng.check_status()


def test_none_weight_zero_and_a_null_struct_are_the_guided_loop(dev, fused_model):
    """xrd_guidance=None, weight 0 and arreau_sample_loop_xrd_guided with a NULL struct are arreau_sample_loop_guided bit for bit;
    another weight on the same buffers with graph replay is not a stale replay (the struct is part of the graph key)."""
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    lib = _hip.lib()
    case = Batch(dev, seed=53, sampler_like=False)
    contact = lambda: (CONTACTS, cg.allocate_info(case.B, dev))
    want = case.fresh()
    eng.sample_loop(*want[:3], case.an, case.off, 30, 3, SEED, None, want[3], guidance=contact())
    zero = case.fresh()
    eng.sample_loop(*zero[:3], case.an, case.off, 30, 3, SEED, None, zero[3], guidance=contact(), xrd_guidance=_loop_guidance(eng, m, case, dev, 0.0))
    assert_same_bits(zero, want, "weight 0")
    got = case.fresh()
    ws = eng.workspace(case.N, case.B)
    ctl = _hip.SpeciesControlC(None, 1.0)
    c = eng._guidance_struct(contact(), case.B)
    _hip.check(lib.arreau_sample_loop_xrd_guided(
        eng._handle, _hip.ptr(got[0]), _hip.ptr(got[1]), _hip.ptr(got[2]), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N, 30, 3, SEED,
        None, None, _hip.ptr(got[3]), _hip.ptr(ws), ws.numel(), 0, None, None, None, None, None, None, None, None, ctypes.byref(ctl),
        None, ctypes.byref(c), None, _hip.stream_ptr(dev)), "arreau_sample_loop_xrd_guided")
    assert_same_bits(got, want, "NULL struct")
    bufs, seen = case.fresh(), []
    for weight in (2.0, 0.5, 0.0, 2.0):
        case.load(bufs)
        eng.sample_loop(*bufs[:3], case.an, case.off, 50, 4, SEED, None, bufs[3], use_graph=True, xrd_guidance=_loop_guidance(eng, m, case, dev, weight))
        eager = case.fresh()
        eng.sample_loop(*eager[:3], case.an, case.off, 50, 4, SEED, None, eager[3], xrd_guidance=_loop_guidance(eng, m, case, dev, weight))
        assert_same_bits(bufs, eager, weight)
        seen.append(bufs[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and torch.equal(seen[0], seen[3])
    eng.check_status()


# ------------------------------------------------------------------------------------------- sample()
def _start(case, t):
    return inversion.SamplerState(frac_x=case.frac.numpy().astype(np.float64) % 1.0, species=case.types.numpy().astype(np.int64),
                                  lengths=case.lengths.numpy().astype(np.float64), angles=case.angles.numpy().astype(np.float64),
                                  num_atoms=np.asarray(Batch.COUNTS, dtype=np.int64), t=t)


def test_sample_takes_the_option_in_every_noise_mode(dev, fused_model):
    """At eta = 0 and species temperature 0 no draw is read, so sample(noise=...) from one state is the same run in all three
    modes: the library loop and the host-noise driver's evaluate() return the same bytes and the same diagnostics in
    SampleResult.info["xrd_guidance"], and differ from the call without the option.  Targets given as crystals are the patterns
    xrd.xrd gives for them; None is the sampler as it was; encode rejects the option."""
    m, _ = fused_model
    case = Batch(dev, seed=61, sampler_like=False)
    state = _start(case, 40)
    other = Batch(dev, seed=62, sampler_like=False)
    zs = np.asarray(m.z_table_zs.tolist())
    crystals = type("Crystals", (), {})()
    crystals.frac_x, crystals.lattice = other.frac.numpy().astype(np.float64), lattice_from_params(case.lengths.to(dev), case.an).cpu().numpy().astype(np.float64)
    crystals.num_atoms, crystals.atomic_numbers = np.asarray(Batch.COUNTS), zs[np.minimum(other.types.numpy(), S - 2)]
    guide = xg.XrdGuidance(crystals, weight=WEIGHT, params=LOOP_PARAMS)
    kw = dict(initial_state=state, num_steps=6, eta=0.0, species_temperature=0.0)
    keys = ("frac_x", "atomic_numbers", "lattice", "num_atoms")
    runs = {mode: m.sample(xrd_guidance=guide, noise=mode, **kw) for mode in ("philox", "device", "reference")}
    plain = m.sample(noise="philox", **kw)
    none = m.sample(noise="philox", xrd_guidance=None, **kw)
    want = runs["philox"]
    info = want.info["xrd_guidance"]
    assert set(info) == set(xg.INFO_KEYS) and info["distance"].shape == (3,) and info["distance"].dtype == np.float32
    assert (info["flags"] == 0).any() and "xrd_guidance" not in (plain.info or {})
    for mode, res in runs.items():
        for q in keys:
            assert np.asarray(getattr(res, q)).tobytes() == np.asarray(getattr(want, q)).tobytes(), (mode, q)
        for q in xg.INFO_KEYS:
            assert res.info["xrd_guidance"][q].tobytes() == info[q].tobytes(), (mode, q)
        assert not np.array_equal(res.frac_x, plain.frac_x), mode
    for q in keys:
        assert np.asarray(getattr(none, q)).tobytes() == np.asarray(getattr(plain, q)).tobytes(), q
    rows = guide.patterns(3, dev)
    again = m.sample(xrd_guidance=xg.XrdGuidance(rows, weight=WEIGHT, params=LOOP_PARAMS), noise="philox", **kw)
    assert np.asarray(again.frac_x).tobytes() == np.asarray(want.frac_x).tobytes()
    with pytest.raises(ValueError, match="inversion"):
        m.encode(plain, t=10, xrd_guidance=guide)
    with pytest.raises(ValueError, match="xrd_guidance must be"):
        m.sample(Batch.COUNTS, 3, max_steps=2, xrd_guidance=True)
