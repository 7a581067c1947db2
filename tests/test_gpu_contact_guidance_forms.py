"""Contact guidance under every predictor the loop accepts (rule 5 of include/arreau_hip.h, "contact guidance": "ancestral,
respaced, eta, multistep and its history, tied, symmetric, species control, keyed" and the corrector; rule 6: evaluate, guide,
correct, evaluate, guide, predict; rule 7: known atoms still push).  tests/test_gpu_contact_guidance.py runs plain, respaced at
eta = 0, corrector and keyed; here: an eta > 0, a tie, multistep and its history, species rows, a symmetric step, a fixed cell,
resampling, all of them combined with a condition, the shape-general model, and the host-noise drivers.  In the loop without a
prep launch the cell the guidance launch reads is left behind by another update-kernel instance (or by the jump kernel) in each
of these, and the timestep it reads is advanced by another kernel.

The pattern is that module's `chain`: predict_scores, contact_guidance_step on lattice_from_params(lengths, angles), the form's
step export fed arreau_philox_fill's draws, against Engine.sample_loop(guidance=...): the state and the three diagnostic arrays
of the last evaluation bit for bit, eager and with graph replay.  Each form also shows (b) that the unguided loop with the same
options ends elsewhere and (c) that the guided loop without the option ends elsewhere.

Not here: the kernel's 64-bit index branch (n M above 2^32 - 64) needs about 900 000 atoms in one crystal at the largest image
count and stays untested.  Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest
import torch

from arreau_amd.diffusion import contact_guidance as cg, multistep as ms, resampling as rs, respacing, species as sp
from arreau_amd.diffusion.lattice_helpers import lattice_from_params
from tests import species_cases as C
from tests.sampling_helpers import S, T, any_model, assert_same_bits, dev, full_i32, fused_model, model_seed  # noqa: F401 (fixtures)
from tests.test_gpu_contact_guidance import CLIP, GUIDE, SEED, SNR, Batch, chain, draws, guided_scores

pytestmark = pytest.mark.gpu

STEPS = [60, 30, 1]  # the respaced forms' schedule
INFO = lambda info: [info[q] for q in cg.INFO_KEYS]


def _prep(monkeypatch, loop_prep):
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)


def _loop(eng, start, an, off, steps, guidance, use_graph=False, **kw):
    """Engine.sample_loop over `steps` from a copy of `start`: (the state, the info arrays)."""
    got = tuple(x.clone() for x in start)
    info = cg.allocate_info(got[2].shape[0], eng.device)
    eng.sample_loop(*got[:3], an, off, steps[0], len(steps), SEED, None, got[3], use_graph=use_graph,
                    guidance=(GUIDE, info) if guidance else None, **kw)
    return got, info


def _differs(a, b):
    return any(not torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def _assert_form(eng, start, an, off, steps, want, want_info, what, kw, without, loose_cell=False):
    """(a) loop == chain, eager and replayed; (b) the unguided loop differs; (c) the guided loop under `without` differs; (d)."""
    for use_graph in (False, True):
        got, info = _loop(eng, start, an, off, steps, True, use_graph, **kw)
        if loose_cell:  # (the cell: another kernel's evaluation of it)
            assert_same_bits(got[:3], want[:3], (what, use_graph))
            assert torch.allclose(got[3], want[3], rtol=1e-6, atol=1e-6), (what, use_graph)
        else:
            assert_same_bits(got, want, (what, use_graph))
        assert_same_bits(INFO(info), INFO(want_info), (what, "info", use_graph))
    unguided, _ = _loop(eng, start, an, off, steps, False, **kw)
    assert not torch.equal(unguided[0], want[0]), (what, "the guidance is idle")
    other, _ = _loop(eng, start, an, off, steps, True, **without)
    assert _differs(other, want), (what, "the option is not taken")
    eng.check_status()
    return unguided


# ------------------------------------------------------------------------------------------- one option each
FORMS = ["eta", "tied", "multistep", "multistep-tied", "species", "fixed cell"]
BOTH = {"tied", "multistep", "multistep-tied"}  # the forms run with a prep launch per step too


@pytest.mark.parametrize("form,loop_prep", [(f, p) for f in FORMS for p in ((None, "1") if f in BOTH else (None,))],
                         ids=lambda v: {None: "no-prep", "1": "prep-per-step"}.get(v, v))
def test_guided_loop_with_an_option_is_its_steps(dev, fused_model, form, loop_prep, monkeypatch):
    """Respaced [60, 30, 1] on the batch of 4, 8 and 5 atoms: eta = 0.3 through reverse_step_eta; a tie [0, 1, 2] through
    reverse_step_tied; multistep with and without the tie through reverse_step_multistep, its four history buffers bit for bit
    too (rule 5: the history holds eps', so hist_eps differs from the unguided run's); species rows at temperature 0.5 through
    reverse_step_species, the final species within their sets; fixed_lengths through reverse_step_to with the lengths put back
    after every step, as the loop re-imposes them: the lengths stay the start's bits."""
    _prep(monkeypatch, loop_prep)
    m, _ = fused_model
    eng = m.engine()
    case = Batch(dev, seed=41)
    B, N = case.B, case.N
    start = case.fresh()
    tie = torch.as_tensor([0, 1, 2], dtype=torch.int32, device=dev)
    rows = C.rows_of(C.ROWS["S12"]["mixed"][:B], S)
    ctl = (sp.device_rows(rows, dev), 0.5)
    base = dict(next_table=respacing.next_table(T, STEPS).to(dev), lattice_clipmax=CLIP)
    hists = {k: ms.allocate_history(N, B, dev) for k in ("chain", "loop", "unguided")}
    opt = {"eta": dict(eta=0.3), "tied": dict(length_tie=tie), "multistep": {}, "multistep-tied": dict(length_tie=tie), "species": dict(species=ctl),
           "fixed cell": dict(fixed_lengths=start[2].clone())}[form]

    def step(state, t, s, t_c, s_c, scores):
        f, ty, le, lat = state
        z_l, z_f, u_t = draws(eng, SEED, t, B, N)
        a = (f, ty, le, case.an, t_c, s_c, case.off, *scores)
        if form == "eta":
            eng.reverse_step_eta(*a, z_l, z_f, u_t, lat, 0.3, None, CLIP)
        elif form == "tied":
            eng.reverse_step_tied(*a, z_l, z_f, u_t, lat, tie, CLIP)
        elif form.startswith("multistep"):
            eng.reverse_step_multistep(*a, u_t, lat, hists["chain"], opt.get("length_tie"), CLIP)
        elif form == "species":
            eng.reverse_step_species(*a, z_l, z_f, u_t, lat, ctl, lattice_clipmax=CLIP)
        else:
            eng.reverse_step_to(*a, z_l, z_f, u_t, lat, CLIP)
            le.copy_(opt["fixed_lengths"])
            lat.copy_(lattice_from_params(le, case.an))
    want, want_info = chain(eng, start, case.an, case.off, STEPS, STEPS[1:] + [0], step)
    if not form.startswith("multistep"):
        _assert_form(eng, start, case.an, case.off, STEPS, want, want_info, form, dict(base, **opt), base, loose_cell=form == "fixed cell")
        if form == "species":
            E = sp.admitted(rows, 1)[case.crystal]
            ty = want[1].cpu().numpy().astype(np.int64)
            assert bool(E[np.arange(N), ty].all())
        if form == "fixed cell":
            assert_same_bits([want[2]], [start[2]], "the fixed lengths")
        return
    # multistep: the history is read and overwritten by every call, so every run gets an empty one
    for use_graph in (False, True):
        ms.empty_history(hists["loop"])
        got, info = _loop(eng, start, case.an, case.off, STEPS, True, use_graph, multistep=hists["loop"], **base, **opt)
        assert_same_bits(got, want, (form, use_graph))
        assert_same_bits(INFO(info), INFO(want_info), (form, "info", use_graph))
        assert_same_bits([hists["loop"][k] for k in ms.HISTORY_KEYS], [hists["chain"][k] for k in ms.HISTORY_KEYS], (form, "history", use_graph))
    unguided, _ = _loop(eng, start, case.an, case.off, STEPS, False, multistep=hists["unguided"], **base, **opt)
    assert not torch.equal(unguided[0], want[0])
    assert not torch.equal(hists["unguided"]["hist_eps"], hists["chain"]["hist_eps"])  # the history holds the guided eps'
    assert torch.equal(hists["unguided"]["hist_t_atom"], hists["chain"]["hist_t_atom"])
    other, _ = _loop(eng, start, case.an, case.off, STEPS, True, eta=0.0, **base, **opt)  # the eta = 0 step it extrapolates
    assert _differs(other, want)
    eng.check_status()


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
def test_guided_symmetric_loop_is_its_steps(dev, fused_model, loop_prep, monkeypatch):
    """The symmetry batch of test_symmetric_species_loop_is_its_steps with its tie and tables, through reverse_step_sym.  The
    gradient of a symmetric penalty is equivariant, so the guided loop's end keeps the orbits (assert_symmetric)."""
    from tests import symmetry_cases as SC
    from tests.test_gpu_symmetry import _on_device, assert_symmetric
    _prep(monkeypatch, loop_prep)
    m, _ = fused_model
    eng = m.engine()
    specs, counts = SC.batch(SC.LOOP)
    B, N = len(counts), sum(counts)
    start, an, off, tie, tables = _on_device(dev, specs, counts, S, 61, cell=(7.0, 11.0))
    eng.status(reset=True)

    def step(state, t, s, t_c, s_c, scores):
        f, ty, le, lat = state
        eng.reverse_step_sym(f, ty, le, an, t_c, s_c, off, *scores, *draws(eng, SEED, t, B, N), lat, tie, tables, CLIP)
    want, want_info = chain(eng, start, an, off, STEPS, STEPS[1:] + [0], step)
    base = dict(next_table=respacing.next_table(T, STEPS).to(dev), lattice_clipmax=CLIP)
    guided = (want_info["flags"].cpu().numpy() & cg.SKIPPED) == 0  # (the 3-atom crystal's shrinking cell ends CELL: left alone)
    assert int(want_info["contacts"].cpu().numpy()[guided].sum()) > 0 and guided[[0, 2, 3, 5, 6, 7]].all()  # every symmetric crystal is guided
    _assert_form(eng, start, an, off, STEPS, want, want_info, "symmetric", dict(base, length_tie=tie, symmetry=tables), dict(base, length_tie=tie))
    assert_symmetric(specs, counts, want[0].cpu().numpy(), want[1].cpu().numpy(), "the guided loop's end")


# ------------------------------------------------------------------------------------------- resampling
def _events(eng, start, an, off, steps, succ, R, J, respaced, seed=SEED):
    """The events of resampling.plan one by one, every evaluation guided: a jump is resample_jump on _jump_noise, a step uses the
    draws of counter word 256 r."""
    from tests.test_gpu_resampled_sampling import _jump_noise
    f, ty, le, lat = state = tuple(x.clone() for x in start)
    B, N, dev = le.shape[0], f.shape[0], eng.device
    info = cg.allocate_info(B, dev)
    for ev in rs.plan(steps, succ, R, J):
        if ev.kind == "jump":
            eng.resample_jump(f, ty, le, an, full_i32(B, ev.s, dev), full_i32(B, ev.t, dev), off, *_jump_noise(eng, seed, ev.t, ev.r, B, N), lat)
            continue
        t_c = full_i32(B, ev.t, dev)
        scores = guided_scores(eng, state, an, off, t_c, info)
        noise = draws(eng, seed, ev.t, B, N, 256 * ev.r)
        if respaced:
            eng.reverse_step_to(f, ty, le, an, t_c, full_i32(B, ev.s, dev), off, *scores, *noise, lat, CLIP)
        else:
            eng.reverse_step(f, ty, le, an, t_c, off, *scores, *noise, lat)
    return state, info


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
@pytest.mark.parametrize("respaced", [False, True], ids=["plain", "respaced"])
def test_guided_resampled_loop_is_its_events(dev, fused_model, respaced, loop_prep, monkeypatch):
    """R = 2, J = 2 on [60, 59, 58, 57] and on the respaced [60, 30, 10, 1]: after a jump the guidance launch reads the cell the
    jump kernel left and the timestep the jump set back."""
    _prep(monkeypatch, loop_prep)
    m, _ = fused_model
    eng = m.engine()
    case, R, J = Batch(dev, seed=41), 2, 2
    start = case.fresh()
    steps, succ = ([60, 30, 10, 1], 0) if respaced else ([60, 59, 58, 57], 56)
    base = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP) if respaced else {}
    want, want_info = _events(eng, start, case.an, case.off, steps, succ, R, J, respaced)
    _assert_form(eng, start, case.an, case.off, steps, want, want_info, ("resampled", respaced),
                 dict(base, resampling=(R, J, steps) if respaced else (R, J)), base)


# ------------------------------------------------------------------------------------------- everything at once
def _min_image_distance(a, b, L):
    d = a - b
    d -= np.rint(d)
    shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)
    return float(np.linalg.norm((d + shifts) @ L, axis=1).min())


def test_guided_combined_loop_is_its_events(dev, fused_model):
    """The event walk of test_combined_species_loop_is_its_events -- respaced, conditioned, one corrector move per step,
    resampling (R = 2, J = 2), species rows -- with the guidance launch after every evaluation (rule 6: evaluate, guide, correct,
    evaluate, guide, predict), block by block against the loop with graph replay: positions, species and lengths bit for bit, the
    cell to its 1e-6, the diagnostics of the block's last evaluation bit for bit.  Rule 7: the known atoms end on the template,
    and still push: a free atom that ends within d0 of a known one ends elsewhere once that known atom's template position is
    moved out of its range."""
    from arreau_amd import _hip
    from tests.test_gpu_ddim_sampling import _condition
    from tests.test_gpu_resampled_sampling import _jump_noise, _replace
    from tests.test_gpu_species_sampling import Case as SpeciesCase

    m, om = fused_model
    eng = m.engine()
    case, seed, R, J, M = SpeciesCase(dev, seed=43, sampler_like=False), 31415, 2, 2, 1
    B, N = case.B, case.N
    cond = _condition(case)
    rows = C.rows_of(C.ROWS["S12"]["mixed"], S)
    ctl = (sp.device_rows(rows, dev), 0.5)
    steps = [60, 45, 30, 20, 3, 2, 1]
    kw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP, resampling=(R, J, steps), corrector=(M, SNR), species=ctl)
    pm, tm, lm = cond["pos_mask"].bool(), cond["type_mask"].bool(), cond["len_mask"].bool()
    loop = case.fresh()
    eng.status(reset=True)
    eng.condition_initial_state(*loop[:3], steps[0], seed, cond)
    first = tuple(x.clone() for x in loop)
    info, want_info = cg.allocate_info(B, dev), cg.allocate_info(B, dev)
    for lo in range(0, len(steps), J):
        hi = min(lo + J, len(steps))
        f, ty, le, lat = state = tuple(x.clone() for x in loop)
        eng.sample_loop(*loop[:3], case.an, case.off, steps[lo], hi - lo, seed, None, loop[3], use_graph=True, condition=cond,
                        guidance=(GUIDE, info), **kw)
        for ev in rs.plan(steps[lo:hi], steps[hi] if hi < len(steps) else 0, R, J):
            if ev.kind == "jump":
                eng.resample_jump(f, ty, le, case.an, full_i32(B, ev.s, dev), full_i32(B, ev.t, dev), case.off,
                                  *_jump_noise(eng, seed, ev.t, ev.r, B, N), lat, condition=cond)
                continue
            t, w = ev.t, 256 * ev.r
            t_c = full_i32(B, t, dev)
            scores = guided_scores(eng, state, case.an, case.off, t_c, want_info)
            for j in range(M):
                eng.corrector_step(f, t_c, case.off, scores[0], eng.philox_fill_word(seed, t, 5, w + j, 3 * N).view(N, 3), SNR, condition=cond)
                scores = guided_scores(eng, state, case.an, case.off, t_c, want_info)
            eng.reverse_step_species(f, ty, le, case.an, t_c, full_i32(B, ev.s, dev), case.off, *scores, *draws(eng, seed, t, B, N, w), lat, ctl,
                                     lattice_clipmax=CLIP)
            _replace(eng, om, cond, seed, t, ev.s, ev.r, f, ty, le, case.an, lat)
        assert torch.equal(loop[1][tm], cond["a0"][tm]), steps[lo]
        assert_same_bits(loop[:3], (f, ty, le), steps[lo])
        assert torch.allclose(loop[3], lat, rtol=1e-6, atol=1e-6), steps[lo]  # (the cell: another kernel's evaluation of it)
        assert_same_bits(INFO(info), INFO(want_info), (steps[lo], "info"))
    free = ~tm.cpu().numpy()
    E = sp.admitted(rows, 1)[case.crystal[free]]
    assert bool(E[np.arange(int(free.sum())), loop[1][~tm].cpu().numpy().astype(np.int64)].all())
    assert not eng.status(reset=True)["flags"] & (_hip.STATUS_BAD_TIMESTEP | _hip.STATUS_BAD_TYPE)
    # rule 7: the run ends at 0, the known atoms on the template
    assert torch.equal(loop[0][pm], torch.remainder(cond["x0"], 1.0)[pm]) and torch.equal(loop[2][lm], cond["l0"][lm])
    # the guidance is not idle, and the known atoms push: the closest (free, known) pair of the end state
    unguided = tuple(x.clone() for x in first)
    eng.sample_loop(*unguided[:3], case.an, case.off, steps[0], len(steps), seed, None, unguided[3], condition=cond, **kw)
    assert not torch.equal(unguided[0][~pm], loop[0][~pm])
    x, L, known = loop[0].cpu().numpy().astype(np.float64), loop[3].cpu().numpy().astype(np.float64), pm.cpu().numpy().astype(bool)
    d0 = GUIDE.min_distance
    pairs = [(_min_image_distance(x[k], x[i], L[case.crystal[i]]), i, k) for i in range(N) if not known[i]
             for k in np.nonzero(known & (case.crystal == case.crystal[i]))[0]]
    d, i, k = min(pairs)
    assert d < d0, "no free atom ends within d0 of a known one: another seed"
    halves = [np.array(h) * 0.5 for h in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))]
    far, shift = max(((_min_image_distance(x[k] + h, x[i], L[case.crystal[i]]), h) for h in halves), key=lambda p: p[0])
    assert far > d0
    moved = {q: v.clone() for q, v in cond.items()}
    moved["x0"][k] += torch.as_tensor(shift, dtype=torch.float32, device=dev)
    again = tuple(x.clone() for x in first)
    eng.sample_loop(*again[:3], case.an, case.off, steps[0], len(steps), seed, None, again[3], condition=moved, guidance=GUIDE, **kw)
    assert not torch.equal(again[0][i], loop[0][i])
    eng.check_status()


# ------------------------------------------------------------------------------------------- the shape-general model
@pytest.mark.parametrize("form", ["plain", "respaced-eta0"])
def test_guided_loop_is_its_steps_on_every_model(dev, any_model, form):
    """The forms of test_guided_loop_is_its_steps_bit_for_bit on the shape-general model (general-C64) too: its loop has a prep
    launch in every step and another network path in front of the same guidance launch."""
    m, _ = any_model
    eng = m.engine()
    case = Batch(dev, seed=41)
    B, N = case.B, case.N
    start = case.fresh()
    if form == "plain":
        steps, succ, kw = [60, 59, 58], [59, 58, 57], {}
    else:
        steps, succ, kw = STEPS, STEPS[1:] + [0], dict(next_table=respacing.next_table(T, STEPS).to(dev), lattice_clipmax=CLIP, eta=0.0)

    def step(state, t, s, t_c, s_c, scores):
        f, ty, le, lat = state
        z_l, z_f, u_t = draws(eng, SEED, t, B, N)
        if form == "plain":
            eng.reverse_step(f, ty, le, case.an, t_c, case.off, *scores, z_l, z_f, u_t, lat)
        else:
            eng.reverse_step_eta(f, ty, le, case.an, t_c, s_c, case.off, *scores, None, None, u_t, lat, 0.0, None, CLIP)
    want, want_info = chain(eng, start, case.an, case.off, steps, succ, step)
    for use_graph in (False, True):
        got, info = _loop(eng, start, case.an, case.off, steps, True, use_graph, **kw)
        assert_same_bits(got, want, (form, use_graph))
        assert_same_bits(INFO(info), INFO(want_info), (form, "info", use_graph))
    unguided, _ = _loop(eng, start, case.an, case.off, steps, False, **kw)
    assert not torch.equal(unguided[0], want[0])
    eng.check_status()


# ------------------------------------------------------------------------------------------- the host-noise drivers
def test_the_noise_modes_agree_where_no_draw_is_read(dev, fused_model):
    """At eta = 0 and species temperature 0 no draw is read, so sample(noise=...) from one initial state is the same run in all
    three modes: the library loop ('philox') and the host-noise driver's evaluate() ('device', 'reference') must return the same
    bytes -- frac_x, atomic_numbers, lattice and the three contact_guidance arrays -- and differ from the unguided call.  With
    corrector_steps = 1 the modes would not agree: the corrector's move reads a normal draw, which 'philox' takes from the keyed
    stream and the host modes from torch's generators, and no argument makes it common; that combination is left out."""
    m, _ = fused_model
    counts = [3, 8, 1, 5]
    torch.manual_seed(7)
    np.random.seed(7)
    state = m.diffusion_loss.draw_initial_state(counts, len(counts), num_atomic_states=S)
    kw = dict(initial_state=state, num_steps=10, eta=0.0, species_temperature=0.0)
    keys = ("frac_x", "atomic_numbers", "lattice", "num_atoms")
    fields = lambda: {k: np.array(v).tobytes() for k, v in vars(state).items() if isinstance(v, (np.ndarray, torch.Tensor))}
    before, runs = fields(), {}
    assert before
    for mode in ("philox", "device", "reference"):
        runs[mode] = m.sample(contact_guidance=GUIDE, noise=mode, **kw)
        assert fields() == before, mode  # every run starts from the same state
    plain = m.sample(noise="philox", **kw)
    want = runs["philox"]
    assert np.isfinite(want.frac_x).all() and np.isfinite(want.lattice).all()
    for mode, res in runs.items():
        for q in keys:
            assert np.asarray(getattr(res, q)).tobytes() == np.asarray(getattr(want, q)).tobytes(), (mode, q)
        for q in cg.INFO_KEYS:
            a, b = res.info["contact_guidance"][q], want.info["contact_guidance"][q]
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (mode, q)
        assert not np.array_equal(res.frac_x, plain.frac_x), mode
