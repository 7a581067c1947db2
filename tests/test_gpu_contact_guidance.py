"""Contact guidance on the GPU (rules in include/arreau_hip.h, "contact guidance"; diffusion/contact_guidance.py): the guidance
launch against the float64 restatement within the derived float32 bounds, its reproducibility, the guided loop against its steps
bit for bit, the step identity, and the paths that must not change.  The launch cases reach 257 atoms in one crystal (the path
that does not stage positions in LDS), eight image shells, 70 crystals and timesteps outside 1..T; the kernel's 64-bit index
branch (n M above 2^32 - 64: about 900 000 atoms in one crystal at the largest M) stays untested.  The loop under the other
predictor forms: tests/test_gpu_contact_guidance_forms.py, which imports `chain`, `guided_scores` and `draws` from here."""
import ctypes

import numpy as np
import pytest
import torch

from arreau_amd.diffusion import contact_guidance as cg, keyed, respacing
from arreau_amd.diffusion.lattice_helpers import lattice_from_params
from tests import contact_guidance_cases as cases
from tests.sampling_helpers import Case, S, T, assert_same_bits, dev, full_i32, fused_model, model_seed  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SEED = 20250311
CLIP = 0.999
SNR = 0.16
GUIDE = cg.ContactGuidance(min_distance=2.0, weight=0.3)  # the loop tests': wide enough that the random crystals hold contacts
FLAT_BATCH = cases.batch_of("flat+pair", [cases.flat_case(), cases.GuidanceCase("pair1", cases.pair_case().frac, cases.pair_case().lattice, [2],
                                                                               cases.flat_case().params, contacts=[1])])
STEP_CASES = cases.all_cases() + [cases.mixed_batch(), FLAT_BATCH] + cases.launch_cases()  # (`large`: the unstaged path; `eight shells`)

assert cases.T == T


class Batch(Case):
    COUNTS = [4, 8, 5]


def _sigmas(m):
    return m.diffusion_loss.pos_diffusion.sigmas.detach().cpu().to(torch.float32).numpy().astype(np.float64)


def _upload(case, dev):
    d = lambda a: torch.as_tensor(a, device=dev).contiguous()
    return d(case.frac), d(case.lattice), d(case.t), d(case.offsets)


def _guide_step(eng, case, dev, eps, params=None):
    """One launch on a copy of eps [N,3] (numpy float32): (eps' as numpy, the info arrays as numpy)."""
    frac, lattice, t, off = _upload(case, dev)
    info = cg.allocate_info(case.B, dev)
    out = torch.as_tensor(eps, device=dev).contiguous().clone()
    eng.contact_guidance_step(frac, lattice, t, off, out, (params or case.params, info))
    return out.cpu().numpy(), cg.info_to_numpy(info)


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- the launch against the restatement
@pytest.mark.parametrize("case", STEP_CASES, ids=[c.name for c in STEP_CASES])
def test_step_matches_the_restatement(dev, fused_model, case):
    """eps' within eps_bound (the derived float32 bound on g times w / sigma_t^2, plus the last two roundings), g itself (from
    eps = 0) within g_bound, contacts and flags equal, the energy within energy_bound; a flagged crystal's eps unchanged bit for
    bit; a second launch gives the same bits."""
    m, _ = fused_model
    eng = m.engine()
    ref = cg.reference(case.frac, case.lattice, case.offsets, case.params)
    sig = _sigmas(m)
    k = cg.sigma_coefficient(sig, case.t, case.params.weight)
    d0 = float(np.float32(case.params.min_distance))
    eps = np.random.RandomState(7).normal(size=case.frac.shape).astype(np.float32)
    got, info = _guide_step(eng, case, dev, eps)
    again, info2 = _guide_step(eng, case, dev, eps)
    assert _same_bytes(got, again) and all(_same_bytes(info[q], info2[q]) for q in cg.INFO_KEYS)
    g_only, _ = _guide_step(eng, case, dev, np.zeros_like(eps))
    want = cg.guided_eps(eps, ref, case.offsets, sig, case.t, case.params)
    assert list(info["flags"]) == list(ref.flags) == list(case.flags)
    assert list(info["contacts"]) == list(ref.contacts)
    for b in range(case.B):
        a, e = case.offsets[b], case.offsets[b + 1]
        if ref.flags[b] & cg.SKIPPED:
            assert _same_bytes(got[a:e], eps[a:e]) and info["energy"][b] == 0 and info["contacts"][b] == 0
            continue
        most = int(ref.atom_contacts[a:e].max()) if e > a else 0
        gb = cg.g_bound(d0, ref.d_min[b], case.lattice[b], ref.shells[b], most)
        tol = cg.eps_bound(k[b], gb, ref.g[a:e], want[a:e])
        err = np.abs(got[a:e].astype(np.float64) - want[a:e])
        g_err = np.abs(g_only[a:e].astype(np.float64) / k[b] - ref.g[a:e])
        g_tol = gb + 6 * cg.U32 * np.abs(ref.g[a:e])  # (k in float32 and the product: 4 u of |g|, and 2 u to spare)
        ub = cg.energy_bound(d0, case.lattice[b], ref.shells[b], ref.ordered[b], ref.U[b])
        print(f"{case.name}[{b}]: n {e - a}, contacts {ref.contacts[b]}, largest |g| {np.abs(ref.g[a:e]).max():.3g}, g error {g_err.max():.3g} "
              f"of bound {gb:.3g}, eps' error / bound {np.max(err / np.maximum(tol, 1e-300)):.3g}, U {ref.U[b]:.6g} error "
              f"{abs(float(info['energy'][b]) - ref.U[b]):.3g} of bound {ub:.3g}")
        assert (g_err <= g_tol).all() and (err <= tol).all()
        assert abs(float(info["energy"][b]) - ref.U[b]) <= ub
        if ref.ordered[b] == 0:  # no contact: eps + k 0 is eps
            assert np.array_equal(got[a:e], eps[a:e])
    eng.check_status()


def test_diagnostics_are_optional_and_weight_zero_adds_nothing(dev, fused_model):
    """NULL diagnostic pointers: the same eps'.  weight == 0 through the step export: eps + 0 g, the diagnostics still written."""
    m, _ = fused_model
    eng = m.engine()
    case = cases.ragged_case()
    eps = np.random.RandomState(8).normal(size=case.frac.shape).astype(np.float32)
    got, info = _guide_step(eng, case, dev, eps)
    frac, lattice, t, off = _upload(case, dev)
    out = torch.as_tensor(eps, device=dev).clone()
    eng.contact_guidance_step(frac, lattice, t, off, out, case.params)
    assert _same_bytes(out.cpu().numpy(), got)
    zero, info0 = _guide_step(eng, case, dev, eps, cg.ContactGuidance(min_distance=case.params.min_distance, weight=0.0))
    assert np.array_equal(zero, eps) and all(_same_bytes(info[q], info0[q]) for q in cg.INFO_KEYS)


@pytest.mark.parametrize("which", ["mixed", "ragged", "seventy"])
def test_a_crystal_gives_the_same_bits_wherever_it_sits_in_the_batch(dev, fused_model, which):
    """`mixed` and `ragged`: the batch in another order.  `seventy`: its first crystal, its last and a 65-atom one launched alone
    (each at its own timestep) against their rows of the 70-crystal launch."""
    m, _ = fused_model
    eng = m.engine()
    if which == "seventy":
        base = cases.seventy_case()
        eps = np.random.RandomState(9).normal(size=base.frac.shape).astype(np.float32)
        got, info = _guide_step(eng, base, dev, eps)
        assert base.counts[34] == 65
        for b in (0, base.B - 1, 34):
            a, e = base.offsets[b], base.offsets[b + 1]
            alone, info_1 = _guide_step(eng, base.crystal(b), dev, eps[a:e])
            assert _same_bytes(alone, got[a:e]), b
            for q in cg.INFO_KEYS:
                assert info_1[q].tobytes() == info[q][b:b + 1].tobytes(), (b, q)
        assert info["contacts"][34] > 10 and not _same_bytes(got, eps)
        return
    base = cases.mixed_batch() if which == "mixed" else cases.ragged_case()
    order = [3, 5, 0, 4, 2, 1] if which == "mixed" else [4, 2, 0, 3, 1]
    moved = cases.batch_of("moved", [base], order)
    rng = np.random.RandomState(9)
    eps = rng.normal(size=base.frac.shape).astype(np.float32)
    eps_moved = np.concatenate([eps[base.offsets[b]:base.offsets[b + 1]] for b in order])
    got, info = _guide_step(eng, base, dev, eps)
    got_m, info_m = _guide_step(eng, moved, dev, eps_moved)
    for at, b in enumerate(order):
        assert _same_bytes(got_m[moved.offsets[at]:moved.offsets[at + 1]], got[base.offsets[b]:base.offsets[b + 1]]), (which, b)
        for q in cg.INFO_KEYS:
            assert info_m[q][at:at + 1].tobytes() == info[q][b:b + 1].tobytes(), (which, b, q)


def test_the_unstaged_path_gives_the_staged_path_s_bits(dev, fused_model):
    """`large` (257 atoms: positions formed from global memory at every use) against the same crystal without its last atom (256:
    staged in LDS).  The two share the cell, hence the image count M.  Lane l of atom i's wave walks e = l, l + 64, ... of
    e = j M + m in both, so it meets the same contacts in the same order; the extra range e in [256 M, 257 M) is atom 256, which is
    farther than d0 from everything and adds nothing to any sum (the CPU test asserts it).  Atom 256 belongs to wave 0, which adds
    wave_sum(0) = 0 to its energy after the last of its atoms: x + 0 is x.  So eps' of atoms 0..255, the energy and the contacts
    must be the same bytes, provided crystal_cart from global memory and from LDS are "the same values" as the kernel says."""
    m, _ = fused_model
    eng = m.engine()
    big, less = cases.large_case(), cases.large_case(n=256)
    assert big.counts == [257] and less.counts == [256] and np.array_equal(big.frac[:256], less.frac)
    eps = np.random.RandomState(11).normal(size=big.frac.shape).astype(np.float32)
    got, info = _guide_step(eng, big, dev, eps)
    got_less, info_less = _guide_step(eng, less, dev, eps[:256])
    assert _same_bytes(got[:256], got_less) and _same_bytes(got[256:], eps[256:])  # (the lone atom: eps + k 0)
    assert all(_same_bytes(info[q], info_less[q]) for q in cg.INFO_KEYS)
    assert info["contacts"][0] >= 300 and info["flags"][0] == 0 and not _same_bytes(got_less, eps[:256])
    eng.check_status()


def test_timesteps_outside_the_schedule_are_clamped_and_flagged(dev, fused_model):
    """`ragged` at t = [0, -3, T + 1, 5, T]: eps' is guided_eps at the clamped timesteps [1, 1, T, 5, T] within the bounds of
    test_step_matches_the_restatement and the same bytes as the launch at the clamped timesteps; STATUS_BAD_TIMESTEP is set by the
    first launch and not by the second."""
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    base = cases.ragged_case()
    bad = cases.GuidanceCase("bad t", base.frac, base.lattice, base.counts, base.params, t=cases.BAD_T)
    good = cases.GuidanceCase("clamped t", base.frac, base.lattice, base.counts, base.params, t=np.clip(cases.BAD_T, 1, T))
    ref = cg.reference(base.frac, base.lattice, base.offsets, base.params)
    sig = _sigmas(m)
    k = cg.sigma_coefficient(sig, bad.t, base.params.weight)
    assert np.array_equal(k, cg.sigma_coefficient(sig, good.t, base.params.weight)) and k[0] == k[1] != k[3]
    eps = np.random.RandomState(12).normal(size=base.frac.shape).astype(np.float32)
    eng.status(reset=True)
    got, info = _guide_step(eng, bad, dev, eps)
    assert eng.status(reset=True)["flags"] & _hip.STATUS_BAD_TIMESTEP
    clamped, info_c = _guide_step(eng, good, dev, eps)
    assert eng.status(reset=True)["flags"] == 0
    assert _same_bytes(got, clamped) and all(_same_bytes(info[q], info_c[q]) for q in cg.INFO_KEYS)
    want = cg.guided_eps(eps, ref, base.offsets, sig, bad.t, base.params)
    d0 = float(np.float32(base.params.min_distance))
    assert list(info["contacts"]) == list(ref.contacts) and not info["flags"].any()
    for b in range(base.B):
        a, e = base.offsets[b], base.offsets[b + 1]
        gb = cg.g_bound(d0, ref.d_min[b], base.lattice[b], ref.shells[b], int(ref.atom_contacts[a:e].max()))
        assert (np.abs(got[a:e].astype(np.float64) - want[a:e]) <= cg.eps_bound(k[b], gb, ref.g[a:e], want[a:e])).all(), b


@pytest.mark.parametrize("name", ["ragged", "large", "seventy"])
def test_the_device_s_forces_sum_to_zero(dev, fused_model, name):
    """Every contact pushes its two atoms with opposite forces, so sum_i D_i = sum_i g_i L = 0 in every unflagged crystal.  On the
    device's own numbers (g from a launch on eps = 0, divided by k = w / sigma_t^2): each g_i is within g_bound + 6 u max|g| of the
    exact one (g_bound; k in float32 and the product, as in test_step_matches_the_restatement), the exact ones sum to zero, so per
    Cartesian component d, |sum_i (g_i L)_d| <= n (g_bound + 6 u max|g|) sum_k |L_kd|.  The restatement supplies the bound's
    arguments alone (d_min, shells, contacts per atom): its pair enumeration is not what the sum is compared with."""
    m, _ = fused_model
    eng = m.engine()
    case = {c.name: c for c in [cases.ragged_case()] + cases.launch_cases()}[name]
    ref = cg.reference(case.frac, case.lattice, case.offsets, case.params)
    k = cg.sigma_coefficient(_sigmas(m), case.t, case.params.weight)
    d0 = float(np.float32(case.params.min_distance))
    g_dev, info = _guide_step(eng, case, dev, np.zeros_like(case.frac))
    checked = 0
    for b in range(case.B):
        a, e = case.offsets[b], case.offsets[b + 1]
        if info["flags"][b] & cg.SKIPPED or ref.ordered[b] == 0:
            assert not g_dev[a:e].any()
            continue
        L = case.lattice[b].astype(np.float64)
        g = g_dev[a:e].astype(np.float64) / k[b]
        gb = cg.g_bound(d0, ref.d_min[b], L, ref.shells[b], int(ref.atom_contacts[a:e].max()))
        total = np.abs((g @ L).sum(0))
        bound = (e - a) * (gb + 6 * cg.U32 * np.abs(g).max()) * np.abs(L).sum(0)
        print(f"{name}[{b}]: n {e - a}, |sum g L| {total.max():.3g} of bound {bound.min():.3g}, largest |g L| {np.abs(g @ L).max():.3g}")
        assert (total <= bound).all(), (b, total, bound)
        checked += 1
    assert checked >= {"ragged": 3, "large": 3, "seventy": 28}[name]
    eng.check_status()


# ------------------------------------------------------------------------------------------- the loop against its steps
def guided_scores(eng, state, an, off, t_c, info, params=GUIDE):
    """One evaluation as the guided loop makes it: predict_scores, then contact_guidance_step on the cell the evaluation saw
    (lattice_from_params of the state's lengths).  Returns (eps', logits, len0)."""
    f, ty, le = state[:3]
    eps, logits, len0 = eng.predict_scores(f, ty, le, an, t_c, off)
    eng.contact_guidance_step(f, lattice_from_params(le, an), t_c, off, eps, (params, info))
    return eps, logits, len0


def draws(eng, seed, t, B, N, word=0):
    """The loop's draws of timestep t, counter word `word`: z_lattice [B,3], z_frac [N,3], u_types [N,S]."""
    return (eng.philox_fill_word(seed, t, 0, word, 3 * B).view(B, 3), eng.philox_fill_word(seed, t, 1, word, 3 * N).view(N, 3),
            eng.philox_fill_word(seed, t, 2, word, N * S).view(N, S))


def chain(eng, start, an, off, steps, successors, step, corrector=False, seed=SEED):
    """predict_scores -> contact_guidance_step -> (corrector_step -> predict_scores -> contact_guidance_step ->) `step`, for every
    step, from a copy of `start` = (frac, types, lengths, lattice).  `step(state, t, s, t_c, s_c, scores)` calls the form's step
    export with its options on the state in place, fed the filled draws.  Returns the state and the info of the last evaluation."""
    state = tuple(x.clone() for x in start)
    B, N, dev = state[2].shape[0], state[0].shape[0], eng.device
    info = cg.allocate_info(B, dev)
    for t, s in zip(steps, successors):
        t_c, s_c = full_i32(B, t, dev), full_i32(B, s, dev)
        scores = guided_scores(eng, state, an, off, t_c, info)
        if corrector:
            eng.corrector_step(state[0], t_c, off, scores[0], eng.philox_fill_word(seed, t, 5, 0, 3 * N).view(N, 3), SNR)
            scores = guided_scores(eng, state, an, off, t_c, info)
        step(state, t, s, t_c, s_c, scores)
    return state, info


def _step_of(eng, case, form, seeds=None):
    """The step exports of the forms of test_guided_loop_is_its_steps_bit_for_bit."""
    B, N = case.B, case.N

    def step(state, t, s, t_c, s_c, scores):
        f, ty, le, lat = state
        if form == "keyed":
            z_l = eng.philox_fill_crystals(seeds, case.off, t, 0, per_crystal_width=3)
            z_f = eng.philox_fill_crystals(seeds, case.off, t, 1, per_atom_width=3)
            u_t = eng.philox_fill_crystals(seeds, case.off, t, 2, per_atom_width=S)
            eng.reverse_step_species(f, ty, le, case.an, t_c, s_c, case.off, *scores, z_l, z_f, u_t, lat, (None, 1.0), lattice_clipmax=CLIP)
            return
        z_l, z_f, u_t = (eng.philox_fill(SEED, t, 0, 3 * B).view(B, 3), eng.philox_fill(SEED, t, 1, 3 * N).view(N, 3),
                         eng.philox_fill(SEED, t, 2, N * S).view(N, S))
        if form == "respaced-eta0":
            eng.reverse_step_eta(f, ty, le, case.an, t_c, s_c, case.off, *scores, None, None, u_t, lat, 0.0, None, CLIP)
        else:
            eng.reverse_step(f, ty, le, case.an, t_c, case.off, *scores, z_l, z_f, u_t, lat)
    return step


def _chain(eng, case, form, steps, successors, seeds=None):
    return chain(eng, case.fresh(), case.an, case.off, steps, successors, _step_of(eng, case, form, seeds), corrector=form == "corrector")


@pytest.mark.parametrize("loop_prep", [None, "1"], ids=["no-prep", "prep-per-step"])
@pytest.mark.parametrize("form", ["plain", "respaced-eta0", "corrector", "keyed"])
def test_guided_loop_is_its_steps_bit_for_bit(dev, fused_model, form, loop_prep, monkeypatch):
    """Three steps of Engine.sample_loop(guidance=...) against the chain of exports, eager and with graph replay; the diagnostics of
    the last evaluation too.  The guidance is not idle: the unguided loop ends elsewhere."""
    if loop_prep is None:
        monkeypatch.delenv("ARREAU_LOOP_PREP", raising=False)
    else:
        monkeypatch.setenv("ARREAU_LOOP_PREP", loop_prep)
    m, _ = fused_model
    eng = m.engine()
    case = Batch(dev, seed=41)
    kw, seeds = {}, None
    if form in ("respaced-eta0", "keyed"):
        steps = [60, 30, 1]
        successors = steps[1:] + [0]
        kw.update(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP)
        if form == "respaced-eta0":
            kw.update(eta=0.0)
        else:
            seeds = torch.as_tensor(keyed.stream_seeds(SEED, [11, 4, 29]).view(np.int64), device=dev).contiguous()
            kw.update(crystal_seeds=seeds)
    else:
        steps = [60, 59, 58]
        successors = [59, 58, 57]
        if form == "corrector":
            kw.update(corrector=(1, SNR))
    want, want_info = _chain(eng, case, form, steps, successors, seeds)
    for use_graph in (False, True):
        got = case.fresh()
        info = cg.allocate_info(case.B, dev)
        eng.sample_loop(*got[:3], case.an, case.off, steps[0], len(steps), SEED, None, got[3], use_graph=use_graph, guidance=(GUIDE, info), **kw)
        assert_same_bits(got, want, (form, loop_prep, use_graph))
        assert_same_bits([info[q] for q in cg.INFO_KEYS], [want_info[q] for q in cg.INFO_KEYS], (form, "info", use_graph))
    plain = case.fresh()
    eng.sample_loop(*plain[:3], case.an, case.off, steps[0], len(steps), SEED, None, plain[3], **kw)
    assert not torch.equal(plain[0], want[0])
    eng.check_status()


def test_eager_equals_graph_replay_over_five_steps(dev, fused_model):
    m, _ = fused_model
    eng = m.engine()
    case = Batch(dev, seed=43)
    runs = []
    for use_graph in (False, True):
        got = case.fresh()
        info = cg.allocate_info(case.B, dev)
        eng.sample_loop(*got[:3], case.an, case.off, 40, 5, SEED, None, got[3], use_graph=use_graph, guidance=(GUIDE, info))
        runs.append(list(got) + [info[q] for q in cg.INFO_KEYS])
    assert_same_bits(runs[1], runs[0], "eager vs replay")
    eng.check_status()


def test_another_weight_on_the_same_buffers_is_not_a_stale_replay(dev, fused_model):
    """The parameters and the diagnostic pointers are part of the graph key: on the same buffers with use_graph every weight,
    min_distance and info array gives what the eager loop gives, and different weights give different states."""
    m, _ = fused_model
    eng = m.engine()
    case, k = Batch(dev, seed=47), 4
    bufs = case.fresh()
    infos = [cg.allocate_info(case.B, dev), cg.allocate_info(case.B, dev)]
    seen = []
    for params, which in ((GUIDE, 0), (cg.ContactGuidance(2.0, 0.1), 0), (cg.ContactGuidance(1.5, 0.1), 0), (cg.ContactGuidance(1.5, 0.1), 1),
                          (cg.ContactGuidance(1.5, 0.0), 1), (GUIDE, 0)):
        case.load(bufs)
        for q in cg.INFO_KEYS:
            infos[which][q].zero_()
        eng.sample_loop(*bufs[:3], case.an, case.off, 50, k, SEED, None, bufs[3], use_graph=True, guidance=(params, infos[which]))
        want = case.fresh()
        want_info = cg.allocate_info(case.B, dev)
        eng.sample_loop(*want[:3], case.an, case.off, 50, k, SEED, None, want[3], use_graph=False, guidance=(params, want_info))
        assert_same_bits(bufs, want, params)
        assert_same_bits([infos[which][q] for q in cg.INFO_KEYS], [want_info[q] for q in cg.INFO_KEYS], (params, "info"))
        seen.append(bufs[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and torch.equal(seen[2], seen[3])
    assert not torch.equal(seen[3], seen[4]) and torch.equal(seen[0], seen[5])
    # guidance with another option on the same buffers: multistep, a tie, neither, multistep again
    from arreau_amd.diffusion import multistep as ms
    steps = [60, 45, 30, 1]
    tie = torch.as_tensor([0, 1, 2], dtype=torch.int32, device=dev)
    kw = dict(next_table=respacing.next_table(T, steps).to(dev), lattice_clipmax=CLIP)
    hist = ms.allocate_history(case.N, case.B, dev)
    seen = []
    for option in ("multistep", "tie", None, "multistep"):
        more = lambda h: {"multistep": dict(multistep=h), "tie": dict(length_tie=tie), None: {}}[option]
        case.load(bufs)
        for q in ms.HISTORY_KEYS:
            hist[q].zero_()
        eng.sample_loop(*bufs[:3], case.an, case.off, steps[0], len(steps), SEED, None, bufs[3], use_graph=True, guidance=(GUIDE, infos[0]), **kw,
                        **more(hist))
        want, want_info, want_hist = case.fresh(), cg.allocate_info(case.B, dev), ms.allocate_history(case.N, case.B, dev)
        eng.sample_loop(*want[:3], case.an, case.off, steps[0], len(steps), SEED, None, want[3], use_graph=False, guidance=(GUIDE, want_info), **kw,
                        **more(want_hist))
        assert_same_bits(bufs, want, option)
        assert_same_bits([infos[0][q] for q in cg.INFO_KEYS], [want_info[q] for q in cg.INFO_KEYS], (option, "info"))
        if option == "multistep":
            assert_same_bits([hist[q] for q in ms.HISTORY_KEYS], [want_hist[q] for q in ms.HISTORY_KEYS], "history")
        seen.append([x.clone() for x in bufs])
    assert_same_bits(seen[3], seen[0], "multistep again")
    assert not torch.equal(seen[0][0], seen[2][0]) and not torch.equal(seen[1][2], seen[2][2]) and not torch.equal(seen[0][2], seen[1][2])
    eng.check_status()


# ------------------------------------------------------------------------------------------- the step identity
def test_isolated_pairs_end_at_min_distance_after_the_last_step(dev):
    """Three isolated 0.3 A pairs in one 6-atom crystal, eps = 0, guided with d0 = 0.5 and w = 0.5, then arreau_reverse_step_eta at
    eta = 0 from t = 1 to 0: every pair ends at d0 within the bound, and the screen counts no contact below d0 - bound.  The eta = 0
    step moves x by -eps sig_1 (sig_1 - sig_0); it lands on the clean-position estimate x - sig_1^2 eps, which is what guidance
    moves by -w g, where sig_0 = 0.  The geometric ladder of VE_pbc ends at sig_0 = sigma_min > 0 (there the last step covers
    1 - sig_0 / sig_1 of the way, a property of that step with or without guidance), so this test's model has its sig_0 set to 0.
    Distances are taken in the cell the evaluation saw (the step also replaces the lengths by its own prediction).  The bound: each
    of a pair's two atoms is off by at most the cell's largest row norm times sqrt(3) times (w g_bound + 8 u w |g| + 2 u): the
    gradient's bound, the four roundings from g to the move, and the rounding of the new coordinate (< 1)."""
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=S, seed=2, num_timesteps=T).to(dev)
    with torch.no_grad():
        m.diffusion_loss.pos_diffusion.sigmas[0] = 0.0
    eng = m.engine()
    params = cg.ContactGuidance()
    d0, w = 0.5, 0.5
    lengths = torch.tensor([[6.0, 6.5, 7.0]], device=dev)
    angles = torch.tensor([[1.4, 1.5, 1.6]], device=dev)
    lattice = lattice_from_params(lengths, angles)
    L = lattice[0].cpu().numpy().astype(np.float64)
    centres = np.array([[0.2, 0.2, 0.2], [0.5, 0.6, 0.3], [0.8, 0.3, 0.7]])
    dirs = np.array([[1.0, 0, 0], [1, 2, 2], [-2, 1, 2]])
    half = 0.15 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True) @ np.linalg.inv(L)  # 0.15 A either way, in fractions
    frac = torch.as_tensor(np.stack([centres - half, centres + half], 1).reshape(6, 3).astype(np.float32), device=dev).contiguous()
    off = torch.tensor([0, 6], dtype=torch.int32, device=dev)
    t_c, s_c = full_i32(1, 1, dev), full_i32(1, 0, dev)
    ref = cg.reference(frac.cpu().numpy(), lattice.cpu().numpy(), [0, 6], params)
    assert ref.contacts[0] == 3 and ref.flags[0] == 0 and np.allclose(ref.d[0], 0.3, atol=1e-5)
    eps = torch.zeros(6, 3, device=dev)
    eng.contact_guidance_step(frac, lattice, t_c, off, eps, params)
    types = torch.ones(6, dtype=torch.int32, device=dev)
    new_lattice = torch.zeros(1, 3, 3, device=dev)
    u_t = eng.philox_fill(SEED, 1, 2, 6 * S).view(6, S)
    eng.reverse_step_eta(frac, types, lengths.clone(), angles, t_c, s_c, off, eps, torch.zeros(6, S, device=dev), lengths.clone(), None, None,
                         u_t, new_lattice, 0.0, None, CLIP)
    x = frac.cpu().numpy().astype(np.float64)
    gb = cg.g_bound(d0, ref.d_min[0], L, ref.shells[0], 1)
    per_atom = np.linalg.norm(L, axis=1).max() * np.sqrt(3.0) * (w * gb + 8 * cg.U32 * w * np.abs(ref.g).max() + 2 * cg.U32)
    bound = 2 * per_atom
    for p in range(3):
        delta = x[2 * p + 1] - x[2 * p]
        d = np.linalg.norm((delta - np.rint(delta)) @ L)
        print(f"pair {p}: d = {d:.9f}, |d - d0| = {abs(d - d0):.3g} of bound {bound:.3g}")
        assert abs(d - d0) <= bound
    from arreau_amd.diffusion.screening import ScreenCriteria
    res = eng.screen(frac, lattice, off, None, ScreenCriteria(min_distance=d0 - bound, mask_type=None))
    assert int(res["n_close"][0]) == 0
    eng.check_status()


# ------------------------------------------------------------------------------------------- what must not change
def _arrays(res):
    return [np.asarray(getattr(res, k)).tobytes() for k in ("frac_x", "atomic_numbers", "lattice", "num_atoms")]


def test_none_and_weight_zero_are_the_sampler_as_it_was(dev, fused_model, monkeypatch):
    from arreau_amd import _hip
    m, _ = fused_model
    lib = _hip.lib()
    called = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("arreau_sample_loop") or name == "arreau_contact_guidance_step":
                called.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(_hip, "lib", lambda: Spy())

    def sample(**kw):  # (the initial state comes from the host's global generators: the same seeds in front of every call)
        torch.manual_seed(5)
        np.random.seed(5)
        return m.sample(Batch.COUNTS, 3, **kw)
    kw = dict(max_steps=4, seed=SEED)
    base = sample(**kw)
    none = sample(contact_guidance=None, **kw)
    assert set(called) == {"arreau_sample_loop"} and "contact_guidance" not in (none.info or {})
    called.clear()
    zero = sample(contact_guidance=cg.ContactGuidance(weight=0.0), **kw)
    guided = sample(contact_guidance=GUIDE, **kw)
    assert set(called) == {"arreau_sample_loop_guided"}
    monkeypatch.undo()
    assert _arrays(none) == _arrays(base) and _arrays(zero) == _arrays(base) and _arrays(guided) != _arrays(base)
    info = guided.info["contact_guidance"]
    assert set(info) == set(cg.INFO_KEYS) and info["contacts"].shape == (3,) and info["energy"].dtype == np.float32
    assert not zero.info["contact_guidance"]["contacts"].any()  # no launch wrote them
    # the host-noise modes run the same launch between the evaluation and the step
    dev_plain = sample(noise="device", max_steps=3)
    dev_zero = sample(noise="device", max_steps=3, contact_guidance=cg.ContactGuidance(weight=0.0))
    dev_guided = sample(noise="device", max_steps=3, contact_guidance=GUIDE)
    assert _arrays(dev_zero) == _arrays(dev_plain) and _arrays(dev_guided) != _arrays(dev_plain)
    assert set(dev_guided.info["contact_guidance"]) == set(cg.INFO_KEYS)


def test_null_struct_is_the_keyed_loop(dev, fused_model):
    """arreau_sample_loop_guided with a NULL struct, called directly, is arreau_sample_loop_keyed bit for bit."""
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    lib = _hip.lib()
    case = Batch(dev, seed=53)
    seeds = torch.as_tensor(keyed.stream_seeds(SEED, [1, 2, 3]).view(np.int64), device=dev).contiguous()
    want = case.fresh()
    eng.sample_loop(*want[:3], case.an, case.off, 30, 3, SEED, None, want[3], crystal_seeds=seeds)
    got = case.fresh()
    ws = eng.workspace(case.N, case.B)
    ctl = _hip.SpeciesControlC(None, 1.0)
    _hip.check(lib.arreau_sample_loop_guided(
        eng._handle, _hip.ptr(got[0]), _hip.ptr(got[1]), _hip.ptr(got[2]), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N, 30, 3, SEED,
        None, None, _hip.ptr(got[3]), _hip.ptr(ws), ws.numel(), 0, None, None, None, None, None, None, None, None, ctypes.byref(ctl),
        _hip.ptr(seeds), None, _hip.stream_ptr(dev)), "arreau_sample_loop_guided")
    assert_same_bits(got, want, "NULL struct")
    eng.check_status()


def test_rejections_leave_the_state_untouched(dev, fused_model):
    from arreau_amd import _hip
    m, _ = fused_model
    eng = m.engine()
    lib = _hip.lib()
    case = Batch(dev, seed=59)
    got = case.fresh()
    before = [t.clone() for t in got]
    ws = eng.workspace(case.N, case.B)
    ctl = _hip.SpeciesControlC(None, 1.0)
    eps = torch.randn(case.N, 3, device=dev)
    eps_before = eps.clone()
    lattice = lattice_from_params(got[2], case.an)
    t_c = full_i32(case.B, 10, dev)
    for d0, w, shells in ((0.0, 0.5, 8), (-1.0, 0.5, 8), (float("nan"), 0.5, 8), (float("inf"), 0.5, 8), (0.5, -0.1, 8), (0.5, float("nan"), 8),
                          (0.5, float("inf"), 8), (0.5, 0.5, 0), (0.5, 0.5, 9)):
        bad = _hip.ContactGuidanceC(d0, w, shells, None, None, None)
        rc = lib.arreau_sample_loop_guided(
            eng._handle, _hip.ptr(got[0]), _hip.ptr(got[1]), _hip.ptr(got[2]), _hip.ptr(case.an), _hip.ptr(case.off), case.B, case.N, 30, 3,
            SEED, None, None, _hip.ptr(got[3]), _hip.ptr(ws), ws.numel(), 0, None, None, None, None, None, None, None, None, ctypes.byref(ctl),
            None, ctypes.byref(bad), _hip.stream_ptr(dev))
        assert rc == -1 and b"guidance" in lib.arreau_last_error(), (d0, w, shells)
        rc = lib.arreau_contact_guidance_step(eng._handle, _hip.ptr(got[0]), _hip.ptr(lattice), _hip.ptr(t_c), _hip.ptr(case.off), case.B, case.N,
                                              _hip.ptr(eps), ctypes.byref(bad), _hip.stream_ptr(dev))
        assert rc == -1, (d0, w, shells)
    rc = lib.arreau_contact_guidance_step(eng._handle, _hip.ptr(got[0]), _hip.ptr(lattice), _hip.ptr(t_c), _hip.ptr(case.off), case.B, case.N,
                                          _hip.ptr(eps), None, _hip.stream_ptr(dev))
    assert rc == -1
    torch.cuda.synchronize(dev)
    assert_same_bits(got, before, "rejected loop")
    assert torch.equal(eps, eps_before)
    # the Python layers: a bad value and an inversion, before any work
    with pytest.raises(ValueError):
        eng.sample_loop(*got[:3], case.an, case.off, 30, 3, SEED, None, got[3], guidance=(0.5, 0.5))
    with pytest.raises(ValueError, match="contact_guidance must be"):
        m.sample(Batch.COUNTS, 3, max_steps=2, contact_guidance=0.5)
    crystals = m.sample(Batch.COUNTS, 3, max_steps=2, seed=SEED)
    with pytest.raises(ValueError, match="inversion"):
        m.encode(crystals, t=10, contact_guidance=GUIDE)
    assert_same_bits(got, before, "rejected calls")
    eng.check_status()
