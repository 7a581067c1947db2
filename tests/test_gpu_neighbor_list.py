"""The periodic neighbour list on the device against its float32 restatement (tests/neighbor_reference.py: `select`), on the
inputs where a selection goes wrong without a rounding error to show for it: exactly symmetric crystals (float32 ties in d^2 at
the top-k cut, broken by the enumeration index), every selection path of the kernel -- register-resident keys, the LDS list, the
re-evaluating rounds; positions staged in LDS or read from global memory -- degenerate geometry, skewed and sampler-like cells,
k = 1 .. 64 and three radii.  Counts, senders and image cells are compared exactly, directions and distances BIT FOR BIT: the
kernel evaluates ((cx L0 + cy L1) + cz L2), (p_j + off) - p_i, (dx^2 + dy^2) + dz^2 and the square root with correctly rounded
float32 operations and no contraction, and so does numpy.  test_neighbor_reference_cpu.py proves on the CPU which path each
input takes and that the restatement is the oracle with a stable sort.  Then the two other forms of the same device code -- the
one predict_scores launches (atom -> crystal map) and the one the sampling loop launches (positions formed from fractional
coordinates) -- against the stand-alone form, and the network and a six-step free-running trajectory on symmetric crystals against the oracle.
Needs an MI355X: `-m gpu`."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sampler as OS
from tests import neighbor_reference as NR
from tests.helpers import assert_scores_close, oracle_from_module, random_state
from tests.sampling_helpers import assert_same_bits, dev  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in NR.cases()}


@pytest.fixture(scope="module")
def small_model(dev):
    """S = 12, T = 100 synthetic checkpoint in the reference layout (C = 128, D = 256, L = 5; radius 5, k = 8)."""
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=12, seed=1234, num_timesteps=100).to(dev)
    return m, oracle_from_module(m, torch.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def device_list(dev, cart, lattice, counts, radius, k):
    """The stand-alone entry point (arreau_radius_graph_pbc + arreau_compact_edges) -> numpy."""
    from arreau_amd.diffusion.diffusion_helpers import radius_graph_pbc
    out = radius_graph_pbc(torch.as_tensor(cart).to(dev), torch.as_tensor(lattice).to(dev), torch.tensor(counts), float(radius), int(k))
    return tuple(v.cpu().numpy() for v in out)


def assert_is_select(got, sel, counts, what):
    """Counts, edge index and image cells exactly; dir and dist bitwise."""
    ei, cells, per_crystal, dist, direction = got
    w_ei, w_cells, w_dist, w_dir = NR.to_edges(sel)
    first = np.concatenate([[0], np.cumsum(counts)])
    assert per_crystal.tolist() == [int(sel.deg[first[b]:first[b + 1]].sum()) for b in range(len(counts))], what
    assert np.array_equal(ei, w_ei), (what, "edge index")
    assert np.array_equal(cells, w_cells), (what, "image cells")
    assert same_bits(direction, w_dir), (what, "dir", int((direction.view(np.uint32) != w_dir.view(np.uint32)).sum()))
    assert same_bits(dist, w_dist), (what, "dist", int((dist.view(np.uint32) != w_dist.view(np.uint32)).sum()))


# ------------------------------------------------------------------------------------------------ the stand-alone list
SMALL = [n for n in CASES if not n.startswith("fallback")]


@pytest.mark.parametrize("name", SMALL)
def test_list_is_the_restatement(dev, name):
    """Symmetric crystals (rock salt, fcc, hcp, R-3m 3a+3b, Pnma 4c, simple-cubic 3^3 / 4^3 / 6^3, general positions of one
    group per lattice system), degenerate geometry (d^2 == r^2, a 2 A cell, both sides of the self-edge threshold, coincident
    atoms, a lone atom) and skewed / sampler-like cells, at the model's radius 5 and k = 8."""
    case = CASES[name]
    sel = NR.select(case.cart, case.lattice, case.counts, case.radius, case.k)
    if name == "self_edge_threshold":
        assert sel.deg.tolist() == [0, 0, 1, 1]  # the restatement decides the side; both sides occur
    assert_is_select(device_list(dev, case.cart, case.lattice, case.counts, case.radius, case.k), sel, case.counts, name)


@pytest.mark.parametrize("radius", NR.SWEEP_RADIUS)
@pytest.mark.parametrize("k", NR.SWEEP_K)
def test_every_k_and_three_radii_on_a_ragged_batch(dev, k, radius):
    """k from 1 to the entry point's limit of 64 (above 8, `count < k` is the common state of a receiver; at 64 every lane
    holds a selection) on rock salt + random crystals of 20, 40 and 150 atoms."""
    case = CASES["mixed"]
    sel = NR.select(case.cart, case.lattice, case.counts, radius, k)
    if k >= 13 and radius == 2.5:
        assert (sel.deg < k).any() and (sel.deg > 8).any()  # (of the input: receivers short of k, others beyond the model's 8)
    assert_is_select(device_list(dev, case.cart, case.lattice, case.counts, radius, k), sel, case.counts, (k, radius))


@pytest.mark.parametrize("name", ["fallback_no_threshold", "fallback_finite_threshold"])
def test_the_re_evaluating_rounds_and_the_scan_carry(dev, name):
    """A crystal of 3712 atoms whose 406-atom cluster offers the LDS list more than its 384 entries (proved by emulation in
    test_neighbor_reference_cpu.py), without a threshold and with one.  N > 1024 receivers also take the edge-offset scan of
    arreau_compact_edges past one chunk.  EVERY receiver is compared: the restatement of one crystal takes a few seconds."""
    case = CASES[name]
    t0 = time.time()
    sel = NR.select(case.cart, case.lattice, case.counts, case.radius, case.k)
    print(f"\n[{name}] restatement of {len(sel.deg)} receivers: {time.time() - t0:.1f} s")
    assert int(sel.deg[1024:].sum()) > 0  # (edges beyond the scan's first chunk)
    assert_is_select(device_list(dev, case.cart, case.lattice, case.counts, case.radius, case.k), sel, case.counts, name)


# ------------------------------------------------------------------------------------------------ the other two forms
def _states():
    """name -> (frac, types, lengths, angles, num_atoms) on the CPU: the symmetric batch and two ragged ones."""
    frac, lengths, angles, counts = NR.symmetric_state()
    types = torch.tensor(np.random.RandomState(4).randint(0, 12, len(frac)))
    out = {"symmetric": (torch.from_numpy(frac), types, torch.from_numpy(lengths), torch.from_numpy(angles), torch.tensor(counts))}
    out["ragged"] = random_state(12, [20, 5, 8, 40, 130], 9)
    out["ragged sampler-like"] = random_state(12, [20, 5, 8, 40, 130], 9, sampler_like=True)
    return out


def _on_device(dev, state):
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    frac, types, lengths, angles, na = state
    d = lambda v: v.to(dev).contiguous()
    return d(frac), d(types.to(torch.int32)), d(lengths), d(angles), crystal_offsets(na, dev)


@pytest.mark.parametrize("which", ["symmetric", "ragged", "ragged sampler-like"])
def test_slot_form_of_predict_scores_is_the_stand_alone_list(dev, small_model, which):
    """predict_scores(return_edges=True) runs neighbor_embed_kernel<false>, which finds the receiver's crystal in the atom ->
    crystal map where the stand-alone kernel searches the offsets: deg, src, dir and dist bitwise those of the stand-alone
    list built on the device's own lattice_from_params / frac_to_cart_coords (and of the restatement on these), unused slots
    cleared."""
    from arreau_amd.diffusion.diffusion_helpers import frac_to_cart_coords, radius_graph_pbc_slots
    from arreau_amd.diffusion.lattice_helpers import lattice_from_params
    m, _ = small_model
    eng = m.engine()
    state = _states()[which]
    na = state[4]
    f, ty, le, an, off = _on_device(dev, state)
    t_c = torch.full((len(na),), 50, device=dev, dtype=torch.int32)
    *_, (deg, src, sdir, sdist) = eng.predict_scores(f, ty, le, an, t_c, off, return_edges=True)
    lattice = lattice_from_params(le, an)
    cart = frac_to_cart_coords(f, lattice, na)
    a_deg, a_src, _cell, a_dir, a_dist, _off = radius_graph_pbc_slots(cart, lattice, na, 5.0, eng.k)
    assert_same_bits((deg, src, sdir, sdist), (a_deg, a_src, a_dir, a_dist), which, nan_ok=False)
    unused = torch.arange(eng.k, device=dev)[None, :] >= deg[:, None]
    assert bool((src[unused] == -1).all()) and bool((sdir[unused] == 0).all()) and bool((sdist[unused] == 0).all())
    sel = NR.select(cart.cpu().numpy(), lattice.cpu().numpy(), na.tolist(), 5.0, eng.k)
    assert np.array_equal(deg.cpu().numpy(), sel.deg) and np.array_equal(src.cpu().numpy(), sel.src)
    assert same_bits(sdir.cpu().numpy(), sel.dir) and same_bits(sdist.cpu().numpy(), sel.dist)
    if which == "symmetric":
        assert NR.diagnose(cart.cpu().numpy(), lattice.cpu().numpy(), na.tolist(), 5.0, eng.k).tied.sum() >= 32  # (the device's cos(pi/2) is not 0: the cells are a hair off cubic, most ties survive)
    eng.check_status()


def test_loop_form_breaks_ties_like_the_per_step_path(dev, small_model):
    """sample_loop runs neighbor_embed_kernel<true>, which forms the positions from the fractional coordinates itself.  On rock
    salt, sc 4^3 and sc 6^3 -- ties at the cut of nearly every receiver in the first step -- 1 and 3 steps leave bitwise the
    state of the per-step entry points fed the same Philox draws, eager and replayed: a tie broken differently between the two
    forms would select other edges and change the scores."""
    m, _ = small_model
    eng = m.engine()
    S, seed, T = 12, 192837465, 100
    state = _states()["symmetric"]
    B, N = len(state[4]), state[0].shape[0]
    f0, ty0, le0, an, off = _on_device(dev, state)

    def fresh():
        return f0.clone(), ty0.clone(), le0.clone(), torch.zeros(B, 3, 3, device=dev)

    f, ty, le, lat = fresh()
    states = []
    for t in range(T - 1, T - 4, -1):
        t_c = torch.full((B,), t, device=dev, dtype=torch.int32)
        eps, logits, len0 = eng.predict_scores(f, ty, le, an, t_c, off)
        z_l = eng.philox_fill(seed, t, 0, 3 * B).view(B, 3)
        z_f = eng.philox_fill(seed, t, 1, 3 * N).view(N, 3)
        u_t = eng.philox_fill(seed, t, 2, N * S).view(N, S)
        eng.reverse_step(f, ty, le, an, t_c, off, eps, logits, len0, z_l, z_f, u_t, lat)
        states.append((f.clone(), ty.clone(), le.clone(), lat.clone()))
    for use_graph in (False, True):
        for n_steps in (1, 3):
            got = fresh()
            eng.sample_loop(got[0], got[1], got[2], an, off, T - 1, n_steps, seed, None, got[3], use_graph=use_graph)
            assert_same_bits(got, states[n_steps - 1], (use_graph, n_steps))
    eng.check_status()


def test_network_on_symmetric_crystals(dev, small_model):
    """predict_scores with its own neighbour list on rock salt + sc 4^3 + sc 6^3 against the float32 oracle teacher-forced
    with the restatement's edges, at the suite's bound (assert_scores_close)."""
    from arreau_amd.diffusion.diffusion_helpers import frac_to_cart_coords
    from arreau_amd.diffusion.lattice_helpers import lattice_from_params
    m, om32 = small_model
    eng = m.engine()
    state = _states()["symmetric"]
    frac, types, lengths, angles, na = state
    f, ty, le, an, off = _on_device(dev, state)
    lattice = lattice_from_params(le, an)
    cart = frac_to_cart_coords(f, lattice, na)
    sel = NR.select(cart.cpu().numpy(), lattice.cpu().numpy(), na.tolist(), 5.0, eng.k)
    assert NR.diagnose(cart.cpu().numpy(), lattice.cpu().numpy(), na.tolist(), 5.0, eng.k).tied.sum() >= 32
    ei, _cells, dist, direction = (torch.from_numpy(np.ascontiguousarray(v)) for v in NR.to_edges(sel))
    B, N, t = len(na), frac.shape[0], 40
    batch = torch.arange(B).repeat_interleave(na)
    want = OS.predict_scores(om32, frac, F.one_hot(types, 12), torch.full((N,), t), na, lengths, angles, batch, edges=(ei, dist, direction))
    got = eng.predict_scores(f, ty, le, an, torch.full((B,), t, device=dev, dtype=torch.int32), off)
    assert_scores_close(got, want, "symmetric batch", atoms_per_crystal=int(na.max()))
    eng.check_status()


TRAJECTORY_SEED = 3


def test_free_running_trajectory_from_a_symmetric_state(dev, small_model):
    """Six free-running steps (own neighbour list in every step, reference noise: randn[B,3], randn[N,3], rand[N,S] from the
    global CPU generator in the reference's order) from the state sample(symmetry=rock salt, cubic) starts in -- three crystals
    on the template's sites, all species masked, tied N(0,1) lengths, right angles in radians -- against the oracle's sampler
    with stable_ties=True, at the tolerance of test_free_running_sampler_matches_oracle_sampler.  In so small cells every
    receiver of the first step, and some of the later ones, has an exact tie at the cut: the oracle follows the kernel's rule
    through them.  A NEAR-tie (relative float64 gap at the cut below 1e-5 without an exact float32 tie) may legitimately be
    resolved differently: the seed is chosen so that the oracle's trajectory has none in the six steps, which is asserted."""
    from oracle import geometry as OG
    m, om32 = small_model
    eng = m.engine()
    B, n, S, T, steps = 3, 8, 12, 100, 6
    N = B * n
    torch.manual_seed(TRAJECTORY_SEED)
    lengths = torch.randn(B, 1).repeat(1, 3)
    frac = torch.from_numpy(np.tile(NR.ROCK_SALT, (B, 1)).astype(np.float32))
    state = (frac, torch.full((N,), S - 1), lengths, torch.full((B, 3), float(np.pi / 2)), torch.full((B,), n))
    trace = OS.SampleTrace()
    noise_rng = torch.random.get_rng_state()  # (the same draws for the oracle and for the device leg)
    f_o, ty_o, len_o, lat_o = OS.sample(om32, n, B, torch.float32, trace=trace, max_steps=steps, state=state, stable_ties=True)
    assert len(trace.steps) == steps
    exact = 0
    for step in trace.steps:
        lat = OG.lattice_from_params(step["lengths"], state[3])
        cart = OG.frac_to_cart_coords(step["frac"], lat, state[4])
        about = NR.diagnose(cart.numpy(), lat.numpy(), [n] * B, 5.0, eng.k)
        assert not ((about.gap < 1e-5) & ~about.tied).any(), step["t"]
        exact += int(about.tied.sum())
    assert exact >= N  # (the first step: every receiver)
    f, ty, le, an, off = _on_device(dev, state)
    lat_d = torch.zeros(B, 3, 3, device=dev)
    torch.random.set_rng_state(noise_rng)
    for t in range(T - 1, T - 1 - steps, -1):
        t_c = torch.full((B,), t, device=dev, dtype=torch.int32)
        eps, logits, len0 = eng.predict_scores(f, ty, le, an, t_c, off)
        z_l, z_f, u_t = torch.randn(B, 3), torch.randn(N, 3), torch.rand(N, S)
        eng.reverse_step(f, ty, le, an, t_c, off, eps, logits, len0, z_l.to(dev), z_f.to(dev), u_t.to(dev), lat_d)
    eng.check_status()
    df = np.abs(f.cpu().numpy().astype(np.float64) - f_o.numpy().astype(np.float64))
    df = np.minimum(df, 1 - df)
    print(f"\n[trajectory] frac: 0.9 quantile {np.quantile(df, 0.9):.2e}, max {df.max():.2e}; types differing {int((ty.cpu().long() != ty_o).sum())}")
    assert np.quantile(df, 0.9) <= 1e-5 and df.max() <= 1e-2, (np.quantile(df, 0.9), df.max())
    np.testing.assert_allclose(lat_d.cpu().numpy(), lat_o.numpy(), atol=1e-3 * max(1.0, float(lat_o.abs().max())), rtol=0)
    assert int((ty.cpu().long() != ty_o).sum()) <= 1
