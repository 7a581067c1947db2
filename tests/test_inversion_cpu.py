"""Starting the sampler from given crystals, the host side (no GPU): the float64 restatements of the inversion step
(arreau_amd/diffusion/inversion.py; rules in include/arreau_hip.h) against the eta = 0 step they invert, the ascending table of an
inversion loop, the `top` of the respacing helpers, what sample(initial_state=...) rejects before any work, and generate.py's
--start_from flags."""
import numpy as np
import pytest

from arreau_amd.diffusion import ddim, inversion as iv, respacing
from oracle import diffusion as OD

T = 100
CLIP = 0.999
PAIRS = [(1, 2), (1, 99), (10, 50), (98, 99)]


def _tables():
    """The model's float32 tables, held as float64 (what the device reads, without further rounding)."""
    import torch
    sig = OD.ve_sigmas(T, 0.001, 1.0, dtype=torch.float32).double().numpy()
    ab, betas, _ = OD.vp_schedule(T, dtype=torch.float32)
    return sig, ab.double().numpy(), betas.double().numpy()


def _wrapped(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return np.minimum(d, 1.0 - d)


# ------------------------------------------------------------------------------------------------- 1. restatement algebra
@pytest.mark.parametrize("s,t", PAIRS)
def test_the_eta_zero_step_undoes_the_inversion_step(s, t):
    """The identity of the header section: the eta = 0 reverse step t -> s fed eps sig_s / sig_t and the same x0 returns the
    start.  Lengths: relative to rho (|l| + |x0|), the size of the terms that cancel."""
    sig, ab, betas = _tables()
    rng = np.random.RandomState(10 * s + t)
    x, eps = rng.rand(9, 3), rng.randn(9, 3) * 0.3
    x[:3] = [[1e-9, 1 - 1e-9, 0.5], [0.0, 0.999999, 1e-4], [0.25, 0.75, 1 - 1e-12]]
    L, x0 = rng.rand(4, 3) * 5 + 1, rng.rand(4, 3) * 7 + 1
    x_t = iv.invert_positions(sig, x, eps, s, t)
    assert ((x_t >= 0) & (x_t <= 1)).all()
    back = ddim.ve_step(sig, x_t, eps * sig[s] / sig[t], t, s, None, 0.0)
    assert _wrapped(back, x).max() <= 1e-12
    l_t = iv.invert_lengths(ab, L, x0, s, t)
    l_back = ddim.length_step(ab, betas, l_t, x0, t, s, None, 0.0, CLIP)
    assert (np.abs(l_back - L) <= 1e-12 * iv.invert_rho(ab, s, t) * (np.abs(L) + np.abs(x0))).all()
    assert np.abs(l_back - L).max() <= 1e-12 * 8  # and outright, at these magnitudes


def test_unit_steps_compose_to_the_one_jump_form():
    """t = s + 1 over all levels with a constant x0 and a constant direction eps sig (= d): the lengths land where the jump
    1 -> T lands, the positions at x + d (sig_T - sig_1)."""
    sig, ab, _ = _tables()
    rng = np.random.RandomState(3)
    x, d = rng.rand(6, 3), rng.randn(6, 3) * 0.2
    L, x0 = rng.rand(3, 3) * 5 + 1, rng.rand(3, 3) * 7 + 1
    xs, ls, shift = x.copy(), L.copy(), np.zeros_like(x)
    for s in range(1, T):
        xs = iv.invert_positions(sig, xs, d / sig[s], s, s + 1)
        ls = iv.invert_lengths(ab, ls, x0, s, s + 1)
        shift += d * (sig[s + 1] - sig[s])
    assert _wrapped(xs, np.remainder(x + d * (sig[T] - sig[1]), 1.0)).max() <= 1e-12
    assert _wrapped(xs, iv.invert_positions(sig, x, d / sig[1], 1, T)).max() <= 1e-12
    one = iv.invert_lengths(ab, L, x0, 1, T)
    assert (np.abs(ls - one) <= 1e-12 * iv.invert_rho(ab, 1, T) * (np.abs(L) + np.abs(x0))).all()


def test_rho_and_the_length_bound():
    _, ab, _ = _tables()
    assert 60 < iv.invert_rho(ab, 1, 99) < 66  # the factor the header names for T = 100
    assert iv.invert_rho(ab, 98, 99) > 1.0
    l, x0 = np.array([[2.0, -3.0, 0.0]]), np.array([[1.0, 1.0, 4.0]])
    b = iv.length_error_bound(ab, l, x0, 1, 99)
    want = iv.LENGTH_BOUND_ROUNDINGS * 2.0 ** -24 * iv.invert_rho(ab, 1, 99) * np.array([[3.0, 4.0, 4.0]])
    assert np.allclose(b, want, rtol=1e-15) and (b > 1e-5 * 0.1).all()  # not a flat 1e-5 of O(1) lengths
    # the bound holds for the restatement evaluated in float32, operation by operation
    rng = np.random.RandomState(0)
    f = np.float32
    for s, t in PAIRS:
        L, X0 = rng.randn(50, 3).astype(f) * 3, (rng.rand(50, 3) * 7).astype(f)
        a_s, a_t = f(ab[s]), f(ab[t])
        rho = np.sqrt((f(1) - a_t) / (f(1) - a_s), dtype=f)
        got = np.sqrt(a_t, dtype=f) * X0 + rho * (L - np.sqrt(a_s, dtype=f) * X0)
        assert got.dtype == f
        err = np.abs(got.astype(np.float64) - iv.invert_lengths(ab, L, X0, s, t))
        assert (err <= iv.length_error_bound(ab, L, X0, s, t)).all(), (s, t)


# ------------------------------------------------------------------------------------------------- 2. tables and schedules
def test_ascending_table():
    levels = [1, 2, 3, 10, 50, 99]
    up = iv.ascending_table(T, levels)
    assert up.dtype == np.int32 and up.shape == (T + 1,)
    for a, b in zip(levels, levels[1:]):
        assert up[a] == b
    for u in levels:
        assert up[u - 1] == u  # the "one below" entry of every level: a call may enter at any of them
    assert up[levels[-1]] == 0
    assert sorted(np.flatnonzero(up).tolist()) == [0, 1, 2, 3, 9, 10, 49, 50, 98]
    up = iv.ascending_table(T, [40, 41, 100])
    assert up[39] == 40 and up[40] == 41 and up[41] == 100
    assert iv.ascending_table(T, [7])[6] == 7  # no climb: only the entry


@pytest.mark.parametrize("levels", [[3, 2], [1, 1, 2], [0, 1], [1, T + 1], [1, 2.0], [1, True], [], 5, [1.5, 2], ["1", "2"]])
def test_ascending_table_rejects(levels):
    with pytest.raises(ValueError, match="levels"):
        iv.ascending_table(T, levels)


def _formula(top, K):
    """The docstring's formula, with top in the place of T-1: round-half-up of i (top-1) / (K-1) below top."""
    return [top - int(np.floor(i * (top - 1) / (K - 1) + 0.5)) for i in range(K)]


def test_respacing_with_a_top():
    for K in (2, 5, 7, 40):
        ts = respacing.respaced_timesteps(T, K, top=40)
        assert ts == _formula(40, K) and ts[0] == 40 and ts[-1] == 1 and len(ts) == K
        assert all(a > b for a, b in zip(ts, ts[1:]))
    assert respacing.respaced_timesteps(T, 40, top=40) == list(range(40, 0, -1))
    # the default top: what it was
    for T_, K in ((100, 10), (100, 99), (1000, 50), (30, 2), (100, 7)):
        assert respacing.respaced_timesteps(T_, K) == _formula(T_ - 1, K) == respacing.respaced_timesteps(T_, K, top=T_ - 1)
    assert respacing.resolve_schedule(T, num_steps=5, top=40) == _formula(40, 5)
    assert respacing.resolve_schedule(T, timesteps=[40, 7, 1], top=40) == [40, 7, 1]
    assert respacing.resolve_schedule(T, top=40) is None
    for bad in (dict(num_steps=41, top=40), dict(num_steps=5, top=0), dict(num_steps=5, top=T), dict(num_steps=5, top=2.5),
                dict(timesteps=[41, 1], top=40)):
        with pytest.raises(ValueError):
            respacing.resolve_schedule(T, **bad)


def test_encode_levels_are_the_decode_schedule_reversed():
    assert iv.encode_levels(T) == list(range(1, T))
    assert iv.encode_levels(T, t=5) == [1, 2, 3, 4, 5]
    assert iv.encode_levels(T, num_steps=8) == respacing.respaced_timesteps(T, 8)[::-1]
    assert iv.encode_levels(T, t=40, num_steps=5) == iv.schedule_from(T, 40, num_steps=5)[::-1]
    assert iv.encode_levels(T, timesteps=[50, 10, 3, 1]) == [1, 3, 10, 50]
    for bad in (dict(t=0), dict(t=T), dict(t=40, timesteps=[30, 1]), dict(t=40, num_steps=41), dict(num_steps=3, timesteps=[5, 1])):
        with pytest.raises(ValueError):
            iv.encode_levels(T, **bad)


# ------------------------------------------------------------------------------------------------- 3. rejections
class NoEngine:
    def engine(self):
        raise AssertionError("the engine was touched")


def _dl():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = T
    return dl


def _state(t=40, counts=(3, 2)):
    na = np.asarray(counts, dtype=np.int64)
    N, B = int(na.sum()), len(na)
    rng = np.random.RandomState(1)
    return iv.SamplerState(frac_x=rng.rand(N, 3), species=rng.randint(0, 4, N), lengths=rng.rand(B, 3) + 3,
                           angles=np.full((B, 3), np.pi / 2), num_atoms=na, t=t)


def _rng_states():
    import torch
    return np.random.get_state()[1].copy(), torch.random.get_rng_state().clone()


def _assert_nothing_drawn(before):
    import torch
    assert np.array_equal(np.random.get_state()[1], before[0]) and torch.equal(torch.random.get_rng_state(), before[1])


def test_sample_rejects_initial_state_combinations_before_any_work():
    from arreau_amd.diffusion import symmetry as sy
    from arreau_amd.diffusion.conditioning import SampleCondition
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    gen = sy.SymmetrySpec.general_positions(["-x,y+1/2,-z+1/2", "-x,-y,-z"], 2, "monoclinic")
    tmpl = SampleResult(frac_x=np.zeros((5, 3)), atomic_numbers=np.ones(5), lattice=np.tile(np.eye(3) * 4, (2, 1, 1)),
                        num_atoms=np.array([3, 2]), idx_start=np.array([0, 3]))
    cond = SampleCondition.from_sample_result(tmpl, fix_positions=True)
    before = _rng_states()
    kw = dict(model=NoEngine(), z_table=list(range(5)))
    for extra, match in ((dict(condition=cond), "condition="), (dict(symmetry=gen), "symmetry="),
                         (dict(symmetry=[gen, None]), "symmetry="), (dict(lattice_system="cubic"), "lattice_system="),
                         (dict(lattice_system=["cubic", None]), "lattice_system="),
                         (dict(condition=cond, lattice_system="cubic"), "condition=, lattice_system=")):
        for noise in ("philox", "reference", "device"):
            with pytest.raises(ValueError, match="initial_state= is not combined with " + match):
                _dl().sample(initial_state=_state(), noise=noise, **extra, **kw)
    # a level outside 1..T-1, and not an integer
    for t in (0, T, -3, T + 5, 2.0, "7", True, None):
        with pytest.raises(ValueError, match="initial_state.t"):
            _dl().sample(initial_state=_state(t=t), **kw)
    # a batch that disagrees
    for extra in (dict(num_samples_in_batch=3), dict(num_atoms_per_sample=3), dict(num_atoms_per_sample=[3, 3]),
                  dict(num_atoms_per_sample=[3, 2, 1]), dict(num_atoms_per_sample=[2, 3], num_samples_in_batch=2)):
        with pytest.raises(ValueError, match="disagrees with the initial state"):
            _dl().sample(initial_state=_state(), **extra, **kw)
    # arrays that disagree with each other, species out of range, something that is no state
    s = _state()
    s.frac_x = s.frac_x[:-1]
    with pytest.raises(ValueError, match="frac_x must have shape"):
        _dl().sample(initial_state=s, **kw)
    s = _state()
    s.species = s.species + 5
    with pytest.raises(ValueError, match="species"):
        _dl().sample(initial_state=s, **kw)
    with pytest.raises(ValueError, match="SamplerState"):
        _dl().sample(initial_state=dict(t=3), **kw)
    # a schedule that does not fit the level
    for extra in (dict(num_steps=41), dict(timesteps=[30, 1]), dict(timesteps=[50, 40, 1]), dict(num_steps=5, timesteps=[40, 1])):
        with pytest.raises(ValueError):
            _dl().sample(initial_state=_state(), **extra, **kw)
    _assert_nothing_drawn(before)
    # what is accepted reaches the engine: the state alone, with agreeing counts, with a schedule from its level
    for extra in ({}, dict(num_atoms_per_sample=[3, 2], num_samples_in_batch=2), dict(num_steps=5), dict(timesteps=[40, 7, 1]),
                  dict(eta=0.0, corrector_steps=1, resample_passes=2, fixed_cell=True)):
        with pytest.raises(AssertionError, match="engine was touched"):
            _dl().sample(initial_state=_state(), **extra, **kw)
    with pytest.raises(AssertionError, match="engine was touched"):
        _dl().sample(initial_state=_state(counts=(4, 4)), num_atoms_per_sample=4, **kw)
    _assert_nothing_drawn(before)


def test_wrapper_validates_before_sampling():
    from arreau_amd.checkpoint import make_synthetic_model
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    m = make_synthetic_model(S=12, seed=1, num_timesteps=30)
    m.engine = NoEngine().engine
    before = _rng_states()
    with pytest.raises(ValueError, match="initial_state.t"):
        m.sample(initial_state=_state(t=30))
    with pytest.raises(ValueError, match="lattice_system="):
        m.sample(initial_state=_state(t=20), lattice_system="cubic")
    with pytest.raises(ValueError, match="num_steps"):
        m.sample(initial_state=_state(t=20), num_steps=21)
    zs = m.z_table_zs.tolist()
    crystals = SampleResult(frac_x=np.random.RandomState(0).rand(5, 3), atomic_numbers=np.array([zs[0], zs[1], zs[2], zs[0], zs[3]], dtype=float),
                            lattice=np.tile(np.diag([3.0, 4.0, 5.0]), (2, 1, 1)), num_atoms=np.array([3, 2]))
    for t in (0, 30, 2.5):
        with pytest.raises(ValueError, match="t must be"):
            m.noise_to(crystals, t)
        with pytest.raises(ValueError, match="t must be"):
            m.encode(crystals, t=t)
    with pytest.raises(ValueError, match="num_steps"):
        m.encode(crystals, t=10, num_steps=11)
    with pytest.raises(ValueError, match="unknown lattice system"):
        m.noise_to(crystals, 10, seed=1, lattice_system="cubical")
    bad = SampleResult(frac_x=crystals.frac_x, atomic_numbers=np.full(5, 119.0), lattice=crystals.lattice, num_atoms=crystals.num_atoms)
    with pytest.raises(ValueError, match="not in this model's table"):
        m.noise_to(bad, 10, seed=1)
    _assert_nothing_drawn(before)
    # valid calls reach the engine; the state they build reads the cells with matrix_to_params
    with pytest.raises(AssertionError, match="engine was touched"):
        m.noise_to(crystals, 10, seed=1)
    with pytest.raises(AssertionError, match="engine was touched"):
        m.encode(crystals, num_steps=8)
    st = m._crystal_state(crystals, 10, "test")
    assert st.t == 10 and st.species.tolist() == [0, 1, 2, 0, 3] and st.num_atoms.tolist() == [3, 2]
    assert np.allclose(st.lengths, [[3, 4, 5]] * 2) and np.allclose(st.angles, np.pi / 2)


def test_draw_initial_state_draws_what_sample_draws():
    """The helper alone: the generators of sample() in their order (numpy's for the angles, torch's for lengths, then positions)."""
    import torch
    from arreau_amd.diffusion import lattice_systems
    dl = _dl()
    dl.num_atomic_states = 7
    np.random.seed(5)
    torch.manual_seed(5)
    st = dl.draw_initial_state([3, 1, 4], 3)
    np.random.seed(5)
    torch.manual_seed(5)
    angles, tie = lattice_systems.resolve(None, 3)
    lengths = torch.randn([3, 3])
    frac = torch.randn([8, 3], dtype=torch.get_default_dtype()) * 1.0
    assert tie is None and st.length_tie is None and st.t == T - 1
    assert np.array_equal(st.angles, angles) and np.array_equal(st.lengths, lengths.numpy()) and np.array_equal(st.frac_x, frac.numpy())
    assert st.species.tolist() == [6] * 8 and st.num_atoms.tolist() == [3, 1, 4]
    iv.check_state(st, T, 7)
    st = dl.draw_initial_state(2, 2, constant_atoms=torch.tensor([1, 2, 3, 4]), lattice_system="cubic")
    assert st.species.tolist() == [1, 2, 3, 4] and st.length_tie.tolist() == [2, 2]
    assert (st.lengths[:, 1:] == st.lengths[:, :1]).all()


# ------------------------------------------------------------------------------------------------- 4. generate.py
def test_generate_parses_the_start_flags():
    from arreau_amd import generate
    ap = generate.build_parser()
    base = ["--model_path", "x.ckpt"]
    a = ap.parse_args(base)
    assert a.start_from is None and a.start_t is None and a.invert is False
    assert generate.check_start_arguments(a, ap.error) is False
    a = ap.parse_args(base + ["--start_from", "c.npz", "--start_t", "20"])
    assert (a.start_from, a.start_t, a.invert) == ("c.npz", 20, False) and generate.check_start_arguments(a, ap.error) is True
    a = ap.parse_args(base + ["--start_from", "c.npz", "--start_t", "20", "--invert", "--eta", "0", "--num_steps", "8"])
    assert a.invert is True and a.eta == 0.0 and generate.check_start_arguments(a, ap.error) is True
    for bad in (["--start_from", "c.npz"], ["--start_t", "20"], ["--invert"], ["--start_from", "c.npz", "--start_t", "0"],
                ["--start_from", "c.npz", "--start_t", "20", "--template", "t.npz"],
                ["--start_from", "c.npz", "--start_t", "20", "--symops", "ops.txt"],
                ["--start_from", "c.npz", "--start_t", "20", "--lattice_system", "cubic"],
                ["--start_from", "c.npz", "--start_t", "20", "--require_valid"]):
        with pytest.raises(SystemExit):
            generate.check_start_arguments(ap.parse_args(base + bad), ap.error)
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--start_from", "c.npz", "--start_t", "twenty"])


def test_generate_from_crystals_shards_the_file():
    """Every rank takes its contiguous share of the file, in sub-batches, and rank 0 gets them back in file order."""
    from arreau_amd import generate
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    na = np.array([1, 3, 2, 4, 1, 2, 5])
    N = int(na.sum())
    crystals = SampleResult(frac_x=np.arange(3 * N, dtype=float).reshape(N, 3), atomic_numbers=np.arange(N, dtype=float),
                            lattice=np.arange(9 * len(na), dtype=float).reshape(-1, 3, 3), num_atoms=na, idx_start=np.cumsum(na) - na)
    seen = []

    def start_fn(sub):
        seen.append(np.asarray(sub.num_atoms).tolist())
        return sub

    parts = [generate.generate_from_crystals(start_fn, crystals, 2, rank, 3, gather=lambda obj: [obj]) for rank in range(3)]
    assert parts[1:] == [None, None] and np.asarray(parts[0].num_atoms).tolist() == [1, 3, 2]
    assert seen == [[1, 3], [2], [4, 1], [2, 5]]
    res = generate.generate_from_crystals(start_fn, crystals, 3)
    assert np.array_equal(res.num_atoms, na) and np.array_equal(res.frac_x, crystals.frac_x) and np.array_equal(res.lattice, crystals.lattice)
