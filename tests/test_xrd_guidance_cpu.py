"""XRD guidance without a GPU (rules in include/arreau_hip.h, "XRD guidance"): the float64 restatement of
diffusion/xrd_guidance.py against central differences of the pattern distance, its invariances, the descent run, every flag, the
preconditions of the shared cases (tests/xrd_guidance_cases.py), the recorded float32 deviations, the option's validation, the
sample_plan rules and the front end's dispatch on recording stand-ins."""
import numpy as np
import pytest
import torch

from arreau_amd import _hip, engine as engine_mod
from arreau_amd.diffusion import contact_guidance as cg, diffusion_loss as dl_mod, sample_plan, xrd, xrd_guidance as xg
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable
from tests import xrd_cases as xc, xrd_guidance_cases as cases

ZT = AtomicNumberTable([1, 6, 8, 14, 2001])
T, N, B, S = 100, 5, 2, 5
BATCH = dict(num_atoms_per_sample=[2, 3], num_samples_in_batch=2)


def _crystal(crystal, params=xc.DEFAULT):
    """(frac, cell, amplitudes) float64 of one (frac, cell, species) crystal."""
    f, L, z = crystal
    return np.asarray(f, dtype=np.float64).reshape(-1, 3), np.asarray(L, dtype=np.float64), xrd.host_weights(z, params)


def _exact(f, L, w, Q, params=xc.DEFAULT):
    return xg.reference(f, L[None], [len(f)], w, Q, params, exact_inputs=True)


def _target(crystal, params=xc.DEFAULT):
    f, L, w = _crystal(crystal, params)
    return xrd.xrd_reference(f, L[None], [len(f)], w, params, exact_inputs=True).pattern[0].astype(np.float32)


# ------------------------------------------------------------------------------------------------- the cases' preconditions
def test_the_cases_meet_their_preconditions():
    """Every unflagged test crystal lies at a float64 distance of at least MIN_TEST_DISTANCE from its target; the sizes the batches
    are named for: 1..8 atoms, 70 ragged crystals, five rounds of 256 box entries, exactly 256 atoms, windows of at most one and of
    963 grid points."""
    for name in cases.BATCHES:
        bt, ref = cases.reference(name)
        assert not ref.flags.any() and (ref.distance >= xg.MIN_TEST_DISTANCE).all(), (name, ref.distance.min())
        assert bt.target.dtype == np.float32 and bt.target.shape == (len(bt.counts), bt.params.n_points)
    assert cases.batch("textbook").counts == [1, 2, 4, 8, 8, 2] and len(cases.batch("ragged").counts) == 70
    assert 1 in cases.batch("ragged").counts and max(cases.batch("ragged").counts) <= 24
    assert cases.batch("atoms 256").counts == [xg.MAX_ATOMS] and cases.batch("random 20").counts == [20]
    bt = cases.batch("random 20")
    assert xrd.xrd_reference(bt.frac, bt.lattice, bt.counts, bt.weights, bt.params).rounds.tolist() == [5]
    step = lambda p: (p.two_theta_max - p.two_theta_min) / (p.n_points - 1)
    assert 2 * xrd.derived(xc.NARROW).six_sigma < step(xc.NARROW) and int(2 * xrd.derived(xc.WIDE).six_sigma / step(xc.WIDE)) + 1 == 963


@pytest.mark.parametrize("name", cases.BATCHES)
def test_the_recorded_float32_deviations_are_the_measured_ones(name):
    """tools/exp/xrd_guidance_f32_deviation.py's measurement again: F32_DEVIATION holds it to three digits, and the bound is 16
    times the largest entry."""
    from tools.exp.xrd_guidance_f32_deviation import deviation
    bt, r64 = cases.reference(name)
    r32 = xg.reference(bt.frac, bt.lattice, bt.counts, bt.weights, bt.target, bt.params, dtype=np.float32)
    assert np.array_equal(r32.flags, r64.flags) and np.array_equal(r32.reflections, r64.reflections)
    assert float(f"{deviation(bt, r64, r32):.3g}") == xg.F32_DEVIATION[name]
    assert tuple(xg.F32_DEVIATION) == cases.BATCHES and xg.G_F32_BOUND == 16 * max(xg.F32_DEVIATION.values()) == xrd.BOUND_FACTOR * 3.65e-06


# ------------------------------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("which", ["rock salt", "triclinic", "random 20"])
def test_gamma_is_the_central_difference_of_the_distance(which):
    """g times the metric against central differences (h = 1e-6) of xrd.distance(xrd_reference(...), Q) in every fractional
    coordinate: to 1e-7 of the largest component."""
    clean = {"rock salt": cases.rock_salt(), "triclinic": xc.triclinic_crystal(), "random 20": xc.random_crystal(cases.RANDOM_20_SEED, 20)}[which]
    f, L, w = _crystal(cases.displaced(clean, 0))
    Q = _target(clean)
    ref = _exact(f, L, w, Q)
    gam = xg.gamma(ref.g, L)
    dist = lambda x: xrd.distance(xrd.xrd_reference(x, L[None], [len(x)], w, xc.DEFAULT, exact_inputs=True).pattern[0], Q)
    assert abs(dist(f) - ref.distance[0]) <= 1e-15 and ref.distance[0] >= xg.MIN_TEST_DISTANCE
    h, num = 1e-6, np.zeros_like(f)
    for a in range(len(f)):
        for k in range(3):
            up, down = f.copy(), f.copy()
            up[a, k] += h
            down[a, k] -= h
            num[a, k] = (dist(up) - dist(down)) / (2 * h)
    err = np.abs(num - gam).max() / np.abs(gam).max()
    print(f"{which}: distance {ref.distance[0]:.4g}, largest |gamma| {np.abs(gam).max():.4g}, error {err:.3g} of it")
    assert err <= 1e-7


def test_g_is_the_cartesian_gradient_times_the_inverse_cell():
    """g = D L^-1 in the skewed triclinic cell: g L = D, and the fractional move -w g is the Cartesian move -w D."""
    f, L, w = _crystal(cases.displaced(xc.triclinic_crystal(), 1))
    ref = _exact(f, L, w, _target(xc.triclinic_crystal()))
    assert np.abs(ref.g @ L - ref.D).max() <= 1e-13 * np.abs(ref.D).max() and np.abs(ref.D).max() > 0
    assert np.abs(ref.g - ref.D @ np.linalg.inv(L)).max() <= 1e-12 * np.abs(ref.g).max()


def test_a_translation_changes_nothing_and_the_gradients_sum_to_zero():
    f, L, w = _crystal(cases.displaced(xc.triclinic_crystal(), 2))
    Q = _target(xc.triclinic_crystal())
    ref = _exact(f, L, w, Q)
    moved = _exact(f + np.array([0.137, -0.29, 0.611]), L, w, Q)
    top = np.abs(ref.g).max()
    assert np.abs(moved.g - ref.g).max() <= 1e-12 * top and np.abs(ref.g.sum(axis=0)).max() <= 1e-12 * top and top > 0
    assert abs(moved.distance[0] - ref.distance[0]) <= 1e-14


def test_a_masked_atom_is_not_pushed_and_does_not_scatter():
    """An atom of amplitude 0 (the mask class under class_weights) has g = 0 and leaves the pattern and the others' g those of
    the crystal without it."""
    f, L, w = _crystal(cases.displaced(cases.rock_salt(), 3))
    Q = _target(cases.rock_salt())
    w0 = w.copy()
    w0[2] = 0.0
    with_mask = _exact(f, L, w0, Q)
    keep = np.arange(8) != 2
    without = _exact(f[keep], L, w[keep], Q)
    assert not with_mask.g[2].any() and np.abs(with_mask.g).max() > 0
    assert np.abs(with_mask.pattern[0] - without.pattern[0]).max() <= 1e-12 * without.pattern[0].max()
    assert np.abs(with_mask.g[keep] - without.g).max() <= 1e-12 * np.abs(without.g).max()
    table = xg.class_weights(ZT, xc.DEFAULT)
    assert table.tolist() == [1.0, 6.0, 8.0, 14.0, 0.0] and xg.class_weights(ZT, xrd.XrdParams(scattering="unit")).tolist() == [1, 1, 1, 1, 0]
    assert xg.atom_weights([0, 4, 3, -1, 5], table).tolist() == [1.0, 0.0, 14.0, 0.0, 0.0]


def test_plain_descent_lowers_the_distance_monotonically():
    """Rock salt, seed 0, 0.15 A, x <- x - w g with w = 2 A^2, 50 moves: the distance falls at every move and ends below 1e-2 of
    its start."""
    f, L, w = _crystal(cases.displaced(cases.rock_salt(), 0))
    Q = _target(cases.rock_salt())
    trace = []
    for _ in range(50):
        ref = _exact(f, L, w, Q)
        trace.append(ref.distance[0])
        f = f - xg.DEFAULT_WEIGHT * ref.g
    trace.append(_exact(f, L, w, Q).distance[0])
    print(f"descent: {trace[0]:.4g} -> {trace[-1]:.4g} ({trace[-1] / trace[0]:.3g} of the start)")
    assert (np.diff(trace) < 0).all() and trace[-1] <= 1e-2 * trace[0]


def test_the_float32_mode_stays_near_the_float64_mode():
    bt, r64 = cases.reference("triclinic")
    r32 = xg.reference(bt.frac, bt.lattice, bt.counts, bt.weights, bt.target, bt.params, dtype=np.float32)
    assert r32.g.dtype == np.float32 and np.abs(r32.g - r64.g).max() <= xg.g_bound(r64.g, r64.g_terms) / xg.BOUND_FACTOR * 1.01
    assert abs(r32.distance[0] - r64.distance[0]) <= 1e-6


# ------------------------------------------------------------------------------------------------- flags
def test_every_flag():
    bt = cases.flags_batch()
    ref = xg.reference(bt.frac, bt.lattice, bt.counts, bt.weights, bt.target, bt.params)
    assert list(ref.flags) == cases.FLAGS_EXPECTED and bt.counts[4] == xg.MAX_ATOMS + 1
    off = cases.offsets(bt)
    for b, flag in enumerate(cases.FLAGS_EXPECTED):
        if flag:
            assert not ref.g[off[b]:off[b + 1]].any() and np.isnan(ref.distance[b]) and ref.reflections[b] == 0
    assert ref.g[off[-2]:].any() and ref.distance[-1] > 0
    dark = cases.dark_batch()
    ref = xg.reference(dark.frac, dark.lattice, dark.counts, dark.weights, dark.target, dark.params)
    assert list(ref.flags) == [xg.DARK] and not ref.g.any()
    for bad in (np.nan, np.inf, -1.0):
        bt = cases.single(cases.batch("triclinic"), 0)
        bt.target[0, 7] = bad
        assert list(xg.reference(bt.frac, bt.lattice, bt.counts, bt.weights, bt.target, bt.params).flags) == [xg.NO_TARGET]
    assert xg.describe(xg.LARGE) == "LARGE" and xg.describe(xg.RANGE) == "RANGE" and xg.describe(0) == "ok"
    assert (xg.NO_TARGET, xg.DARK, xg.LARGE) == (16, 32, 64) and xg.SKIPPED == 127


def test_guided_eps_and_the_statistics():
    bt, ref = cases.reference("textbook")
    sig = np.linspace(0.01, 1.0, T + 1)
    t = cases.timesteps(len(bt.counts))
    eps = np.ones_like(bt.frac)
    got = xg.guided_eps(eps, ref, bt.counts, sig, t, 2.0)
    k = np.repeat(2.0 / sig[t] ** 2, bt.counts)
    assert np.allclose(got, 1.0 + k[:, None] * ref.g, rtol=1e-15) and np.array_equal(xg.sigma_coefficient(sig, [0, T + 5], 1.0), 1.0 / sig[[1, T]] ** 2)
    info = {"distance": np.array([0.25, np.nan, 0.01], np.float32), "reflections": np.array([10, 0, 4]), "flags": np.array([0, xg.DARK, 0])}
    lines = xg.summary_lines([xg.stats_of(info, 0), xg.stats_of(info, 1)])
    assert len(lines) == 3 and lines[0].startswith("xrd guidance, rank 0: 3 crystals, last evaluation: 2 guided, distance to the target mean 0.130000, min 0.010000, max 0.250000")
    assert lines[2].startswith("xrd guidance, total: 6 crystals") and lines[2].endswith("flags: DARK 2")


def test_header_binding_and_build_agree():
    import os
    import re
    from arreau_amd import build
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "arreau_hip.h")) as fh:
        text = fh.read()
    defs = {k: int(v) for k, v in re.findall(r"#define ARREAU_XGUIDE_(\w+) (\d+)", text)}
    assert defs == {"NO_TARGET": xg.NO_TARGET, "DARK": xg.DARK, "LARGE": xg.LARGE}
    fields = re.search(r"typedef struct arreau_xrd_guidance \{(.*?)\} arreau_xrd_guidance;", text, re.S).group(1)
    assert tuple(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+(\w+);", fields, re.M)) == tuple(n for n, _ in _hip.XrdGuidanceC._fields_)
    assert tuple(n for n, _ in _hip.XrdGuidanceC._fields_)[-3:] == tuple("d_" + k for k in xg.INFO_KEYS)
    assert "xrd_guide.hip" in build.SOURCES and "xrd_guide.hip" in build.ASM_LINT and "xrd_dev.h" in build.HEADERS
    assert xg.MAX_ATOMS == 256 and xg.FLAG_NAMES[:4] == xrd.FLAG_NAMES


# ------------------------------------------------------------------------------------------------- validation
def test_the_option_is_validated_before_any_work():
    P = xrd.XrdParams(n_points=64)
    ok = xg.XrdGuidance(np.ones(64), params=P)
    assert ok.weight == 2.0 and ok.count() == 1 and ok.patterns(3).shape == (3, 64) and ok.patterns(3).dtype == np.float32
    assert xg.XrdGuidance(np.ones((2, 64)), 0.0, P).count() == 2
    for bad, text in ((dict(target=np.ones(63)), "n_points = 64"), (dict(target=np.ones((2, 2, 64))), "n_points = 64"),
                      (dict(target=np.full(64, np.nan)), "finite"), (dict(target=np.full(64, 1e39)), "finite"),
                      (dict(target=-np.ones(64)), "non-negative"), (dict(target=np.zeros(64)), "all zero"),
                      (dict(target=np.stack([np.ones(64), np.zeros(64)])), "all zero"), (dict(target=None), "required"),
                      (dict(target=np.ones(64), weight=-0.5), "weight"), (dict(target=np.ones(64), weight=float("nan")), "weight"),
                      (dict(target=np.ones(64), weight=True), "weight"), (dict(target=np.ones(64), weight=1e39), "weight"),
                      (dict(target=np.ones(64), params="Cu"), "XrdParams")):
        with pytest.raises(ValueError, match=text):
            xg.XrdGuidance(**{**dict(params=P), **bad})
    with pytest.raises(ValueError, match="2 target patterns for 3 crystals"):
        xg.XrdGuidance(np.ones((2, 64)), params=P).patterns(3)
    assert xg.resolve(None) is None and xg.resolve(False) is None and xg.resolve(ok) is ok
    for bad in (True, 2.0, np.ones(64)):
        with pytest.raises(ValueError, match="xrd_guidance must be None or an XrdGuidance"):
            xg.resolve(bad)
    with pytest.raises(ValueError, match="inversion"):
        xg.check_sampling(ok, inversion=True)
    with pytest.raises(ValueError, match='scattering "weights"'):
        xg.check_sampling(xg.XrdGuidance(np.ones(64), params=xrd.XrdParams(n_points=64, scattering="weights")))
    with pytest.raises(ValueError, match='scattering "weights"'):
        xg.class_weights(ZT, xrd.XrdParams(scattering="weights"))
    xg.check_sampling(None, inversion=True)
    crystals = type("Crystals", (), dict(frac_x=np.zeros((1, 3)), lattice=np.eye(3)[None] * 4, num_atoms=np.array([1]), atomic_numbers=np.array([6])))()
    assert xg.XrdGuidance(crystals).count() == 1 and xg.XrdGuidance(crystals).target is None


def test_the_sample_plan_rules():
    P = xrd.XrdParams(n_points=64)
    one, two, three = (xg.XrdGuidance(np.ones((k, 64)), params=P) for k in (1, 2, 3))
    assert sample_plan.resolve(T, ZT, **BATCH).xrd_guidance is None
    for noise in sample_plan.NOISE_MODES:
        assert sample_plan.resolve(T, ZT, xrd_guidance=one, noise=noise, **BATCH).xrd_guidance is one
    plan = sample_plan.resolve(T, ZT, xrd_guidance=two, contact_guidance=True, corrector_steps=1, fixed_cell=True, **BATCH)
    assert plan.xrd_guidance is two and plan.guidance is not None and plan.fixed_cell
    with pytest.raises(ValueError, match="3 targets for 2 crystals"):
        sample_plan.resolve(T, ZT, xrd_guidance=three, **BATCH)
    with pytest.raises(ValueError, match="xrd_guidance must be"):
        sample_plan.check_options(xrd_guidance=True)
    with pytest.raises(ValueError, match='scattering "weights"'):
        sample_plan.check_options(xrd_guidance=xg.XrdGuidance(np.ones(64), params=xrd.XrdParams(n_points=64, scattering="weights")))


# ------------------------------------------------------------------------------------------------- the front end's dispatch
class RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == "arreau_workspace_bytes":
            return lambda *a: 64

        def export(*args):
            self.calls.append((name, args))
            return 0
        return export


def _engine():
    eng = engine_mod.HipEngine.__new__(engine_mod.HipEngine)
    eng.device, eng.cfg, eng._handle, eng._ws, eng._ws_cap, eng.S = torch.device("cpu"), _hip.Config(num_timesteps=T), "H", None, (0, 0), S
    return eng


def _device_guidance(info=True, **kw):
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
    fields = dict(class_weights=f(S))
    fields.update(kw)
    made = {"distance": f(B), "reflections": torch.zeros(B, dtype=torch.int32), "flags": torch.zeros(B, dtype=torch.int32)}
    return xg.DeviceGuidance(xrd.XrdParams(n_points=64), 2.0, f(B, 64), info=made if info else None, **fields)


def test_the_engine_reaches_the_export_and_fills_the_struct(monkeypatch):
    rec = RecordingLib()
    monkeypatch.setattr(_hip, "lib", lambda: rec)
    monkeypatch.setattr(_hip, "stream_ptr", lambda device=None: "stream")
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
    i = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    frac, types, lengths, angles, off, lattice = f(N, 3), i(N), f(B, 3), f(B, 3), i(B + 1), f(B, 3, 3)
    null = lambda a: a is None or (hasattr(a, "value") and not a.value)
    guide = _device_guidance()
    eng = _engine()
    eng.sample_loop(frac, types, lengths, angles, off, 90, 3, 7, None, lattice, xrd_guidance=guide)
    eng.sample_loop(frac, types, lengths, angles, off, 90, 3, 7, None, lattice, xrd_guidance=guide, guidance=cg.ContactGuidance(), length_tie=i(B))
    eng.sample_loop(frac, types, lengths, angles, off, 90, 3, 7, None, lattice, guidance=cg.ContactGuidance())
    (n0, a0), (n1, a1), (n2, _) = rec.calls
    assert n0 == n1 == "arreau_sample_loop_xrd_guided" and n2 == "arreau_sample_loop_guided"
    assert "".join("0" if null(a) else "1" for a in a0[17:-1]) == "0000" "00001" "001"  # species (every class), then the struct
    assert "".join("0" if null(a) else "1" for a in a1[17:-1]) == "0000" "10001" "011"
    c = a0[-2]._obj
    assert (c.params.n_points, c.params.wavelength, c.weight) == (64, 1.54184, 2.0) and c.d_target == guide.target.data_ptr()
    assert c.d_class_weights == guide.class_weights.data_ptr() and not c.d_atom_weights and c.d_flags == guide.info["flags"].data_ptr()
    rec.calls.clear()
    eps, grad = f(N, 3), f(N, 3)
    eng.xrd_guidance_step(frac, None, lattice, i(B), off, eps, _device_guidance(info=False, class_weights=None, atom_weights=f(N)), gradient=grad)
    (name, args), = rec.calls
    assert name == "arreau_xrd_guidance_step" and null(args[2]) and args[6:8] == (B, N) and args[10].value == grad.data_ptr()
    assert args[9]._obj.d_atom_weights and not args[9]._obj.d_class_weights and not args[9]._obj.d_distance
    for bad, text in ((_device_guidance(atom_weights=f(N)), "exactly one"), (_device_guidance(class_weights=None), "exactly one"),
                      (_device_guidance(class_weights=f(S + 1)), "class_weights must be"), ("no", "DeviceGuidance")):
        with pytest.raises(ValueError, match=text):
            eng.sample_loop(frac, types, lengths, angles, off, 90, 3, 7, None, lattice, xrd_guidance=bad)
    with pytest.raises(ValueError, match="exactly one"):  # a loop takes class weights
        eng.sample_loop(frac, types, lengths, angles, off, 90, 3, 7, None, lattice, xrd_guidance=_device_guidance(class_weights=None, atom_weights=f(N)))
    with pytest.raises(ValueError, match="^xrd guidance: target must be"):
        eng.xrd_guidance_step(frac, types, lattice, i(B + 1), i(B + 2), eps, guide)
    assert sorted(_hip.EXPORTS).count("arreau_sample_loop_xrd_guided") == 1 and "arreau_xrd_guidance_step" in _hip._prototypes()


class RecordingEngine:
    def __init__(self):
        self.calls, self.device = [], torch.device("cpu")

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append(name)
            if name == "predict_scores":
                return torch.zeros(N, 3), torch.zeros(N, S), torch.zeros(B, 3)
        return call


@pytest.mark.parametrize("contacts", [False, True])
def test_the_host_noise_driver_guides_every_evaluation_in_rule_7_s_order(contacts, monkeypatch):
    one = xg.XrdGuidance(np.ones(64), params=xrd.XrdParams(n_points=64))
    plan = sample_plan.resolve(T, ZT, noise="device", timesteps=[90, 1], corrector_steps=1, xrd_guidance=one, contact_guidance=contacts or None, **BATCH)
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
    buf = dl_mod._RunBuffers(frac_d=f(N, 3), types_d=torch.zeros(N, dtype=torch.int32), len_d=f(B, 3) + 4, ang_d=f(B, 3) + 1.5,
                             off_d=torch.tensor([0, 2, 5], dtype=torch.int32), lattice_d=f(B, 3, 3), clipmax=0.99,
                             guide=(plan.guidance, {}) if contacts else None, xguide=_device_guidance())
    monkeypatch.setattr(dl_mod, "lattice_from_params", lambda lengths, angles: f(B, 3, 3))
    eng = RecordingEngine()
    dl_mod._host_noise_driver(eng, plan, buf, None, False, lambda suffix: None)
    evaluation = ["predict_scores"] + (["contact_guidance_step"] if contacts else []) + ["xrd_guidance_step"]
    assert eng.calls == (evaluation + ["corrector_step"] + evaluation + ["predictor_step"]) * 2
    buf.xguide.weight = 0.0  # weight 0: no launch is added
    eng = RecordingEngine()
    dl_mod._host_noise_driver(eng, plan, buf, None, False, lambda suffix: None)
    assert "xrd_guidance_step" not in eng.calls
