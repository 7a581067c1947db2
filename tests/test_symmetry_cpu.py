"""Space-group symmetry on the host (arreau_amd/diffusion/symmetry.py): parsing of xyz operations, group closure, the metric
check, orbits of templates, the float64 restatements (positions and species), the reach and the power of the cases the GPU tests
step (tests/symmetry_cases.py), sampler and CLI argument errors.  No GPU."""
import argparse

import numpy as np
import pytest

from arreau_amd.diffusion import symmetry as sy
from tests import symmetry_cases as C

GROUPS = {
    "P21/c": (["-x,y+1/2,-z+1/2", "-x,-y,-z"], "monoclinic", 4),
    "Pnma": (["-x+1/2,-y,z+1/2", "-x,y+1/2,-z", "-x,-y,-z"], "orthorhombic", 8),
    "P4/mmm": (["-y,x,z", "x,-y,-z", "-x,-y,-z"], "tetragonal", 16),
    "R-3m": (["-y,x-y,z", "y,x,-z", "-x,-y,-z", "x+2/3,y+1/3,z+1/3"], "hexagonal", 36),
    "Fm-3m": (["z,x,y", "-y,x,z", "-x,-y,-z", "x,y+1/2,z+1/2", "x+1/2,y,z+1/2"], "cubic", 192),
}
FCC = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
ROCK_SALT = np.concatenate([FCC, (FCC + 0.5) % 1])


def pnma_4c(x=0.1377, z=0.3141):
    return np.array([[x, 0.25, z], [-x + 0.5, 0.75, z + 0.5], [-x, 0.75, -z], [x + 0.5, 0.25, -z + 0.5]]) % 1


def wrapped(d):
    return np.abs(d - np.round(d))


def assert_symmetric(spec, x, tol=1e-12):
    """Every op g_m maps every atom onto an atom, within tol (wrapped)."""
    for R, t in spec.ops:
        gx = x @ R.T + t
        d = wrapped(gx[:, None, :] - x[None, :, :]).max(axis=2).min(axis=1)
        assert d.max() <= tol, (R, t, d.max())


# ---- parsing --------------------------------------------------------------------------------------------------------------
def test_parse_exact():
    R, t = sy.parse_symop("-x+1/2,y,-z+1/2")
    assert R.tolist() == [[-1, 0, 0], [0, 1, 0], [0, 0, -1]] and t.tolist() == [0.5, 0.0, 0.5]
    R, t = sy.parse_symop("x-y+2/3, x+1/3, Z-1/6")
    assert R.tolist() == [[1, -1, 0], [1, 0, 0], [0, 0, 1]]
    assert t[0] == 2 / 3 and t[1] == 1 / 3 and t[2] == 5 / 6  # reduced to [0, 1), exact as float64 quotients
    assert sy.parse_symop("1/4+x,y+3/4,-z+1")[1].tolist() == [0.25, 0.75, 0.0]
    assert sy.format_symop(*sy.parse_symop("-x+1/2,y,-z+2/3")) == "-x+1/2,y,-z+2/3"


@pytest.mark.parametrize("bad", ["x,y", "x,y,z,x", "x+1/5,y,z", "x+0.5,y,z", "x,x,z", "x+y,y,z+w", "x,y,", "2x,y,z",
                                 "x+x,y,z", "x+1/2+1/2,y,z", "x+y,x+y,z", "", "x;y;z"])
def test_parse_rejects(bad):
    with pytest.raises(ValueError):
        sy.parse_symop(bad)


# ---- closure and metric ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_closed_orders(name):
    gens, system, order = GROUPS[name]
    group = sy.close_group(gens)
    assert len(group) == order
    assert np.array_equal(group[0][0], np.eye(3)) and not group[0][1].any()  # identity first
    assert len(sy.close_group([sy.format_symop(R, t) for R, t in group])) == order  # closed: closing again adds nothing
    sy.check_metric(group, system)


def test_over_192_raises():
    # Fm-3m plus a translation of 1/3 along x: not a space group, more than 192 elements modulo integer translations
    with pytest.raises(ValueError, match="192"):
        sy.close_group(GROUPS["Fm-3m"][0] + ["x+1/3,y,z"])


def test_metric_mismatch_raises():
    with pytest.raises(ValueError, match="metric"):
        sy.SymmetrySpec.general_positions(GROUPS["R-3m"][0], 1, "cubic")
    with pytest.raises(ValueError, match="metric"):
        sy.SymmetrySpec.general_positions(GROUPS["P4/mmm"][0], 1, "orthorhombic")  # a = b is needed
    with pytest.raises(ValueError, match="metric"):
        sy.SymmetrySpec.general_positions(["-x,-y,z"], 1, "monoclinic")  # c-unique: beta is the free angle
    with pytest.raises(ValueError, match="unknown lattice system"):
        sy.SymmetrySpec.general_positions(GROUPS["P21/c"][0], 1, "monoclinc")


# ---- orbits ------------------------------------------------------------------------------------------------------------------
def test_rock_salt_orbits():
    spec = sy.SymmetrySpec.from_template(ROCK_SALT, GROUPS["Fm-3m"][0], "cubic")
    assert [o.tolist() for o in spec.orbits] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert [len(h) for h in spec.stabilizers] == [48, 48] and spec.order == 192
    assert spec.leader.tolist() == [0] * 4 + [4] * 4
    for j in range(8):  # g_k(j)(x_leader) = x_j (mod 1)
        l, k = spec.leader[j], spec.op[j]
        assert wrapped(spec.R[k] @ ROCK_SALT[l] + spec.t[k] - ROCK_SALT[j]).max() < 1e-12


def test_pnma_4c_orbit():
    spec = sy.SymmetrySpec.from_template(pnma_4c(), GROUPS["Pnma"][0], "orthorhombic")
    assert len(spec.orbits) == 1 and len(spec.orbits[0]) == 4 and len(spec.stabilizers[0]) == 2


def test_general_positions_layout():
    spec = sy.SymmetrySpec.general_positions(GROUPS["P21/c"][0], 5, "monoclinic")
    assert spec.n_atoms == 20 and spec.leader.tolist() == sum([[4 * o] * 4 for o in range(5)], [])
    assert spec.op.tolist() == list(range(4)) * 5 and all(h.tolist() == [0] for h in spec.stabilizers)


def test_asymmetric_template_raises():
    x = pnma_4c()
    x[2, 0] += 0.01
    with pytest.raises(ValueError, match="atom"):
        sy.SymmetrySpec.from_template(x, GROUPS["Pnma"][0], "orthorhombic")
    with pytest.raises(ValueError, match="atom 0"):
        sy.SymmetrySpec.from_template(ROCK_SALT[:7], GROUPS["Fm-3m"][0], "cubic")


# ---- float64 restatements ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rock salt", "pnma 4c", "r-3m general"])
def test_projection_idempotent_and_expansion_symmetric(case):
    rng = np.random.RandomState(3)
    if case == "rock salt":
        spec, anchors = sy.SymmetrySpec.from_template(ROCK_SALT, GROUPS["Fm-3m"][0], "cubic"), ROCK_SALT[[0, 4]]
    elif case == "pnma 4c":
        spec, anchors = sy.SymmetrySpec.from_template(pnma_4c(), GROUPS["Pnma"][0], "orthorhombic"), pnma_4c()[:1]
    else:
        spec = sy.SymmetrySpec.general_positions(GROUPS["R-3m"][0], 2, "hexagonal")
        anchors = rng.uniform(0, 1, (2, 3))
    xl = np.stack([spec.project_leader(o, anchors[o] + rng.normal(0, 0.3, 3), anchors[o]) for o in range(len(spec.orbits))])
    again = np.stack([spec.project_leader(o, xl[o], xl[o]) for o in range(len(spec.orbits))])
    assert wrapped(again - xl).max() <= 1e-12
    x = spec.expand(xl)
    assert ((x >= 0) & (x <= 1)).all()  # (a tiny negative wraps to exactly 1.0, as remainder_one does on the device)
    assert_symmetric(spec, x)


def test_pnma_site_keeps_free_coordinates():
    spec = sy.SymmetrySpec.from_template(pnma_4c(), GROUPS["Pnma"][0], "orthorhombic")
    p = spec.project_leader(0, np.array([0.2, 0.31, 0.4]), pnma_4c()[0])
    assert np.allclose(p, [0.2, 0.25, 0.4], atol=1e-15)  # (x, 1/4, z): y pinned, x and z free


def test_step_positions_is_symmetric_and_general_position_is_the_plain_update():
    rng = np.random.RandomState(8)
    spec = sy.SymmetrySpec.general_positions(GROUPS["P21/c"][0], 2, "monoclinic")
    x = spec.expand(rng.uniform(0, 1, (2, 3)))
    eps, z = rng.normal(size=(8, 3)), rng.normal(size=(8, 3))
    new = spec.step_positions(x, eps, z, 0.7, 0.65)
    assert_symmetric(spec, new)
    # one orbit whose members' noise is the image of the leader's: eps_bar is the leader's own noise
    eps2 = np.stack([spec.R[spec.op[j]] @ eps[spec.leader[j]] for j in range(8)])
    s2, sp2 = 0.49, 0.65 ** 2
    y = x[0] - eps[0] * (s2 - sp2) + np.sqrt(sp2 * (s2 - sp2) / s2) * z[0]
    assert wrapped(spec.step_positions(x, eps2, z, 0.7, 0.65)[0] - y).max() <= 1e-12


def test_initial_positions_on_site_and_unwrapped():
    spec = sy.SymmetrySpec.from_template(ROCK_SALT, GROUPS["Fm-3m"][0], "cubic")
    draw = np.random.RandomState(1).normal(0, 2.0, (8, 3))
    x = spec.initial_positions(draw)
    assert wrapped(x - ROCK_SALT).max() <= 1e-12  # point sites: every draw projects onto them
    assert_symmetric(spec, x % 1)


def test_species_check():
    spec = sy.SymmetrySpec.from_template(ROCK_SALT, GROUPS["Fm-3m"][0], "cubic")
    spec.check_species([1, 1, 1, 1, 2, 2, 2, 2])
    with pytest.raises(ValueError, match="orbit"):
        spec.check_species([1, 1, 2, 1, 2, 2, 2, 2])


def test_device_arrays_layout():
    import torch
    a = sy.SymmetrySpec.general_positions(GROUPS["P21/c"][0], 1, "monoclinic")
    b = sy.SymmetrySpec.from_template(pnma_4c(), GROUPS["Pnma"][0], "orthorhombic")
    t = sy.device_arrays([a, None, b, a], np.array([0, 4, 7, 11, 15]), torch.device("cpu"))
    assert t["leader"].tolist() == [0] * 4 + [-1] * 3 + [7] * 4 + [11] * 4
    assert t["orbit"].tolist() == [0] * 4 + [-1] * 3 + [1] * 4 + [2] * 4
    assert t["orbit_ptr"].tolist() == [0, 4, 8, 12] and t["stab_ptr"].tolist() == [0, 1, 3, 4]
    assert t["rot"].shape == (12, 9) and t["trans"].shape == (12, 3) and t["rot"].dtype == torch.float32  # a's rows shared
    assert t["op"][11:].tolist() == [0, 1, 2, 3] and t["op"][7:11].min() >= 4
    with pytest.raises(ValueError, match="holds 3 atoms"):
        sy.device_arrays([a, b], np.array([0, 4, 7]), torch.device("cpu"))


# ---- rule 5, the species ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(C.MODELS))
def tables(request):
    """(S, sigmas, q_one_step_transposed, q_mats) of the synthetic model of the GPU value tests, float64."""
    import torch
    from arreau_amd.checkpoint import make_synthetic_model
    from tests.helpers import oracle_from_module
    kw = dict(C.MODELS[request.param])
    om = oracle_from_module(make_synthetic_model(seed=4321, num_timesteps=C.T, **kw), torch.float32)
    return (kw["S"],) + C.model_tables(om)


def _d3pm_post(q1t, qmats, logits, xt, t, s):
    """The posterior as tests/test_gpu_respaced_sampling.py states it, in torch float64."""
    import torch
    if t == 1:
        return logits
    fact1 = q1t[t - 1, xt, :] if s == t - 1 else qmats[t - s - 1][:, xt].T
    fact2 = torch.softmax(logits, dim=-1) @ qmats[s - 1]
    return torch.log(fact1 + 1e-6) + torch.log(fact2 + 1e-6)


@pytest.mark.parametrize("t,s", C.PAIRS)
def test_step_species_of_p1_is_the_plain_arg_max(tables, t, s):
    """Orbits of one atom: exactly the arg-max of the D3PM posterior plus the atom's own Gumbel noise, per atom."""
    import torch
    S, _, q1t, qm = tables
    n = 40
    spec = sy.SymmetrySpec.general_positions(C.GENS["P1"], n, "triclinic")
    assert spec.order == 1 and [o.tolist() for o in spec.orbits] == [[j] for j in range(n)]
    rng = np.random.RandomState(t)
    logits, u, ty = rng.normal(0, 2, (n, S)), rng.uniform(0, 1, (n, S)), rng.randint(0, S, n)
    ty[::3] = S - 1
    u[0, 0] = 0.0  # below the clip
    cls, margin = spec.step_species(logits, ty, u, t, s, q1t, qm)
    post = _d3pm_post(torch.as_tensor(q1t), torch.as_tensor(qm), torch.as_tensor(logits), torch.as_tensor(ty), t, s)
    val = post - torch.log(-torch.log(torch.clip(torch.as_tensor(u), 1e-6, 1.0))) * (0.2 if t == 1 else 1.0)
    assert np.array_equal(cls, torch.argmax(val, dim=-1).numpy())
    top = torch.topk(val, 2, dim=-1).values
    assert np.allclose(margin, (top[:, 0] - top[:, 1]).numpy(), rtol=0, atol=1e-12) and (margin >= 0).all()


def test_step_species_is_the_orbits_draw(tables):
    """Classes constant on orbits; members' uniforms and classes are not read; one member's logits move the orbit's mean."""
    S, _, q1t, qm = tables
    spec = C.spec("fm3m-mixed")
    n = spec.n_atoms
    rng = np.random.RandomState(5)
    logits, u, ty = rng.normal(0, 2, (n, S)), rng.uniform(0, 1, (n, S)), rng.randint(0, S, n)
    member = np.ones(n, dtype=bool)
    member[spec.leaders] = False
    for t, s in C.PAIRS:
        cls, margin = spec.step_species(logits, ty, u, t, s, q1t, qm)
        spec.check_species(cls)
        u2, ty2 = u.copy(), ty.copy()
        u2[member], ty2[member] = rng.uniform(0, 1, (int(member.sum()), S)), (ty[member] + 1) % S
        cls2, margin2 = spec.step_species(logits, ty2, u2, t, s, q1t, qm)
        assert np.array_equal(cls, cls2) and np.array_equal(margin, margin2), (t, s)
        # the last member of the 96-atom orbit votes for the class the orbit did not take, hard enough to carry the mean
        j, other = int(spec.orbits[0][-1]), (int(cls[0]) + 1) % (S - 1)
        lg = logits.copy()
        lg[j, other] += 96 * 60.0
        cls3, _ = spec.step_species(lg, ty, u, t, s, q1t, qm)
        if t == 1 or ty[0] == S - 1:  # (an unmasked atom keeps its class until the last step, whatever the logits)
            assert (cls3[spec.orbits[0]] == other).all(), (t, s)
        assert np.array_equal(cls3[spec.orbits[1]], cls[spec.orbits[1]]) and np.array_equal(cls3[spec.orbits[2]], cls[spec.orbits[2]])


# ---- the cases the GPU tests step ----------------------------------------------------------------------------------------------
def test_reach_of_the_cases():
    """Orbit sizes and stabilizer orders of the specs with reach: 192, 96, 48, 32, 24, 18, 8 and 6 atoms; orders 1, 2, 4, 6, 8,
    24 and 48.  The wide batch holds them all, the deep one more than 64 crystals."""
    for name, (sizes, orders) in C.REACH.items():
        s = C.spec(name)
        assert [len(o) for o in s.orbits] == sizes and [len(h) for h in s.stabilizers] == orders, (name, s)
        rot, lead = C.can_tell(s)
        assert all(rot[o] for o in C.TELLS_ROT.get(name, [])), name
    assert set(C.REACH) <= set(C.WIDE) and len(C.DEEP) > 64
    assert sum(C.batch(C.WIDE)[1]) == 604 and max(C.batch(C.LOOP)[1]) >= 96
    assert C.can_tell(C.spec("fm3m-mixed"))[1].tolist() == [True, False, False]  # 4a and 8c are points
    assert not C.can_tell(C.spec("r3m-6c"))[0].any() and C.can_tell(C.spec("r3m-6c"))[1].all()


@pytest.mark.parametrize("batch_name", ["wide", "deep"])
def test_the_step_cases_tell_the_rules_apart(tables, batch_name):
    """The inputs of test_gpu_symmetry.py::test_step_values_against_the_restatements, stepped by the restatements alone: no
    orbit's two best classes are within MARGIN (so the device must give every class), wrong rules move every orbit that can
    show them by more than TELL and change the class of some orbits at every pair below T - 1, and leaders on special positions
    leave the cell.  At (T-1, T-2) the species rule is NOT told apart (0 to 2 orbits change class; printed only): the posterior
    keeps x_t there whatever the logits, so rule 5 rests on the other four pairs."""
    S, sig, q1t, qm = tables
    specs, counts = C.batch(C.WIDE if batch_name == "wide" else C.DEEP)
    first = C.first_atoms(counts)
    tells = {b: C.can_tell(s) for b, s in enumerate(specs) if s is not None}
    for t, s in C.PAIRS:
        x, ty = C.state(specs, counts, S, C.step_seed(batch_name, t))[:2]
        rng = np.random.RandomState(1000 + t)
        by_logits = by_uniforms = left = 0
        for _ in range(C.STEPS):
            sc = C.scores(rng, specs, counts, S, sigma_t=sig[t], sigma_s=sig[s])
            r = C.reference_step(specs, counts, x, ty, sc, t, s, sig, q1t, qm)
            for b in r.frac:
                assert (r.margins[b] >= C.MARGIN).all(), (t, s, b, r.margins[b].min())
                assert (r.rot[b][tells[b][0]] > C.TELL).all() and (r.lead[b][tells[b][1]] > C.TELL).all(), (t, s, b, r.rot[b], r.lead[b])
                x[first[b]:first[b + 1]], ty[first[b]:first[b + 1]] = r.frac[b], r.classes[b]
            by_logits, by_uniforms, left = by_logits + r.logit_orbits, by_uniforms + r.uniform_orbits, left + r.left
        print(f"{batch_name} S={S} ({t},{s}): orbits whose class the leader's own logits change {by_logits}, a member's uniforms "
              f"{by_uniforms}; special-position leaders that left the cell {left}")
        assert left >= 3, (t, s)  # (where the anchoring n_h of rule 3 decides a position)
        if t < C.T - 1:  # (at T - 1 the posterior keeps x_t by a margin of about 3, whatever the logits)
            assert by_logits >= 3 and by_uniforms >= 3, (t, s, by_logits, by_uniforms)


# ---- sampler and CLI errors --------------------------------------------------------------------------------------------------
class NoEngine:
    def engine(self):
        raise AssertionError("the engine was touched")


def _dl():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = 100
    return dl


def test_sample_rejects_before_any_work():
    from arreau_amd.diffusion.conditioning import SampleCondition  # noqa: F401  (only its presence is needed)
    gen = sy.SymmetrySpec.general_positions(GROUPS["P21/c"][0], 2, "monoclinic")
    rs = sy.SymmetrySpec.from_template(ROCK_SALT, GROUPS["Fm-3m"][0], "cubic")
    state = np.random.get_state()
    cases = [
        (dict(symmetry=gen, num_samples_in_batch=2, corrector_steps=1), "corrector_steps"),
        (dict(symmetry=gen, num_samples_in_batch=2, resample_passes=2), "resample_passes"),
        (dict(symmetry=gen, num_samples_in_batch=2, noise="reference"), "noise"),
        (dict(symmetry=gen, num_samples_in_batch=2, noise="device"), "noise"),
        (dict(symmetry=gen, num_samples_in_batch=2, condition=object()), "condition"),
        (dict(symmetry=gen), "num_samples_in_batch"),
        (dict(symmetry=[gen, None]), "num_atoms_per_sample"),
        (dict(symmetry=[gen, rs], num_samples_in_batch=3), "3 crystals"),
        (dict(symmetry=gen, num_samples_in_batch=2, num_atoms_per_sample=6), "6 atoms"),
        (dict(symmetry=[gen, rs], lattice_system="monoclinic"), "disagrees"),
        (dict(symmetry=[gen, 5]), "SymmetrySpec"),
        (dict(symmetry=rs, num_samples_in_batch=2, num_atoms_per_sample=8,
              constant_atoms=np.array([0, 0, 1, 0, 1, 1, 1, 1] * 2)), "orbit"),
    ]
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            _dl().sample(model=NoEngine(), z_table=None, **kw)
    assert np.array_equal(np.random.get_state()[1], state[1])  # nothing drawn


def _args(**kw):
    base = dict(symops=None, orbits=None, symmetry_template=None, template=None, lattice_system=None)
    base.update(kw)
    return argparse.Namespace(**base)


def _error(msg):
    raise ValueError(msg)


def test_cli_symmetry_options(tmp_path):
    from arreau_amd.generate import build_parser, load_symmetry
    ops = tmp_path / "p21c.txt"
    ops.write_text("# P2_1/c, b unique\n-x,y+1/2,-z+1/2   # screw\n\n-x,-y,-z\n")
    assert load_symmetry(_args(), _error) is None
    spec = load_symmetry(_args(symops=str(ops), orbits=3, lattice_system="monoclinic"), _error)
    assert spec.n_atoms == 12 and spec.order == 4
    for kw, match in ((dict(orbits=3), "lattice_system"), (dict(lattice_system="monoclinic"), "exactly one"),
                      (dict(lattice_system="monoclinic", orbits=1, symmetry_template="t.npz"), "exactly one"),
                      (dict(lattice_system="monoclinic", orbits=1, template="t.npz"), "--template"),
                      (dict(lattice_system="triclinic", orbits=1), "metric")):
        with pytest.raises(ValueError, match=match):
            load_symmetry(_args(symops=str(ops), **kw), _error)
    with pytest.raises(ValueError, match="need --symops"):
        load_symmetry(_args(orbits=2), _error)
    bad = tmp_path / "bad.txt"
    bad.write_text("x,y,z+1/5\n")
    with pytest.raises(ValueError, match="1/5"):
        load_symmetry(_args(symops=str(bad), orbits=1, lattice_system="triclinic"), _error)
    a = build_parser().parse_args(["--model_path", "m", "--symops", str(ops), "--orbits", "2", "--lattice_system", "monoclinic"])
    assert a.symops == str(ops) and a.orbits == 2


def test_cli_symmetry_template(tmp_path):
    from arreau_amd.diffusion.diffusion_loss import SampleResult
    from arreau_amd.generate import load_symmetry, save_sample_results
    ops = tmp_path / "fm3m.txt"
    ops.write_text("\n".join(GROUPS["Fm-3m"][0]) + "\n")
    na = np.array([8, 3])
    res = SampleResult(frac_x=np.concatenate([ROCK_SALT, np.random.RandomState(0).uniform(0, 1, (3, 3))]),
                       atomic_numbers=np.array([11] * 4 + [17] * 4 + [1] * 3, dtype=np.float64), lattice=np.stack([np.eye(3) * 5.6] * 2),
                       num_atoms=na, idx_start=np.cumsum(na) - na)
    path = save_sample_results(res, str(tmp_path / "t.npz"))
    spec = load_symmetry(_args(symops=str(ops), symmetry_template=path, lattice_system="cubic"), _error)
    assert spec.n_atoms == 8 and [len(o) for o in spec.orbits] == [4, 4]
