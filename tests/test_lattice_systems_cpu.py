"""Lattice systems on the host (arreau_amd/diffusion/lattice_systems.py): the table against the reference's prior, the draws of
`resolve`, argument errors, the host tie, and the float64 restatements of the tied update and jump.  No GPU."""
import numpy as np
import pytest
import torch

from arreau_amd.diffusion import lattice_systems as ls
from arreau_amd.diffusion.diffusion_helpers import sample_bravais_angles

TABLE = {"cubic": 2, "tetragonal": 1, "orthorhombic": 0, "hexagonal": 1, "rhombohedral": 2, "monoclinic": 0, "triclinic": 0}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_angles_are_the_prior_in_radians(name):
    np.random.seed(11)
    want = np.stack([np.deg2rad(sample_bravais_angles(name)) for _ in range(5)])
    np.random.seed(11)
    angles, codes = ls.resolve(name, 5)
    assert np.array_equal(angles, want)
    assert codes.dtype == np.int32 and codes.tolist() == [TABLE[name]] * 5
    assert ls.TIE_CODES == TABLE


def test_system_geometry_of_the_draws():
    np.random.seed(2)
    angles, _ = ls.resolve(["cubic", "hexagonal", "rhombohedral", "monoclinic", "triclinic"], 5)
    assert np.allclose(angles[0], np.pi / 2) and np.allclose(angles[1], [np.pi / 2, np.pi / 2, 2 * np.pi / 3])
    assert angles[2, 0] == angles[2, 1] == angles[2, 2] and np.pi / 3 <= angles[2, 0] <= 2 * np.pi / 3
    assert angles[3, 0] == angles[3, 2] == np.pi / 2 and np.pi / 2 <= angles[3, 1] <= np.pi
    assert ((angles[4] >= np.pi / 3) & (angles[4] <= 2 * np.pi / 3)).all()


def test_none_is_todays_draw():
    np.random.seed(5)
    want = np.array([sample_bravais_angles("monoclinic") for _ in range(7)])
    after = np.random.uniform()
    np.random.seed(5)
    angles, codes = ls.resolve(None, 7)
    assert codes is None and np.array_equal(angles, want)  # degrees, unconverted (read as radians by the device)
    assert angles[0, 0] == 90 and np.random.uniform() == after  # exactly the draws the old code consumed


def test_mixed_and_partial_systems_draw_in_crystal_order():
    names = ["triclinic", None, "cubic", "monoclinic"]
    np.random.seed(9)
    want = [np.deg2rad(sample_bravais_angles("triclinic")), sample_bravais_angles("monoclinic"),
            np.deg2rad(sample_bravais_angles("cubic")), np.deg2rad(sample_bravais_angles("monoclinic"))]
    np.random.seed(9)
    angles, codes = ls.resolve(names, 4)
    assert np.array_equal(angles, np.stack(want)) and codes.tolist() == [0, 0, 2, 0]


def test_errors_raise_before_any_draw():
    state = np.random.get_state()
    with pytest.raises(ValueError, match="unknown lattice system"):
        ls.resolve("quasicrystal", 3)
    with pytest.raises(ValueError, match="unknown lattice system"):
        ls.resolve(["cubic", "hexagnal", "cubic"], 3)
    with pytest.raises(ValueError, match="3 crystals"):
        ls.resolve(["cubic", "cubic"], 3)
    with pytest.raises(ValueError, match="knows"):
        ls.resolve(["cubic", None, "hexagonal"], 3, lattice_known=np.array([False, False, True]))
    with pytest.raises(ValueError):
        ls.resolve(5, 3)
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
    # no system on the known cell: accepted
    assert ls.check(["cubic", None], 2, lattice_known=[False, True]) == ["cubic", None]


def test_sample_rejects_before_any_work():
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss

    class NoEngine:
        def engine(self):
            raise AssertionError("the engine was touched")

    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = 100
    for kw, match in ((dict(lattice_system="cubix"), "unknown lattice system"), (dict(lattice_system=["cubic"] * 2), "3 crystals")):
        with pytest.raises(ValueError, match=match):
            dl.sample(model=NoEngine(), z_table=None, num_atoms_per_sample=4, num_samples_in_batch=3, **kw)


def test_host_tie():
    lengths = torch.randn(4, 3)
    orig = lengths.clone()
    ls.tie_lengths(lengths, np.array([0, 1, 2, 0], dtype=np.int32))
    assert torch.equal(lengths[0], orig[0]) and torch.equal(lengths[3], orig[3])
    assert lengths[1, 0] == lengths[1, 1] == orig[1, 0] and lengths[1, 2] == orig[1, 2]
    assert (lengths[2] == orig[2, 0]).all()


# ---- float64 restatements -------------------------------------------------------------------------------------------
T = 100


def _tables():
    betas = np.linspace(1e-4, 0.02, T + 1)
    betas[0] = 0.0
    return np.cumprod(1.0 - betas), betas


def _per_axis_rule2(xt, x0, z, t, s, ab, betas, clipmax):
    """Rule 2 of the respaced section (and the stride-1 step), per axis, written out independently."""
    out = np.empty_like(xt)
    for b in range(xt.shape[0]):
        for i in range(3):
            at, ap = ab[t[b]], ab[s[b]]
            beta = betas[t[b]] if s[b] == t[b] - 1 else min(1 - at / ap, clipmax)
            mean = (np.sqrt(ap) * beta * x0[b, i] + np.sqrt(1 - beta) * (1 - ap) * xt[b, i]) / (1 - at)
            out[b, i] = mean + (1 - ap) * beta / (1 - at) * (z[b, i] if t[b] > 1 else 0.0)
    return out


PAIRS = [(99, 98), (60, 12), (2, 1), (1, 0), (37, 36)]


def _inputs(seed, B=5):
    r = np.random.default_rng(seed)
    t = np.array([p[0] for p in PAIRS][:B])
    s = np.array([p[1] for p in PAIRS][:B])
    return r.normal(size=(B, 3)) * 3, r.normal(size=(B, 3)) * 4, r.normal(size=(B, 3)), t, s


def test_untied_update_is_rule_2():
    ab, betas = _tables()
    xt, x0, z, t, s = _inputs(1)
    got = ls.tied_update(xt, x0, z, t, s, ab, betas, np.zeros(5, dtype=np.int32), clipmax=0.5)
    assert np.allclose(got, _per_axis_rule2(xt, x0, z, t, s, ab, betas, 0.5), rtol=1e-13, atol=1e-13)
    # a bad code counts as 0, and a known cell is untied
    got = ls.tied_update(xt, x0, z, t, s, ab, betas, np.array([7, -1, 2, 1, 2]), clipmax=0.5, len_mask=np.array([0, 0, 1, 1, 1]))
    assert np.allclose(got, _per_axis_rule2(xt, x0, z, t, s, ab, betas, 0.5), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("code", [1, 2])
def test_tied_update(code):
    ab, betas = _tables()
    xt, x0, z, t, s = _inputs(2)
    codes = np.full(5, code, dtype=np.int32)
    got = ls.tied_update(xt, x0, z, t, s, ab, betas, codes)
    g = code + 1
    assert (got[:, :g] == got[:, :1]).all()  # tied axes exactly equal
    # the projection: the leader's x_t and draw with the group's mean x0
    xt_p, z_p, x0_p = xt.copy(), z.copy(), x0.copy()
    xt_p[:, :g], z_p[:, :g] = xt[:, :1], z[:, :1]
    x0_p[:, :g] = x0[:, :g].mean(axis=1, keepdims=True)
    assert np.allclose(got, _per_axis_rule2(xt_p, x0_p, z_p, t, s, ab, betas, 0.999), rtol=1e-13, atol=1e-13)
    if code == 1:  # the untied axis is as without a tie
        assert np.allclose(got[:, 2], _per_axis_rule2(xt, x0, z, t, s, ab, betas, 0.999)[:, 2], rtol=1e-13, atol=1e-13)
    # already tied inputs with one x0 across the group: the untied rule
    xt_t, x0_t, z_t = xt.copy(), x0.copy(), z.copy()
    xt_t[:, :g], x0_t[:, :g], z_t[:, :g] = xt[:, :1], x0[:, :1], z[:, :1]
    assert np.allclose(got := ls.tied_update(xt_t, x0_t, z_t, t, s, ab, betas, codes),
                       _per_axis_rule2(xt_t, x0_t, z_t, t, s, ab, betas, 0.999), rtol=1e-13, atol=1e-13)
    assert np.allclose(ls.tied_update(xt_t, x0_t, z, t, s, ab, betas, codes), got, rtol=1e-13, atol=1e-13)  # others' draws unused


def test_tied_jump():
    ab, _ = _tables()
    r = np.random.default_rng(3)
    l, z = r.normal(size=(4, 3)) * 3, r.normal(size=(4, 3))
    s, t = np.array([0, 10, 5, 98]), np.array([37, 60, 6, 99])
    codes = np.array([0, 1, 2, 2], dtype=np.int32)
    got = ls.tied_jump(l, z, s, t, ab, codes)
    for b in range(4):
        ratio = ab[t[b]] / ab[s[b]] if s[b] > 0 else ab[t[b]]
        for i in range(3):
            j = 0 if (codes[b] > 0 and i <= codes[b]) else i
            assert np.isclose(got[b, i], np.sqrt(ratio) * l[b, j] + np.sqrt(1 - ratio) * z[b, j], rtol=1e-13)
    assert got[1, 0] == got[1, 1] and (got[2] == got[2, 0]).all() and (got[3] == got[3, 0]).all()
    assert np.array_equal(ls.tied_jump(l, z, s, t, ab, codes, len_mask=[1, 1, 1, 1]), ls.tied_jump(l, z, s, t, ab, np.zeros(4)))
