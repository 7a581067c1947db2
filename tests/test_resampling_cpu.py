"""RePaint resampling, the host side (no GPU): the event plan of a run (arreau_amd/diffusion/resampling.py; rules in
include/arreau_hip.h) against hand-written lists, the float64 restatement of the jump (composition, held components), and
validation of resample_passes / jump_length in sample() and generate.py before the engine is touched."""
import numpy as np
import pytest
import torch

from arreau_amd.diffusion import resampling as rs
from arreau_amd.diffusion.d3pm import D3PM
from arreau_amd.diffusion.diffusion_helpers import VE_pbc, VP_lattice
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable
from arreau_amd.lightning_wrappers.diffusion import VisualizationSetting

ZT = AtomicNumberTable(list(range(1, 12)) + [2001])
T, S = 100, 12
SIG = VE_pbc(T, 0.001, 1.0).sigmas.double().numpy()
AB = VP_lattice(T).alpha_bars.double().numpy()
QM = D3PM(None, T, num_classes=S).q_mats.double().numpy()


def _ev(kind, t, s, r):
    return rs.Event(kind, t, s, r)


# ------------------------------------------------------------------------------------------------------------ the plan
def test_plan_nine_steps_blocks_of_four_three_passes():
    steps = list(range(9, 0, -1))  # 9 .. 1, successor 0
    got = rs.plan(steps, 0, 3, 4)
    want = []
    for top, block, bottom in ((9, [9, 8, 7, 6], 5), (5, [5, 4, 3, 2], 1), (1, [1], 0)):  # the last block is short
        for r in range(3):
            if r:
                want.append(_ev("jump", top, bottom, r))
            want += [_ev("step", t, t - 1, r) for t in block]
    assert got == want
    assert got[-2:] == [_ev("jump", 1, 0, 2), _ev("step", 1, 0, 2)]  # the final block, bottom 0, is resampled too
    assert sum(e.kind == "step" for e in got) == 27 and sum(e.kind == "jump" for e in got) == 6


def test_plan_on_a_respaced_schedule():
    sched = [99, 80, 61, 40, 3, 2, 1]
    got = rs.plan(sched, 0, 2, 3)
    want = [_ev("step", 99, 80, 0), _ev("step", 80, 61, 0), _ev("step", 61, 40, 0),
            _ev("jump", 99, 40, 1), _ev("step", 99, 80, 1), _ev("step", 80, 61, 1), _ev("step", 61, 40, 1),
            _ev("step", 40, 3, 0), _ev("step", 3, 2, 0), _ev("step", 2, 1, 0),
            _ev("jump", 40, 1, 1), _ev("step", 40, 3, 1), _ev("step", 3, 2, 1), _ev("step", 2, 1, 1),
            _ev("step", 1, 0, 0), _ev("jump", 1, 0, 1), _ev("step", 1, 0, 1)]
    assert got == want
    # a run cut by max_steps: the blocks are formed from what remains, the last bottom is the cut step's successor
    got = rs.plan(sched[:4], sched[4], 2, 3)
    assert got[-3:] == [_ev("step", 40, 3, 0), _ev("jump", 40, 3, 1), _ev("step", 40, 3, 1)]


@pytest.mark.parametrize("J", [1, 4, 10, 1000])
def test_one_pass_is_the_plain_list(J):
    steps = list(range(20, 0, -1))
    assert rs.plan(steps, 0, 1, J) == [_ev("step", t, t - 1, 0) for t in steps]
    assert rs.plan([], 0, 3, J) == []


# ------------------------------------------------------------------------------------------------------ the restatement
def test_positions_compose_in_distribution():
    """s -> u -> t against s -> t: the added variances sum (VE), so the two draws have the same law."""
    for s, u, t in ((0, 5, 60), (3, 4, 99), (0, 1, 2)):
        var_st = SIG[t] ** 2 - SIG[s] ** 2
        var_sut = (SIG[u] ** 2 - SIG[s] ** 2) + (SIG[t] ** 2 - SIG[u] ** 2)
        assert var_sut == pytest.approx(var_st, rel=1e-12)
        # one unit of z moves by the standard deviation of the jump; at small sigma without cancellation
        x = np.full((1, 3), 0.5)
        z = np.array([[1.0, 0.0, -1.0]])
        got = rs.jump_positions(x, s, t, SIG, z)
        np.testing.assert_allclose(got, np.remainder(0.5 + np.sqrt(var_st) * z, 1.0), rtol=1e-12, atol=1e-15)
    rng = np.random.RandomState(0)
    x = rng.uniform(0.4, 0.6, (40000, 3))
    a = rs.jump_positions(rs.jump_positions(x, 0, 5, SIG, rng.randn(*x.shape)), 5, 9, SIG, rng.randn(*x.shape))
    b = rs.jump_positions(x, 0, 9, SIG, rng.randn(*x.shape))
    sd = np.sqrt(SIG[9] ** 2 - SIG[0] ** 2)  # small: nothing wraps
    assert np.std(a - x) == pytest.approx(sd, rel=0.02) and np.std(b - x) == pytest.approx(sd, rel=0.02)


def test_lengths_compose_in_scale_and_variance():
    for s, u, t in ((0, 30, 70), (10, 11, 99), (0, 1, 100)):
        abar = lambda k: AB[k] if k > 0 else 1.0
        r_su, r_ut, r_st = abar(u) / abar(s), abar(t) / abar(u), abar(t) / abar(s)
        assert np.sqrt(r_su) * np.sqrt(r_ut) == pytest.approx(np.sqrt(r_st), rel=1e-12)  # scale of l
        assert r_ut * (1 - r_su) + (1 - r_ut) == pytest.approx(1 - r_st, rel=1e-12, abs=1e-15)  # noise variance
        l0 = np.array([[2.0, -1.0, 0.5]])
        np.testing.assert_allclose(rs.jump_lengths(l0, s, t, AB, np.zeros((1, 3))), np.sqrt(r_st) * l0, rtol=1e-14)
        np.testing.assert_allclose(rs.jump_lengths(np.zeros((1, 3)), s, t, AB, np.ones((1, 3))), np.sqrt(1 - r_st), rtol=1e-12)


def test_species_law_follows_qbar_homogeneity():
    """Qbar_{t-s} = Qbar_{u-s} Qbar_{t-u} (the chain is time-homogeneous), so jumping s -> u -> t and s -> t mask an atom with
    the same probability; the Gumbel arg-max samples the row of Qbar_{t-s}."""
    for s, u, t in ((0, 20, 50), (5, 6, 99)):
        np.testing.assert_allclose(QM[u - s - 1] @ QM[t - u - 1], QM[t - s - 1], rtol=0, atol=1e-6)  # (float32 running products)
    rng = np.random.RandomState(1)
    n = 60000
    x = np.full(n, 3)
    got = rs.jump_species(x, 10, 60, QM, rng.uniform(size=(n, S)))
    p_mask = QM[49][3, S - 1]
    assert set(np.unique(got)) <= {3, S - 1}
    assert np.mean(got == S - 1) == pytest.approx(p_mask, abs=5 * np.sqrt(p_mask * (1 - p_mask) / n))
    # the mask class is absorbing
    assert (rs.jump_species(np.full(50, S - 1), 0, 80, QM, rng.uniform(size=(50, S))) == S - 1).all()
    # ties: the first index wins
    q = np.ones((1, 2, 2)) * 0.5
    assert rs.jump_species([0], 0, 1, q, np.full((1, 2), 0.3)).tolist() == [0]


def test_held_components_are_untouched():
    rng = np.random.RandomState(2)
    na = [3, 2]
    frac, types, lengths = rng.uniform(size=(5, 3)), np.array([0, 1, 2, 3, 4]), rng.randn(2, 3)
    z_f, z_l, u = rng.randn(5, 3), rng.randn(2, 3), rng.uniform(size=(5, S))
    s, t = np.array([0, 10]), np.array([90, 99])
    f1, t1, l1 = rs.jump(frac, types, lengths, s, t, na, SIG, AB, QM, z_f, z_l, u)
    assert not np.array_equal(f1, frac) and not np.array_equal(l1, lengths)
    f2, t2, l2 = rs.jump(frac, types, lengths, s, t, na, SIG, AB, QM, z_f, z_l, u, const_types=types, fixed_cell=True)
    assert np.array_equal(t2, types) and np.array_equal(l2, lengths) and np.array_equal(f2, f1)
    known = np.array([True, False, True, False, False])
    _, t3, l3 = rs.jump(frac, types, lengths, s, t, na, SIG, AB, QM, z_f, z_l, u, type_known=known)
    assert np.array_equal(t3[known], types[known]) and np.array_equal(t3[~known], t1[~known])
    assert np.array_equal(l3, l1)


# -------------------------------------------------------------------------------- validation before the engine is used
@pytest.mark.parametrize("R,J", [(1, 1), (1, 10), (64, 1), (3, 1000)])
def test_valid_arguments(R, J):
    assert rs.check_resampling(R, J) == (R, J)


@pytest.mark.parametrize("R,J", [(0, 10), (65, 10), (-1, 10), (2, 0), (2, -3), (2.0, 10), ("2", 10), (True, 10), (2, None),
                                 (2, 1.5), (None, 4)])
def test_invalid_arguments(R, J):
    with pytest.raises(ValueError):
        rs.check_resampling(R, J)


class _NoEngine:
    """A model whose engine must not be reached: every ValueError below comes from validation first."""
    def engine(self):
        raise AssertionError("the engine was touched before the resampling arguments were validated")


def _sample(**kw):
    from arreau_amd.diffusion.diffusion_loss import DiffusionLoss
    dl = DiffusionLoss.__new__(DiffusionLoss)
    dl.T = 100
    return dl.sample(model=_NoEngine(), z_table=ZT, num_atoms_per_sample=3, num_samples_in_batch=2, **kw)


@pytest.mark.parametrize("kw", [
    dict(resample_passes=0), dict(resample_passes=65), dict(resample_passes=1.5), dict(resample_passes="2"),
    dict(resample_passes=2, jump_length=0), dict(resample_passes=2, jump_length=-1), dict(jump_length=2.5),
    dict(resample_passes=2, num_steps=10, jump_length=0),
    dict(resample_passes=2, visualization_setting=VisualizationSetting.ALL, vis_name="x"),
    dict(resample_passes=3, visualization_setting=VisualizationSetting.ALL_DETAILED, vis_name="x"),
], ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()))
@pytest.mark.parametrize("noise", ["philox", "reference", "device"])
def test_invalid_resampling_raises_before_the_engine(kw, noise):
    with pytest.raises(ValueError):
        _sample(noise=noise, **kw)


@pytest.mark.parametrize("kw", [dict(resample_passes=2, jump_length=5),
                                dict(resample_passes=2, visualization_setting=VisualizationSetting.LAST, vis_name="x"),
                                dict(resample_passes=1, visualization_setting=VisualizationSetting.ALL, vis_name="x")])
def test_valid_resampling_reaches_the_engine(kw):
    with pytest.raises(AssertionError, match="engine was touched"):
        _sample(**kw)


def test_wrapper_validates_before_any_work():
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    w = PONITA_DIFFUSION.__new__(PONITA_DIFFUSION)
    for kw in (dict(resample_passes=0), dict(resample_passes=2, jump_length=0)):
        with pytest.raises(ValueError):
            w.sample(3, 2, **kw)


# ------------------------------------------------------------------------------------------------------------ generate.py
def test_generate_parser_takes_the_resampling_flags():
    from arreau_amd.generate import build_parser
    args = build_parser().parse_args(["--model_path", "x.ckpt"])
    assert (args.resample_passes, args.jump_length) == (1, 10)
    args = build_parser().parse_args(["--model_path", "x.ckpt", "--resample_passes", "3", "--jump_length", "5"])
    assert (args.resample_passes, args.jump_length) == (3, 5)


@pytest.mark.parametrize("argv", [["--resample_passes", "0"], ["--resample_passes", "65"], ["--resample_passes", "1.5"],
                                  ["--jump_length", "0"], ["--jump_length", "-2"], ["--jump_length", "x"]])
def test_generate_parser_rejects_bad_resampling_flags(argv, capsys):
    from arreau_amd.generate import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--model_path", "x.ckpt"] + argv)
    err = capsys.readouterr().err
    assert "resample_passes" in err or "jump_length" in err
