"""Species control on the host (arreau_amd/diffusion/species.py; rules in include/arreau_hip.h): element sets to admission rows
and their packing, the validation, and the float64 restatement of the rule -- against the D3PM formula the DDIM test restates,
its exclusion property, and the near-tie cap on the shared inputs that the GPU comparison relies on.  No GPU."""
import numpy as np
import pytest
import torch

from arreau_amd.diffusion import species as sp
from arreau_amd.diffusion.tools.atomic_number_table import AtomicNumberTable
from tests import species_cases as C

ZT = AtomicNumberTable([3, 8, 26, 57, 2001])  # Li O Fe La + the mask state


# ------------------------------------------------------------------------------------------------ element sets, packing
def test_resolve_elements():
    one = sp.resolve_elements(["Li", 8], ZT, 3)
    assert one.shape == (3, 5) and one.dtype == bool
    assert (one == np.array([True, True, False, False, False])).all()
    per = sp.resolve_elements([["Li", "O"], None, [26]], ZT, 3)
    assert per.tolist() == [[True, True, False, False, False], [True] * 5, [False, False, True, False, False]]
    assert sp.resolve_elements(None, ZT, 2).all()
    assert sp.resolve_elements([np.int64(57), "Fe"], ZT, 1).tolist() == [[False, False, True, True, False]]
    assert sp.resolve_elements(({"La"}, ("O",)), ZT, 2).tolist() == [[False, False, False, True, False], [False, True, False, False, False]]
    # every element of the table: only "no atom ends as the mask state"
    every = sp.resolve_elements([3, 8, 26, 57], ZT, 1)
    assert every[0, :-1].all() and not every[0, -1]
    sp.check_rows(every)


@pytest.mark.parametrize("elements,B,match", [
    (["Li", "Xx"], 2, "unknown element symbol"),
    (["Li", "C"], 2, "not in the model's table"),
    ([3, 6], 2, "not in the model's table"),
    ([2001], 2, "not in the model's table"),
    ([], 2, "must not be empty"),
    ([["Li"], []], 2, "must not be empty"),
    ([["Li"], None, ["O"]], 2, "3 entries for a batch of 2"),
    ("Li", 2, "collection"),
    ([["Li"], "O"], 2, "collection"),
    ([1.5], 2, "neither"),
])
def test_resolve_elements_rejects(elements, B, match):
    with pytest.raises(ValueError, match=match):
        sp.resolve_elements(elements, ZT, B)


def test_rows_without_an_ordinary_class_are_rejected():
    rows = np.zeros((2, 5), dtype=bool)
    rows[0, 1] = True
    rows[1, 4] = True  # the mask class alone
    with pytest.raises(ValueError, match="crystal 1 admits no ordinary class"):
        sp.check_rows(rows)


def test_held_species_outside_their_set():
    rows = sp.resolve_elements([["Li", "O"], None], ZT, 2)
    crystal = np.array([0, 0, 1, 1])
    sp.check_held(rows, crystal, [0, 1, 4, 2], np.ones(4, bool), "held")
    sp.check_held(rows, crystal, [3, 1, 4, 2], [False, True, True, True], "held")  # an atom that is not held is not checked
    with pytest.raises(ValueError, match="atom 0 of crystal 0 holds class 3"):
        sp.check_held(rows, crystal, [3, 1, 4, 2], np.ones(4, bool), "held")
    with pytest.raises(ValueError, match="atom 1 of crystal 0 holds class 4"):  # the mask class of a restricted crystal
        sp.check_held(rows, crystal, [0, 4, 4, 2], np.ones(4, bool), "held")


@pytest.mark.parametrize("S", [5, 12, 32, 33, 64, 65, 124])
def test_pack_and_unpack(S):
    rng = np.random.RandomState(S)
    rows = rng.rand(9, S) < 0.4
    rows[0], rows[1] = True, False
    words = sp.pack_rows(rows)
    assert words.shape == (9, 4) and words.dtype == np.uint32
    for b in range(9):
        for c in range(S):
            assert bool((int(words[b, c >> 5]) >> (c & 31)) & 1) == bool(rows[b, c])
    assert (sp.unpack_rows(words, S) == rows).all()
    # bits at or above S are ignored
    noisy = words.copy()
    for c in range(S, 128):
        noisy[:, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    assert (sp.unpack_rows(noisy, S) == rows).all()
    if S == 124:
        w = sp.pack_rows(C.rows_of([{31}, {32}, {63}, {64}, {122}, {1, 40, 70, 100, 122}], S))
        assert w.tolist() == [[1 << 31, 0, 0, 0], [0, 1, 0, 0], [0, 1 << 31, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1 << 26],
                              [2, 1 << 8, 1 << 6, (1 << 4) | (1 << 26)]]
    with pytest.raises(ValueError):
        sp.pack_rows(np.ones((1, 125), bool))


def test_validate_temperature():
    assert sp.validate_temperature(1) == 1.0 and sp.validate_temperature(0.0) == 0.0 and sp.validate_temperature("0.5") == 0.5
    assert str(sp.validate_temperature(-0.0)) == "0.0"
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "x"):
        with pytest.raises(ValueError):
            sp.validate_temperature(bad)


# ------------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module", params=["S12", "S124"])
def model(request):
    S = C.SIZES[request.param]
    q1t, qm = C.tables(S)
    return request.param, S, q1t.double(), qm.double()


@pytest.mark.parametrize("t,s", C.PAIRS)
def test_all_ones_rows_at_temperature_one_are_todays_formula(model, t, s):
    """species_step on all-ones rows at tau = 1 against _d3pm_post and the Gumbel arg-max of tests/test_gpu_ddim_sampling.py."""
    from tests.test_gpu_ddim_sampling import _d3pm_post
    _, S, q1t, qm = model
    _, logits, _, _, _, u, x_t = C.step_inputs(S, t)
    cls, margin = sp.species_step(q1t, qm, logits, x_t, t, s, u, np.ones((len(C.COUNTS), S), bool), C.crystal_index(), 1.0)
    post = _d3pm_post(q1t, qm, logits.double(), x_t, t, s)
    val = post + (-torch.log(-torch.log(torch.clip(u.double(), 1e-6, 1.0)))) * (1.0 if t != 1 else 0.2)
    assert np.array_equal(cls, torch.argmax(val, dim=-1).numpy())
    top = torch.topk(val, 2, dim=-1).values
    assert np.allclose(margin, (top[:, 0] - top[:, 1]).numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("tau", C.TAUS)
@pytest.mark.parametrize("t,s", C.PAIRS)
@pytest.mark.parametrize("name,group", C.CASES)
def test_exclusion_and_the_near_tie_cap(name, group, t, s, tau):
    """No excluded class is ever chosen; a single-class row at t == 1 gives that class for every atom; and -- a condition on
    the shared inputs that the GPU comparison relies on -- at most one atom has a top-two admitted margin below MARGIN."""
    S = C.SIZES[name]
    q1t, qm = C.tables(S)
    sets = C.ROWS[name][group]
    rows, crystal = C.rows_of(sets, S), C.crystal_index()
    _, logits, _, _, _, u, x_t = C.step_inputs(S, t)
    cls, margin = sp.species_step(q1t, qm, logits, x_t, t, s, u if tau > 0 else None, rows, crystal, tau)
    E = sp.admitted(rows, t)[crystal]
    assert E[np.arange(len(cls)), cls].all()
    for b, e in enumerate(sets):
        if e is not None:
            assert not E[crystal == b][:, sorted(set(range(S - 1)) - e)].any()
            assert E[crystal == b][:, S - 1].all() == (t > 1)
            if t == 1:
                assert set(cls[crystal == b].tolist()) <= e
                if len(e) == 1:
                    assert (cls[crystal == b] == next(iter(e))).all()
    assert (margin >= 0).all()
    assert int((margin < C.MARGIN).sum()) <= 1, np.sort(margin)[:3]


def test_an_atom_outside_its_set_leaves_inside_and_nan_logits_give_the_lowest_admitted_class():
    S = 12
    q1t, qm = C.tables(S)
    rows, crystal = C.rows_of([{3, 7}], S), np.zeros(S, dtype=int)
    logits = torch.randn(S, S, generator=torch.Generator().manual_seed(1)) * 2
    u = torch.rand(S, S, generator=torch.Generator().manual_seed(2))
    x_t = torch.arange(S)  # every class enters, most of them outside {3, 7}
    for t, s in C.PAIRS:
        cls, _ = sp.species_step(q1t, qm, logits, x_t, t, s, u, rows, crystal, 1.0)
        assert set(cls.tolist()) <= ({3, 7, S - 1} if t > 1 else {3, 7})
        bad = logits.clone()
        bad[5] = float("nan")
        cls, _ = sp.species_step(q1t, qm, bad, x_t, t, s, u, rows, crystal, 1.0)
        assert cls[5] == 3
