"""The guards of the sampling-step corner cases (tests/sampling_corner_cases.py), without a GPU: the batch reaches what it is
meant to reach, no atom of any case sits near a Gumbel tie in float64 (so test_gpu_sampling_corners.py may demand equal classes),
the S = 124 step changes classes on both sides of lane 64's boundary, and the gathered references can tell a wrong crystal
lookup from the right one."""
import numpy as np
import pytest

from tests import sampling_corner_cases as C

SPECIES_KINDS = ("plain", "reverse", "jump")  # the kinds with a species rule (the tied and eta steps share "reverse"'s)


def _reference(model, kind):
    om = C.model_and_oracle(model)[1]
    v = C.inputs(model, kind)
    fn = {"plain": lambda t, s: C.reverse_at(om, v, t, s, "plain"), "reverse": lambda t, s: C.reverse_at(om, v, t, s, "sched"),
          "invert": lambda s, t: C.invert_at(om, v, s, t), "jump": lambda s, t: C.jump_at(om, v, s, t),
          "corrector": lambda t, _: C.corrector_at(om, v, t, False)}[kind]
    return v, C.per_pair(model, kind, fn)


def test_the_batch_reaches_the_corners():
    """67 crystals (a second lattice workgroup with three live crystals, the last group of four partly live, two levels of the
    64-ary crystal search), one-atom crystals next to each other's boundaries, 130 atoms in the last; tied crystals past lane 23
    (crystal 6 on) and past crystal 64; neighbouring crystals never hold the same pair."""
    assert C.B == 67 and C.N == 326 and C.COUNTS[-1] == 130 and C.COUNTS[:5] == [1, 2, 3, 5, 4]
    assert C.B > 64 and (C.B - 64) % 4 != 0
    assert any(c == 1 for b, c in enumerate(C.CODES) if b >= 16) and any(c == 2 for b, c in enumerate(C.CODES) if b >= 16)
    assert any(c != 0 for b, c in enumerate(C.CODES) if b >= 64)
    for model in C.MODELS:
        T = C.MODELS[model]["num_timesteps"]
        for kind in C.KINDS:
            first, second = C.pairs_per_crystal(model, kind)
            n = len(C.pair_list(model, kind))
            assert np.gcd(n, 3) == 1, (model, kind, "tie codes and pairs cycle together")
            if n > 1:
                assert np.all((first[1:] != first[:-1]) | (second[1:] != second[:-1])), (model, kind)
            if kind in ("plain", "reverse"):
                assert np.all((1 <= first) & (first <= T) & (0 <= second) & (second < first)), (model, kind)
            elif kind == "invert":
                assert np.all((1 <= first) & (first <= T - 1) & (first < second) & (second <= T)), (model, kind)
            elif kind == "jump":
                assert np.all((0 <= first) & (first < second) & (second <= T)), (model, kind)
            else:
                assert np.all((1 <= first) & (first <= T)), (model, kind)
        assert (C.inputs(model, "reverse").x_t == C.MODELS[model]["S"] - 1).sum() * 3 >= C.N


@pytest.mark.parametrize("kind", SPECIES_KINDS)
@pytest.mark.parametrize("model", sorted(C.MODELS))
def test_no_atom_is_near_a_gumbel_tie(model, kind):
    """The species rules are Gumbel arg-maxima, which fp32 can flip only at a near-tie: in float64 every atom's top-two margin is
    at least 1e-3 (10 x the project's MARGIN) at its own crystal's pair, so the GPU tests demand every class equal.  S = 124:
    the step's changed atoms land on both sides of class 64 (a lane's first and second class)."""
    v, res = _reference(model, kind)
    ref = C.gather(res, model, kind)
    print(f"{model} {kind} (seed {v.seed}): smallest float64 margin {ref['margin'].min():.3g}")
    assert ref["margin"].min() >= C.MARGIN
    if v.S == 124 and kind != "jump":
        changed = ref["types"] != v.x_t.numpy()
        assert (changed & (ref["types"] < 64)).any() and (changed & (ref["types"] >= 64)).any()
        assert (v.x_t.numpy() == 123).any() and (ref["types"] == 123).any()


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("model", sorted(C.MODELS))
def test_the_references_can_tell_a_wrong_crystal(model, kind):
    """Blind spot 1, without a kernel: the gathered reference evaluated again with each atom's crystal replaced by its
    neighbour's (either side), as a wrong lookup would.  For at least half of the atoms whose neighbouring crystal holds another
    pair the two differ by more than 10 x the GPU bound on positions, or in class."""
    v, res = _reference(model, kind)
    ref = C.gather(res, model, kind)
    for shift in (1, -1):
        sel, other = C.neighbour_holds_another_pair(model, kind, shift)
        if not sel.any():
            assert (model, kind) == ("S12-T2", "invert")  # one valid climb, 1 -> 2: nothing to tell apart
            continue
        wrong = C.gather(res, model, kind, crystal_of_atom=other)
        told = C.wrapped(ref["frac"], wrong["frac"]).max(axis=1) > 10 * C.POS_TOL[kind]
        if "types" in ref:
            told |= ref["types"] != wrong["types"]
        print(f"{model} {kind} shift {shift}: {int(told[sel].sum())} of {int(sel.sum())} atoms told apart")
        assert 2 * int(told[sel].sum()) >= int(sel.sum())
