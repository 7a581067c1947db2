"""A call does not depend on what its engine ran before.  A model owns ONE context (arreau_amd/csrc/train_net.hip: ensure_ctx),
carved for a capacity and regrown by a quarter now and then; training steps of any size run inside it, and on the shape-general
path so do predict_scores and the sampling loop.  Every other test runs one call on an engine whose buffers were sized for it.
Here one engine is handed a HISTORY -- larger, smaller, wider batches, a non-finite step, scoring and sampling in between -- and
each call is compared, bit for bit, with the same call on an engine that ran nothing else: a stride taken from the capacity, a
pad assumed clean, a stale NaN multiplied by zero, a mode field left behind or a replayed graph into a freed block would differ.
Bit equality is the right assertion because every sum of the step is ordered and every launch geometry is a function of
(N, B, model) alone.  The batches and what they guarantee: tests/engine_history_cases.py, tests/test_engine_history_cpu.py.
Needs an MI355X: run with `-m gpu`."""
import copy

import numpy as np
import pytest
import torch

from tests import engine_history_cases as C
from tests.helpers import random_state
from tests.test_gpu_parity import _to_dev
from tests.test_gpu_training import assert_step_close_to_float64

pytestmark = pytest.mark.gpu

NEVER = 10 ** 9   # STATUS_CHECK_EVERY: no schedule here reaches a second check, so the arithmetic switch of training_step stays out


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def models(dev):
    """name -> the model on the device; never used itself (no engine), only deep-copied"""
    from arreau_amd.checkpoint import make_synthetic_model
    return {name: make_synthetic_model(S=C.S, seed=1234, num_timesteps=C.T, **kw).to(dev) for name, kw in C.MODELS.items()}


@pytest.fixture(scope="module")
def cases():
    return {name: C.batch(name) for name in C.BATCHES}


def _fresh(m, callibrated=True):
    mm = copy.deepcopy(m)  # (the copy packs its own engine and gets its own context)
    if callibrated:
        for layer in mm.model.interaction_layers:
            layer.conv.callibrated.fill_(True)
    mm.STATUS_CHECK_EVERY = NEVER
    return mm


def _step(mm, case):
    """(loss, {name: gradient}) of one training step, copied: the gradients are views of a buffer the next step may reuse"""
    batch, _lattice0, timestep, noise = case
    loss = mm.training_step(batch, timestep=timestep, noise=noise)
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in mm.named_parameters() if p.grad is not None}


def _assert_same_step(got, want, tag, more_than=0):
    (loss, grads), (loss_c, grads_c) = got, want
    assert torch.equal(loss, loss_c), (tag, "loss", float(loss), float(loss_c))
    assert grads.keys() == grads_c.keys() and len(grads) > more_than, (tag, len(grads), sorted(grads.keys() ^ grads_c.keys()))
    for n in grads:
        assert torch.equal(grads[n], grads_c[n]), (tag, n, float((grads[n] - grads_c[n]).abs().max()))


@pytest.fixture(scope="module")
def control_steps(models, cases):
    """(model, batch) -> the step of a fresh engine that runs only that batch, on the default launches; computed once, shared"""
    done = {}

    def get(which, name):
        if (which, name) not in done:
            done[which, name] = _step(_fresh(models[which]), cases[name])
        return done[which, name]
    return get


# ------------------------------------------------------------------------------------------- 1. a step is a function of its batch
@pytest.mark.parametrize("which,one_kernel_per_operation", [("fused", False), ("narrow", False), ("narrow", True)],
                         ids=["fused", "narrow", "narrow-unmerged-one-stream"])
def test_training_step_is_a_function_of_its_batch(models, cases, control_steps, monkeypatch, which, one_kernel_per_operation):
    """One model runs A, BIG, A, WIDE, A, FULL, OVER, A: the context regrows at BIG, WIDE and OVER, FULL fills it to the last
    atom, and A runs in a fresh context, under BIG's leavings (every slot A leaves unused was written by BIG), under WIDE's and
    under OVER's.  Every loss and gradient equals, bit for bit, that of a fresh model that runs the batch alone; the last A step
    is also held against float64 oracle autograd, which anchors the pair to something outside the library."""
    if one_kernel_per_operation:
        monkeypatch.setenv("ARREAU_TRAIN_FUSE", "0")
        monkeypatch.setenv("ARREAU_TRAIN_SIDE_STREAM", "0")   # (read when a context is created: at every regrow too)
        control = {name: _step(_fresh(models[which]), cases[name]) for name in set(C.SCHEDULE)}
    else:
        control = {name: control_steps(which, name) for name in set(C.SCHEDULE)}
    mm = _fresh(models[which])
    for i, name in enumerate(C.SCHEDULE):
        got = _step(mm, cases[name])
        assert bool(torch.isfinite(got[0])), (which, i, name)
        _assert_same_step(got, control[name], (which, f"step {i}: {name} after {C.SCHEDULE[:i]}"), more_than=60 if which == "fused" else 20)
    assert mm._engine.status()["flags"] == 0
    worst = assert_step_close_to_float64(mm, got[0], got[1], *cases["A"], f"{which}: the last A of the history")
    print(f"\n[{which}{' unmerged' if one_kernel_per_operation else ''}] {len(C.SCHEDULE)} steps bitwise their controls', {len(got[1])} tensors; last A "
          f"against float64: worst gradient error relative to its largest entry {worst[0]:.2e}, float32 oracle autograd {worst[1]:.2e} ({worst[2]})")


# ------------------------------------------------------------------------------------------- 2. a non-finite larger step
def test_nonfinite_step_on_a_larger_batch_leaves_nothing_behind(models, cases):
    """Fused shape.  With one layer's linear_1.weight times 2^20 (exact; the overflow of
    test_training_survives_weights_that_outgrow_the_fp16_forward) the history model runs BIG: non-finite activations and
    gradients in all 50 atoms' rows of the context.  With the weight put back bit for bit, A must give what it gives on a
    control that went through the same weight refreshes and never ran BIG: a kernel that loads a stale value under a slot A
    does not use, and multiplies it by zero, now yields NaN."""
    hist, ctl = _fresh(models["fused"]), _fresh(models["fused"])
    first = [_step(mm, cases["A"]) for mm in (hist, ctl)]
    _assert_same_step(first[0], first[1], "A before the overflow", more_than=60)
    saved = []
    for mm in (hist, ctl):
        w = mm.model.interaction_layers[1].linear_1.weight
        saved.append(w.detach().clone())
        with torch.no_grad():
            w *= 2.0 ** 20
        mm.notify_parameters_changed()
    loss_big, grads_big = _step(hist, cases["BIG"])
    assert not bool(torch.isfinite(loss_big)), float(loss_big)
    st = hist._engine.status(reset=True)
    print(f"\n[non-finite BIG step] loss {float(loss_big)}; status flags {st['flags']}; "
          f"{sum(1 for g in grads_big.values() if not bool(torch.isfinite(g).all()))} of {len(grads_big)} gradient tensors non-finite")
    for mm, w0 in zip((hist, ctl), saved):
        w = mm.model.interaction_layers[1].linear_1.weight
        with torch.no_grad():
            w *= 2.0 ** -20
        assert torch.equal(w.detach(), w0)
        mm.notify_parameters_changed()
    got, want = _step(hist, cases["A"]), _step(ctl, cases["A"])
    assert bool(torch.isfinite(got[0])) and all(bool(torch.isfinite(g).all()) for g in got[1].values()), \
        [n for n, g in got[1].items() if not bool(torch.isfinite(g).all())]
    _assert_same_step(got, want, "A after the non-finite BIG step", more_than=60)
    assert_step_close_to_float64(hist, got[0], got[1], *cases["A"], "A after the non-finite BIG step")
    assert hist._engine.status()["flags"] == 0 and ctl._engine.status()["flags"] == 0


# ------------------------------------------------------------------------------------------- 3. one context for three users
def _scores(eng, dev, state, t):
    f, ty, le, an, off = _to_dev(dev, *state)
    t_c = torch.full((len(state[4]),), t, device=dev, dtype=torch.int32)
    return tuple(x.clone() for x in eng.predict_scores(f, ty, le, an, t_c, off))


def _sample(mm, use_graph):
    from arreau_amd.diffusion.inference.visualize_crystal import VisualizationSetting
    torch.manual_seed(11); np.random.seed(11)
    return mm.sample(C.SAMPLED[0], len(C.SAMPLED), VisualizationSetting.NONE, False, use_graph=use_graph, seed=123)


def test_scores_sampling_and_training_share_the_general_context(dev, models, cases, control_steps):
    """Narrow shape: predict_scores, the sampling loop and the training step use one context.  Scoring before and after a
    larger training step gives the same bits (and a never-trained engine's); the training step after scoring, which has set
    fwd_mode and N, equals its control's; a sample replayed from a captured graph equals itself after a training step has
    regrown the context and freed the block the graph pointed into (ensure_ctx drops the graph key), and equals the eager loop."""
    mm = _fresh(models["narrow"])
    eng = mm.engine()
    state = random_state(C.S, list(C.SCORED_PAIR), 1)
    r0 = _scores(eng, dev, state, 30)
    _step(mm, cases["BIG"])
    assert mm.engine() is eng and not eng.stale_for_sampling
    for name, a, b in zip(("eps", "logits", "len0"), _scores(eng, dev, state, 30), r0):
        assert torch.equal(a, b), ("scores after a training step", name, float((a - b).abs().max()))
    for name, a, b in zip(("eps", "logits", "len0"), _scores(_fresh(models["narrow"]).engine(), dev, state, 30), r0):
        assert torch.equal(a, b), ("scores of an engine that never trained", name, float((a - b).abs().max()))
    _assert_same_step(_step(mm, cases["A"]), control_steps("narrow", "A"), "A after scoring after BIG", more_than=20)
    # (A has more crystals than anything before it, so that step regrew the context and began with a new one's fields.  Once more
    # where A fits: this time the scoring call's fwd_mode and N are still in the context the step is handed)
    for name, a, b in zip(("eps", "logits", "len0"), _scores(eng, dev, state, 30), r0):
        assert torch.equal(a, b), ("scores after two training steps", name, float((a - b).abs().max()))
    _assert_same_step(_step(mm, cases["A"]), control_steps("narrow", "A"), "A after scoring, in the same context", more_than=20)
    s0 = _sample(mm, use_graph=True)
    assert np.isfinite(s0.frac_x).all() and np.isfinite(s0.lattice).all()
    n_grow = cases["GROW"][0].num_atoms
    held = np.asarray(s0.num_atoms).reshape(-1)
    assert int(held.sum()) == 30 and len(held) == 5
    assert int(n_grow.sum()) > int(held.sum()) and len(n_grow) > len(held)
    _assert_same_step(_step(mm, cases["GROW"]), control_steps("narrow", "GROW"), "GROW after sampling", more_than=20)  # regrows the context
    assert mm.engine() is eng
    for use_graph in (True, False):
        s = _sample(mm, use_graph=use_graph)
        for field in ("frac_x", "atomic_numbers", "lattice"):
            assert np.array_equal(getattr(s, field), getattr(s0, field)), ("sample after the context regrew", use_graph, field)
    assert eng.status()["flags"] == 0


# ------------------------------------------------------------------------------------------- 4. calibration in a grown context
def test_calibration_inside_a_context_that_scoring_grew(dev, models, cases):
    """Narrow shape, `callibrated` left False: the first training step calibrates the conv weights from arreau_train_conv_stats,
    here at N = 17 inside a context a 60-atom scoring call has sized and filled (five crystals, as many as A: the step fits and
    runs in that very context).  Weights, loss and gradients equal those of a control whose first call is that step."""
    hist, ctl = _fresh(models["narrow"], callibrated=False), _fresh(models["narrow"], callibrated=False)
    _scores(hist.engine(), dev, random_state(C.S, list(C.SCORED_FIRST), 3), 30)
    got, want = _step(hist, cases["A"]), _step(ctl, cases["A"])
    w0 = models["narrow"].model.interaction_layers
    for l, (a, b) in enumerate(zip(hist.model.interaction_layers, ctl.model.interaction_layers)):
        assert bool(a.conv.callibrated) and bool(b.conv.callibrated)
        assert not torch.equal(b.conv.kernel.weight, w0[l].conv.kernel.weight)  # (the control did calibrate)
        assert torch.equal(a.conv.kernel.weight, b.conv.kernel.weight), (l, "kernel")
        assert torch.equal(a.conv.fiber_kernel.weight, b.conv.fiber_kernel.weight), (l, "fiber_kernel")
    _assert_same_step(got, want, "calibrating step after a 60-atom scoring call", more_than=20)
    assert hist._engine.status()["flags"] == 0
