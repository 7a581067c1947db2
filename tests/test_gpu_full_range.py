"""The full-range kernels (bf16x6: edge_bf16.hip, node_bf16.hip, the K pair conv behind them, bf16x6 products in the
training GEMMs) against the float64 oracle, on models that choose them by themselves -- no `set_variant`, no environment
variable -- and at the benchmark's size.  arreau_model_create starts a model on them when a weight-derived activation bound
exceeds 64 x 65504 (edge chain and ConvNext chain separately) or when a packed weight is 60000 or more (f16_ok = 0: both).
The three models below get there by scaling one layer up and its consumer down, so their outputs stay tame and a float32
evaluation of them stays accurate; the bf16x6 kernels are documented as fp32-grade, so they are held to the parity bounds
plus what float32 itself costs on these weights.  Needs an MI355X: run with `-m gpu`."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import oracle_from_module, random_state, slots_from_edges
from tests.test_gpu_model_shapes import _check_reverse_step, _engine_scores, _ragged_state, _training_inputs
from tests.test_gpu_parity import TOL, _oracle_scores, _to_dev, assert_scores_close, loop_bitwise_across_eager_graph_and_per_step, pooled_bound
from tests.test_gpu_training import assert_step_close_to_float64

pytestmark = pytest.mark.gpu

F64 = torch.float64
F16_SLACK = 64.0 * 65504.0  # model.hip: a bound beyond this starts the chain on bf16x6
F32_LIMIT = 1e-3            # the float32 oracle's distance from float64, relative to the tensor's largest entry, must stay below


def _node_bound_model(m):
    """(a) ConvNext hidden units of layer 1 x 1e6 (linear_1 x 5e5 -- its largest weight stays below 60000 -- on a LayerNorm
    output x 2), linear_2 x 1e-6: the node bound passes 64 x 65504, the edge chain is untouched"""
    layer = m.model.interaction_layers[1]
    layer.linear_1.weight.mul_(5.0e5)
    layer.norm.weight.mul_(2.0)
    layer.norm.bias.mul_(2.0)
    layer.linear_2.weight.mul_(1.0e-6)


def _edge_bound_model(m):
    """(b) the basis (basis_fn's second Linear, weight and bias) x 1e5, every layer's kernel projection x 1e-5: the edge bound
    passes 64 x 65504, the ConvNext chain is untouched"""
    m.model.basis_fn[3].weight.mul_(1.0e5)
    m.model.basis_fn[3].bias.mul_(1.0e5)
    for layer in m.model.interaction_layers:
        layer.conv.kernel.weight.mul_(1.0e-5)


def _fp16_weight_model(m):
    """(c) one weight of layer 2's linear_1 set to 65000 (it does not fit the fp16x3 planes: f16_ok = 0), its hidden unit's
    column of linear_2 x 1e-5; both bounds stay within the slack, so the weight alone decides"""
    layer = m.model.interaction_layers[2]
    layer.linear_1.weight[5, 17] = 6.5e4
    layer.linear_2.weight[:, 5].mul_(1.0e-5)


# id -> (scaling, kernel families arreau_model_create chooses, which bound passes the slack)
MODELS = {
    "node-bound": (_node_bound_model, dict(edge_kernel="fp16x3", mlp_kernel="bf16x6"), (False, True)),
    "edge-bound": (_edge_bound_model, dict(edge_kernel="bf16x6", mlp_kernel="fp16x3-16x16x32"), (True, False)),
    "fp16-weight": (_fp16_weight_model, dict(edge_kernel="bf16x6", mlp_kernel="bf16x6"), (False, False)),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", params=list(MODELS), ids=list(MODELS))
def fr_model(dev, request):
    from arreau_amd.checkpoint import make_synthetic_model
    scale, families, beyond = MODELS[request.param]
    m = make_synthetic_model(S=12, seed=7, num_timesteps=100)
    with torch.no_grad():
        scale(m)
    m = m.to(dev)
    return SimpleNamespace(m=m, om=oracle_from_module(m, F64), om32=oracle_from_module(m, torch.float32), name=request.param,
                           families=families, beyond=beyond, S=12, T=100, k=8)


def _assert_families(fm):
    st = fm.m.engine().status()
    want = dict(fm.families, conv_variant=1, readout_kernel=1)  # K pair conv at this size (below the basis form's 2,000 receivers)
    assert {k: st[k] for k in want} == want, (fm.name, st)
    assert st["flags"] == 0, (fm.name, st)
    return st


def test_the_model_chooses_the_full_range_kernels_itself(dev, fr_model):
    fm = fr_model
    st = fm.m.engine().status()
    assert (st["edge_activation_bound"] > F16_SLACK, st["node_activation_bound"] > F16_SLACK) == fm.beyond, (fm.name, st)
    state = random_state(fm.S, [8, 5, 3], 4)
    f, ty, le, an, off = _to_dev(dev, *state)
    fm.m.engine().predict_scores(f, ty, le, an, torch.full((3,), 50, device=dev, dtype=torch.int32), off)
    _assert_families(fm)


@pytest.mark.parametrize("t_end", ["t=1", "t=T"])
def test_scores_match_float64_oracle(dev, fr_model, t_end):
    """Per output tensor: the parity bound (assert_scores_close) plus twice the float32 oracle's distance from float64 on the
    same edges, which these weights keep below 1e-3 of the tensor's largest entry -- given edges, own edges, sampler-like."""
    fm = fr_model
    t = 1 if t_end == "t=1" else fm.T
    legs = [(_ragged_state(fm.S, 10 if t == 1 else 20), True, 33), (_ragged_state(fm.S, 10 if t == 1 else 20), False, 33),
            (random_state(fm.S, [9, 2, 17], 30 + t, sampler_like=True), True, 20)]
    worst, worst32 = np.zeros(3), np.zeros(3)
    for state, teacher_forced, apc in legs:
        got, want64, want32, deg = _engine_scores(fm, dev, state, t, teacher_forced)
        if teacher_forced and apc == 33:
            assert int(deg.min()) == 0 and len(deg) % 8 != 0  # a degree-0 receiver; N not a multiple of 8
        for i, (name, a, w64, w32) in enumerate(zip(("eps", "logits", "len0"), got, want64, want32)):
            big = float(w64.abs().max())
            d32 = float((w32.double() - w64).abs().max())
            assert d32 <= F32_LIMIT * big, (fm.name, name, d32, big)  # else the bound below would test nothing
            parity = (TOL * max(1.0, big), TOL * max(1.0, big / 8.0), pooled_bound(w64, apc))[i]
            err = float((a.detach().cpu().double() - w64).abs().max())
            assert err <= parity + 2 * d32, (fm.name, t, teacher_forced, name, err, parity, d32)
            worst[i], worst32[i] = max(worst[i], err), max(worst32[i], d32)
        _assert_families(fm)
    print(f"\n[{fm.name} {t_end}] worst against float64: eps {worst[0]:.2e} logits {worst[1]:.2e} len0 {worst[2]:.2e}; "
          f"float32 oracle: eps {worst32[0]:.2e} logits {worst32[1]:.2e} len0 {worst32[2]:.2e}")


@pytest.mark.parametrize("t_end", ["t=1", "t=T"])
def test_reverse_step_matches_float64_oracle(dev, fr_model, t_end):
    _check_reverse_step(fr_model, dev, 1 if t_end == "t=1" else fr_model.T)


def test_training_step_matches_float64_oracle_autograd(dev, fr_model):
    """One training step on the model's own choice of arithmetic: the loss and every gradient against float64 oracle autograd
    (GRAD_TOL x the tensor's largest entry + twice float32 autograd's distance from float64).  The step must come out right
    the first time -- not through the training loop's switch to the full-range products after a non-finite step."""
    import warnings
    fm = fr_model
    batch, lattice0, timestep, noise = _training_inputs(fm.S, fm.T)
    mm = copy.deepcopy(fm.m)
    for layer in mm.model.interaction_layers:
        layer.conv.callibrated.fill_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loss = mm.training_step(batch, timestep=timestep, noise=noise)
    assert bool(torch.isfinite(loss)) and not getattr(mm, "_train_full_range", False), (fm.name, float(loss))
    assert not any("bf16x6" in str(w.message) for w in caught), [str(w.message) for w in caught]
    grads = {n: p.grad.clone() for n, p in mm.named_parameters() if p.grad is not None}
    worst = assert_step_close_to_float64(mm, loss, grads, batch, lattice0, timestep, noise, fm.name)
    assert mm._engine.status()["flags"] == 0
    print(f"\n[{fm.name} training] loss {float(loss):.6f}; worst gradient error relative to its largest entry {worst[0]:.2e}, "
          f"float32 oracle autograd {worst[1]:.2e} ({worst[2]})")


# ------------------------------------------------------------------------------------------- the benchmark's size
@pytest.fixture(scope="module")
def bench_model(dev):
    """S = 90, T = 1000 (the shipped architecture) on the full-range kernels: at 5,120 receivers the default path runs the
    basis form; this one runs the streamed K pair conv (conv_kernel_streamed's persistent loop over many receivers)."""
    from arreau_amd.checkpoint import make_synthetic_model
    m = make_synthetic_model(S=90, seed=1234).to(dev)
    m.engine().set_variant(3, 1)
    return m


BENCH_FAMILIES = dict(edge_kernel="bf16x6", mlp_kernel="bf16x6", conv_variant=1)


def test_the_benchmark_size_against_the_oracle(dev, bench_model):
    """test_the_benchmark_path_against_the_oracle_at_its_own_size on the full-range kernels: 256 crystals x 20 atoms,
    teacher-forced edges, first and last timesteps against the fp32 oracle (assert_scores_close); at t = T against float64,
    within twice the exact fp32-MFMA kernels' distance (plus one fp32 ulp of slack)."""
    m = bench_model
    om32 = oracle_from_module(m, torch.float32)
    B, n = 256, 20
    state = random_state(90, [n] * B, 17, cell=(4.0, 8.0))
    f, ty, le, an, off = _to_dev(dev, *state)
    eng = m.engine()
    for t in (999, 1):
        eps_o, logits_o, len0_o, (ei, dists, direction, _c, _l) = _oracle_scores(om32, *state, t)
        deg, src, sdir, sdist = slots_from_edges(ei, dists, direction, B * n, 8)
        edges = tuple(x.to(dev).contiguous() for x in (deg, src, sdir, sdist))
        t_c = torch.full((B,), t, device=dev, dtype=torch.int32)
        got = eng.predict_scores(f, ty, le, an, t_c, off, edges=edges)
        st = eng.check_status()
        assert {k: st[k] for k in BENCH_FAMILIES} == BENCH_FAMILIES, st
        e, l, g = assert_scores_close(got, (eps_o, logits_o, len0_o), f"full range, t = {t}")
        print(f"\n[bench size, full range, vs fp32 oracle, t = {t}] eps {e:.2e} logits {l:.2e} len0 {g:.2e}")
        if t == 999:
            om64 = oracle_from_module(m, F64)
            eps64, logits64, len064, _ = _oracle_scores(om64, *state, t, edges=(ei, dists.double(), direction.double()), dtype=F64)
            eng.set_variant(0, 0)
            try:
                exact = eng.predict_scores(f, ty, le, an, t_c, off, edges=edges)
                stx = eng.check_status()
            finally:
                eng.set_variant(3, 1)
            assert stx["edge_kernel"] == "fp32-mfma" and stx["mlp_kernel"] == "fp32-mfma", stx
            for name, a, b, ref, ulp in (("eps", got[0], exact[0], eps64, 1e-8), ("logits", got[1], exact[1], logits64, 5e-7),
                                         ("len0", got[2], exact[2], len064, 4e-6)):
                err_fr = float((a.cpu().double() - ref).abs().max())
                err_exact = float((b.cpu().double() - ref).abs().max())
                print(f"   [fp64 ref] {name}: bf16x6 kernels {err_fr:.2e}, fp32-MFMA kernels {err_exact:.2e}")
                assert err_fr <= 2 * err_exact + ulp, (name, err_fr, err_exact)


def test_loop_at_the_benchmark_size_is_bitwise_across_eager_graph_and_per_step(dev, bench_model):
    loop_bitwise_across_eager_graph_and_per_step(bench_model.engine(), BENCH_FAMILIES)
