"""Training a model without layer_scale (the reference's --layer_scale 0: the ConvNext block has no such parameter and the
state_dict no such key) beyond one step.  The library has code of its own for it: a plane of ones stands in for the tensor in
every kernel that multiplies by it, the backward pass writes no d(out) ahead and runs no combined column-sum pass for
d(layer_scale) / d(linear_2.bias) -- a stand-alone scale by the ones and a separate column sum instead --, the flat gradient
buffer keeps a slice no parameter maps to, and the weight refresh after an optimizer step has no source for the plane.  On the
17-atom batch of test_gpu_training.py, S = 12, T = 100.  Needs an MI355X: run with `-m gpu`.

Measured on an MI355X (gradient errors relative to the tensor's largest entry; in brackets float32 oracle autograd's own distance
from float64): first step, loss 11.5568, worst gradient 4.0e-6 (2.5e-6); second step after the optimizer step, loss 16.3229, worst
gradient 1.2e-6 (6.3e-7), scores at the updated weights against the float32 oracle eps 4.1e-8, logits 1.1e-6, len0 9.5e-7; fused
ConvNext forward against the product form, worst gradient difference 5.6e-6 (bound 2e-5); the launch forms bit for bit."""
import copy

import pytest
import torch

from oracle import training as TR
from tests.helpers import assert_scores_close, oracle_from_module
from tests.test_gpu_training import assert_step_close_to_float64, make_setup

pytestmark = pytest.mark.gpu

PER_LAYER = ("conv.kernel.weight", "conv.fiber_kernel.weight", "conv.bias", "norm.weight", "norm.bias", "linear_1.weight",
             "linear_1.bias", "linear_2.weight", "linear_2.bias")


@pytest.fixture(scope="module")
def setup():
    m, om, *rest = make_setup(layer_scale=0.0)
    assert not any("layer_scale" in k for k in m.state_dict()) and m.model.interaction_layers[0].layer_scale is None
    for layer in m.model.interaction_layers:  # (no rescale of the conv weights behind a first step: every copy trains these weights)
        layer.conv.callibrated.fill_(True)
    return (m, om, *rest)


def _grads(mm):
    return {n: p.grad.detach().clone() for n, p in mm.named_parameters() if p.grad is not None}


def _two_steps(m, batch, timestep, noise, lr=None):
    """[(loss, gradients)] of two training steps of a copy of `m` with an optimizer step between them"""
    from arreau_amd.train import optimizer_step
    mm = copy.deepcopy(m)
    opt = mm.configure_optimizers(max_epochs=10)["optimizer"]
    for g in opt.param_groups:
        g["lr"] = g["lr"] if lr is None else lr
    out = []
    for _ in range(2):
        loss = mm.training_step(batch, timestep=timestep, noise=noise)
        out.append((float(loss), _grads(mm)))
        optimizer_step(mm, opt, world_size=1)
    return out


def test_every_trainable_tensor_against_float64_and_the_same_bits_when_repeated(setup):
    """One step against float64 oracle autograd (assert_step_close_to_float64: every trainable tensor compared): nine gradients
    per layer, none of them missing, none for layer_scale; the same loss and gradient bits when the step is repeated."""
    m, om, batch, lattice0, timestep, noise = setup
    mm = copy.deepcopy(m)
    loss = mm.training_step(batch, timestep=timestep, noise=noise)
    assert mm.engine(for_training=True).cfg.has_layer_scale == 0
    params = dict(mm.named_parameters())
    for l in range(5):
        for key in PER_LAYER:
            assert params[f"model.interaction_layers.{l}.{key}"].grad is not None, (l, key)
    grads = _grads(mm)
    assert not any("layer_scale" in n for n in grads) and len(grads) == 9 + 5 * (9 + 2)
    assert all(float(g.abs().max()) > 0 for g in grads.values())
    worst = assert_step_close_to_float64(mm, loss, grads, batch, lattice0, timestep, noise, "no layer_scale")
    for _ in range(2):
        again = mm.training_step(batch, timestep=timestep, noise=noise)
        assert float(again) == float(loss)
        for n, g in _grads(mm).items():
            assert torch.equal(g, grads[n]), ("step not bitwise repeatable", n)
    assert mm._engine.status()["flags"] == 0
    print(f"\n[no layer_scale, one step] loss {float(loss):.6f}; worst gradient error relative to its largest entry {worst[0]:.2e}, "
          f"float32 oracle autograd {worst[1]:.2e} ({worst[2]}), {len(grads)} tensors")


@pytest.mark.parametrize("fuse,side", [("0", "1"), ("1", "0"), ("0", "0")], ids=["FUSE=0", "SIDE_STREAM=0", "both=0"])
def test_merged_launches_are_bitwise_the_one_kernel_per_operation_sequence(setup, monkeypatch, fuse, side):
    """test_gpu_training.py's test of the merged launches on this model: ARREAU_TRAIN_FUSE=0 (one kernel per operation) and
    ARREAU_TRAIN_SIDE_STREAM=0 (one stream) give the loss and every gradient of the default form bit for bit, over two steps with
    an optimizer step between them.  Without layer_scale both forms scale d(x) by the plane of ones in a launch of its own and
    take d(linear_2.bias) as a separate column sum; they differ in where that sum's chunks are added up."""
    m, om, batch, lattice0, timestep, noise = setup
    want = _two_steps(m, batch, timestep, noise)
    monkeypatch.setenv("ARREAU_TRAIN_FUSE", fuse)
    monkeypatch.setenv("ARREAU_TRAIN_SIDE_STREAM", side)
    got = _two_steps(m, batch, timestep, noise)
    for (la, ga), (lb, gb) in zip(want, got):
        assert la == lb, (la, lb)
        assert ga.keys() == gb.keys() and len(ga) == 9 + 5 * (9 + 2)
        for n in ga:
            assert torch.equal(ga[n], gb[n]), ("merged launches changed a gradient", n, float((ga[n] - gb[n]).abs().max()))


def test_fused_convnext_training_forward_against_the_product_form(setup, monkeypatch):
    """ARREAU_TRAIN_FUSED_MLP=1 (the ConvNext block through the sampling step's kernel, which multiplies by the plane of ones)
    against =0 (a LayerNorm launch and two products), with the bound of test_gpu_training.py's test of the same name: 1e-6 on the
    loss, 2e-5 of each gradient's largest entry; again after an optimizer step."""
    m, om, batch, lattice0, timestep, noise = setup
    results = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("ARREAU_TRAIN_FUSED_MLP", fused)
        results[fused] = _two_steps(m, batch, timestep, noise, lr=1e-3)
    worst = 0.0
    for (la, ga), (lb, gb) in zip(results["1"], results["0"]):
        assert abs(la - lb) <= 1e-6 * max(1.0, abs(lb)), (la, lb)
        assert ga.keys() == gb.keys() and len(ga) == 9 + 5 * (9 + 2)
        for n in ga:
            scale = max(float(gb[n].abs().max()), 1e-30)
            err = float((ga[n] - gb[n]).abs().max()) / scale
            assert err <= 2e-5, (n, err)
            worst = max(worst, err)
    print(f"\n[no layer_scale, fused ConvNext forward against the product form] worst gradient difference relative to its largest "
          f"entry {worst:.2e}")


def test_second_step_after_an_optimizer_step_against_float64(setup):
    """training_step -> optimizer_step (ClipAdam on the flat gradient buffer: its step_flat must take the flat path, although
    the buffer's layer_scale slice belongs to no parameter) -> training_step: the second step's loss and every gradient against
    float64 oracle autograd at the updated weights -- the weight refresh on the device with no layer_scale source.  Then the
    scores at the updated weights against the float32 oracle at the suite's bound (assert_scores_close): the training forward of
    the refreshed engine, whose plane of ones the refresh must have left alone, and predict_scores of the engine the module
    packs for sampling from the updated parameters (the refreshed one refuses to sample: its packed planes are stale)."""
    from arreau_amd import _hip
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    from arreau_amd.optim import ClipAdam
    from arreau_amd.train import optimizer_step
    m, om, batch, lattice0, timestep, noise = setup
    mm = copy.deepcopy(m)
    opt = mm.configure_optimizers(max_epochs=10)["optimizer"]
    assert isinstance(opt, ClipAdam)
    for g in opt.param_groups:
        g["lr"] = 1e-3
    norms, step_flat = [], opt.step_flat
    def spy(*a, **kw):
        norms.append(step_flat(*a, **kw))
        return norms[-1]
    opt.step_flat = spy
    before = {n: p.detach().clone() for n, p in mm.named_parameters()}
    mm.training_step(batch, timestep=timestep, noise=noise)
    eng = mm._engine
    norm = optimizer_step(mm, opt, world_size=1)
    assert len(norms) == 1 and norms[0] is not None and norm is norms[0] and float(norm) > 0, norms
    assert mm._engine is eng and eng.stale_for_sampling
    moved = {n for n, p in mm.named_parameters() if not torch.equal(p.detach(), before[n])}
    assert moved == {n for n, p in mm.named_parameters() if p.requires_grad and p.numel() > 0}, sorted(moved)
    loss = mm.training_step(batch, timestep=timestep, noise=noise)
    assert mm._engine is eng
    grads = _grads(mm)
    assert not any("layer_scale" in n for n in grads) and len(grads) == 9 + 5 * (9 + 2)
    worst = assert_step_close_to_float64(mm, loss, grads, batch, lattice0, timestep, noise, "second step")
    # scores at the updated weights on the oracle's own noised batch
    om2 = oracle_from_module(mm, torch.float32)
    _, po = TR.diffusion_loss(om2, batch.X0, batch.A0, lattice0, batch.num_atoms, timestep, *noise, return_parts=True)
    want = (po["pred_eps"], po["logits"], po["pred_lengths"])
    dev = eng.device
    args = (po["noisy_frac"].to(dev).contiguous(), po["noisy_types"].to(dev, torch.int32).contiguous(),
            po["noisy_lengths"].float().to(dev).contiguous(), po["angles"].float().to(dev).contiguous(),
            timestep.to(dev, torch.int32).contiguous(), crystal_offsets(batch.num_atoms, dev))
    e_train = assert_scores_close(eng.train_forward(*args), want, "training forward of the refreshed engine")
    with pytest.raises(_hip.ArreauHipError):
        eng.predict_scores(*args)
    fresh = mm.engine()
    assert fresh is not eng and not fresh.stale_for_sampling and fresh.cfg.has_layer_scale == 0
    e_sample = assert_scores_close(fresh.predict_scores(*args), want, "predict_scores at the updated weights")
    st = fresh.status()
    assert st["flags"] == 0 and st["edge_kernel"] == "fp16x3" and st["mlp_kernel"] == "fp16x3-16x16x32", st
    print(f"\n[no layer_scale, second step] loss {float(loss):.6f}; worst gradient error relative to its largest entry {worst[0]:.2e}, "
          f"float32 oracle autograd {worst[1]:.2e} ({worst[2]}); scores against the float32 oracle (eps, logits, len0): training "
          f"forward " + " ".join(f"{e:.2e}" for e in e_train) + ", predict_scores " + " ".join(f"{e:.2e}" for e in e_sample))
