"""arreau_amd.optim.EMAOptimizer on the CPU: the reference's semantics (NeMo's EMAOptimizer, lightning_wrappers/callbacks.py:
173-392), its state_dict, the swap context, argument checks and the `-EMA` checkpoint twin (arreau_amd.checkpoint)."""
import copy

import pytest
import torch

from arreau_amd.optim import EMAOptimizer


def _params(seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(7, 5), (1030,), (3,), (2, 600)]
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


def _adam(ps):
    # two groups, as configure_optimizers builds them (decay on some tensors only)
    return torch.optim.Adam([{"params": ps[:2], "weight_decay": 1e-2}, {"params": ps[2:], "weight_decay": 0.0}], lr=3e-2)


def _grads(ps, step):
    g = torch.Generator().manual_seed(100 + step)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)


@pytest.mark.parametrize("every", [1, 3])
def test_ema_follows_the_reference_recurrence(every):
    """callbacks.py:174-290 restated: the average starts as a copy of the parameters taken before the first update (group order,
    then parameter order), `ema = decay * ema + (1 - decay) * p` with torch's _foreach pair at steps 0, every, 2 every, ... and the
    step counter counts every step."""
    decay = 0.9
    ps, qs = _params(), _params()
    opt = EMAOptimizer(_adam(ps), decay, every_n_steps=every)
    ref_opt = _adam(qs)
    ref_ema = None
    for step in range(8):
        _grads(ps, step)
        _grads(qs, step)
        opt.step()
        if ref_ema is None:
            ref_ema = [q.detach().clone() for g in ref_opt.param_groups for q in g["params"]]
        ref_opt.step()
        if step % every == 0:
            with torch.no_grad():
                torch._foreach_mul_(ref_ema, decay)
                torch._foreach_add_(ref_ema, [q.detach() for g in ref_opt.param_groups for q in g["params"]], alpha=1.0 - decay)
        assert opt.current_step == step + 1
        assert len(opt.ema_params) == len(ref_ema) == 4
        for e, r in zip(opt.ema_params, ref_ema):
            assert torch.equal(e, r), step
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)
    # at a step without an update the average does not move
    if every == 3:
        before = [e.clone() for e in opt.ema_params]  # current_step 8: no update
        _grads(ps, 8)
        opt.step()
        assert all(torch.equal(a, b) for a, b in zip(before, opt.ema_params))


def test_ema_starts_from_the_values_before_the_first_step():
    ps = _params()
    init = [p.detach().clone() for p in ps]
    opt = EMAOptimizer(_adam(ps), 1.0)
    for step in range(3):
        _grads(ps, step)
        opt.step()
    assert all(torch.equal(e, i) for e, i in zip(opt.ema_params, init))
    assert not any(torch.equal(p, i) for p, i in zip(ps, init))
    # decay 0: the average is the parameters
    ps = _params()
    opt = EMAOptimizer(_adam(ps), 0.0)
    for step in range(3):
        _grads(ps, step)
        opt.step()
        assert all(torch.equal(e, p) for e, p in zip(opt.ema_params, ps))


def test_state_dict_resumes_bit_for_bit():
    """Four steps, state_dict, a fresh Adam and wrapper loaded from it, four more steps: the same bits as eight steps in one go --
    parameters, Adam's moments and the average.  The format is the reference's."""
    ps = _params()
    opt = EMAOptimizer(_adam(ps), 0.8, every_n_steps=3)
    for step in range(8):
        _grads(ps, step)
        opt.step()
    qs = _params()
    opt_a = EMAOptimizer(_adam(qs), 0.8, every_n_steps=3)
    for step in range(4):
        _grads(qs, step)
        opt_a.step()
    sd = copy.deepcopy(opt_a.state_dict())
    assert set(sd) == {"opt", "ema", "current_step", "decay", "every_n_steps"}
    assert isinstance(sd["ema"], tuple) and sd["current_step"] == 4 and sd["decay"] == 0.8 and sd["every_n_steps"] == 3
    rs = [torch.nn.Parameter(q.detach().clone()) for q in qs]
    opt_b = EMAOptimizer(_adam(rs), 0.5)  # (decay and period come from the state_dict)
    opt_b.load_state_dict(sd)
    assert opt_b.decay == 0.8 and opt_b.every_n_steps == 3 and opt_b.current_step == 4
    for step in range(4, 8):
        _grads(rs, step)
        opt_b.step()
    for p, r in zip(ps, rs):
        assert torch.equal(p, r)
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.optimizer.state[p][key], opt_b.optimizer.state[r][key])
    assert all(torch.equal(a, b) for a, b in zip(opt.ema_params, opt_b.ema_params))


def test_swap_exchanges_and_restores_bit_for_bit():
    ps = _params()
    opt = EMAOptimizer(_adam(ps), 0.7)
    for step in range(3):
        _grads(ps, step)
        opt.step()
    w = [p.detach().clone() for p in ps]
    e = [x.clone() for x in opt.ema_params]
    assert not any(torch.equal(a, b) for a, b in zip(w, e))
    with opt.swap_ema_weights():
        assert all(torch.equal(p, b) for p, b in zip(ps, e))
        assert all(torch.equal(x, a) for x, a in zip(opt.ema_params, w))
    assert all(torch.equal(p, a) for p, a in zip(ps, w)) and all(torch.equal(x, b) for x, b in zip(opt.ema_params, e))
    with pytest.raises(RuntimeError, match="inside"):
        with opt.swap_ema_weights():
            raise RuntimeError("inside")
    assert all(torch.equal(p, a) for p, a in zip(ps, w)) and all(torch.equal(x, b) for x, b in zip(opt.ema_params, e))
    with opt.swap_ema_weights(enabled=False):
        assert all(torch.equal(p, a) for p, a in zip(ps, w))


@pytest.mark.parametrize("decay", [-0.1, 1.5, float("nan"), "0.9", None])
def test_bad_decay_raises(decay):
    with pytest.raises(ValueError):
        EMAOptimizer(_adam(_params()), decay)


@pytest.mark.parametrize("every", [0, -2, 1.5, None])
def test_bad_every_n_steps_raises(every):
    with pytest.raises(ValueError):
        EMAOptimizer(_adam(_params()), 0.9, every_n_steps=every)


def test_the_lr_scheduler_stays_on_the_inner_optimizer():
    from arreau_amd.checkpoint import make_synthetic_model
    from arreau_amd.train import configure_training
    m = make_synthetic_model(S=12, num_timesteps=100)
    opt, sched = configure_training(m, 5, ema_decay=0.9, ema_every_n_steps=2)
    assert isinstance(opt, EMAOptimizer) and opt.every_n_steps == 2 and sched.optimizer is opt.optimizer
    assert opt.param_groups is opt.optimizer.param_groups  # (delegated, as the reference's __getattr__ does)
    plain, _ = configure_training(m, 5)
    assert not isinstance(plain, EMAOptimizer)


def test_ema_checkpoint_pair(tmp_path):
    """X.ckpt -> X-EMA.ckpt (the reference callback's naming); the twin loads through load_from_checkpoint, its parameters are the
    average, everything else (buffers, orientation grid, hyper-parameters) the module's."""
    from arreau_amd.checkpoint import ema_checkpoint_path, load_lightning_checkpoint, make_synthetic_model, save_ema_checkpoint
    from arreau_amd.lightning_wrappers.diffusion import ORI_GRID_KEY, PONITA_DIFFUSION
    assert ema_checkpoint_path("out/model.ckpt") == "out/model-EMA.ckpt"
    assert ema_checkpoint_path("/a/b.c/last.ckpt") == "/a/b.c/last-EMA.ckpt"
    m = make_synthetic_model(S=12, num_timesteps=100)
    with torch.no_grad():
        m.model.interaction_layers[0].conv.callibrated.fill_(True)
    opt = EMAOptimizer(m.configure_optimizers(max_epochs=3)["optimizer"], 0.5, module=m)
    for step in range(2):
        g = torch.Generator().manual_seed(step)
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g) * 0.1
        opt.step()
    path = save_ema_checkpoint(str(tmp_path / "trained.ckpt"), m, opt)
    assert path == str(tmp_path / "trained-EMA.ckpt")
    ema = {id(p): e for p, e in zip(opt.all_parameters(), opt.ema_params)}
    names = dict(m.named_parameters())
    ck = load_lightning_checkpoint(path)
    sd = m.state_dict()
    assert set(ck["state_dict"]) == set(sd) | {ORI_GRID_KEY}
    differs = 0
    for k, v in sd.items():
        want = ema[id(names[k])] if k in names else v
        assert torch.equal(ck["state_dict"][k], want), k
        differs += k in names and not torch.equal(want, v)
    assert differs > 0
    assert torch.equal(ck["state_dict"][ORI_GRID_KEY], m.model.ori_grid)
    assert ck["hyper_parameters"]["args"] == m.hparams.args
    loaded = PONITA_DIFFUSION.load_from_checkpoint(path, map_location="cpu").cpu()
    for k, v in loaded.state_dict().items():
        want = ema[id(names[k])] if k in names else sd[k]
        assert torch.equal(v, want), k
    assert bool(loaded.model.interaction_layers[0].conv.callibrated)
    assert torch.equal(loaded.model.ori_grid, m.model.ori_grid)


def test_a_frozen_parameter_keeps_its_first_copy():
    """A parameter with requires_grad False (the module's Fourier projection) is never changed by the optimizer: its average stays
    the exact copy taken at the first step instead of going through the rounding of the recurrence."""
    ps = _params()
    ps[2].requires_grad_(False)
    init = ps[2].detach().clone()
    opt = EMAOptimizer(_adam(ps), 0.9)
    for step in range(5):
        _grads(ps, step)
        ps[2].grad = None
        opt.step()
    assert torch.equal(opt.ema_params[2], init) and torch.equal(ps[2], init)
    assert not torch.equal(opt.ema_params[0], ps[0])
