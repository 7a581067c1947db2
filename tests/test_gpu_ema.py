"""The exponential moving average of the weights on the MI355X (arreau_amd.optim.EMAOptimizer): the fused update inside the Adam launch
(arreau_optimizer_step_ema) against a float64 restatement of the recurrence and against the _foreach fallback, its exact ends, the
calibrated first values, a swap that keeps the HIP engine coherent, and the training driver end to end.  Run with `-m gpu`."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(37, 29), (1024,), (5,), (3, 700), (1,), (2049,)]   # straddle the kernel's 1,024-element chunks
DECAYED = [True, False, False, True, False, True]


def _ulp(x):
    return float(np.spacing(np.float32(x)))


@pytest.fixture(scope="module")
def setup():
    from arreau_amd.checkpoint import make_synthetic_model
    from oracle import geometry as OG
    dev = torch.device("cuda", 0)
    m = make_synthetic_model(S=12, seed=1234, num_timesteps=100).to(dev)
    rng = np.random.RandomState(8)
    num_atoms = [3, 5, 2, 1, 6]
    B, N, S = len(num_atoms), sum(num_atoms), 12
    lengths = torch.tensor(rng.uniform(3.5, 7.0, size=(B, 3)), dtype=torch.float32)
    angles = torch.tensor(np.deg2rad(rng.uniform(75, 105, size=(B, 3))), dtype=torch.float32)
    lattice0 = OG.lattice_from_params(lengths, angles)
    frac0 = torch.tensor(rng.uniform(0, 1, size=(N, 3)), dtype=torch.float32)
    types0 = torch.tensor(rng.randint(0, S - 1, size=N))
    timestep = torch.tensor([1, 50, 100, 2, 77])
    g = torch.Generator().manual_seed(4)
    noise = (torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g), torch.randn(B, 3, generator=g))
    batch = SimpleNamespace(X0=frac0, A0=types0, L0=lattice0.reshape(-1, 3), num_atoms=torch.tensor(num_atoms))
    return m, batch, timestep, noise


def _flat_run(decay, every, ema=True, steps=10):
    """ClipAdam over two groups on flat-buffer gradient views (as HipEngine.train_backward lays them out), optionally wrapped in an
    EMAOptimizer, stepped through step_flat with a changing learning rate, clipped and unclipped steps and one non-finite gradient.
    Returns per-step records (parameters after the step, moments, norm, the EMA)."""
    from arreau_amd.optim import ClipAdam, EMAOptimizer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in SHAPES]
    init = [p.detach().clone() for p in ps]
    inner = ClipAdam([{"params": [p for p, d in zip(ps, DECAYED) if d], "weight_decay": 1e-2},
                      {"params": [p for p, d in zip(ps, DECAYED) if not d], "weight_decay": 0.0}], lr=3e-3)
    opt = EMAOptimizer(inner, decay, every_n_steps=every) if ema else inner
    order = [p for grp in inner.param_groups for p in grp["params"]]
    sizes = [-(-p.numel() // 4) * 4 for p in ps]
    records = []
    for step in range(steps):
        flat = torch.zeros(sum(sizes) + 8, device=dev)
        off = 0
        for p, n in zip(ps, sizes):
            grad = torch.randn(p.shape, generator=g) * (10.0 if step % 2 else 0.01)
            if step == 3:
                grad.view(-1)[0] = float("inf")
            p.grad = flat[off:off + p.numel()].view(p.shape)
            p.grad.copy_(grad)
            off += n
        for grp in inner.param_groups:
            grp["lr"] = 3e-3 * (1 + step)
        ema_before = [e.clone() for e in opt.ema_params] if ema and step else None
        norm = opt.step_flat(flat, 0.5)
        assert norm is not None
        rec = {"p": [p.detach().clone() for p in order], "norm": norm.clone(), "ema_before": ema_before,
               "m": [inner.state[p]["exp_avg"].clone() for p in order], "v": [inner.state[p]["exp_avg_sq"].clone() for p in order]}
        if ema:
            rec["ema"] = [e.clone() for e in opt.ema_params]
            assert opt.current_step == step + 1
            assert all(e.data_ptr() >= opt._ema_flat.data_ptr() for e in opt.ema_params)  # the fused path's buffer
        records.append(rec)
    ids = [id(p) for p in ps]
    return [init[ids.index(id(p))] for p in order], records, opt


@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("every", [1, 3])
def test_fused_ema_against_float64_and_adam_bits(decay, every):
    """The average from arreau_optimizer_step_ema against e <- d e + (1 - d) p in float64, fed the actual per-step parameters.  Per
    update the fp32 form rounds e*d, rounds the fused add and carries d and 1 - d rounded to fp32: each below half an ulp of
    M = max |p|, |e| (the last two as |e| 2^-25 and |p| (1 - d) 2^-25), so under 2 ulp(M) per update; an earlier error only shrinks
    (times d), so after n updates the bound is 2 n ulp(M).  Parameters, moments and the norm are ClipAdam's without the average, bit
    for bit; at a step without an update the average does not move by a bit."""
    init, recs, _ = _flat_run(decay, every)
    _, plain, _ = _flat_run(decay, every, ema=False)
    for a, b in zip(recs, plain):
        assert torch.equal(a["norm"], b["norm"]) or (not torch.isfinite(a["norm"]) and not torch.isfinite(b["norm"]))
        for key in ("p", "m", "v"):
            assert all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    ema64 = [t.double() for t in init]
    M = max(float(t.abs().max()) for t in init)
    n_upd, worst = 0, 0.0
    for step, rec in enumerate(recs):
        M = max(M, max(float(t.abs().max()) for t in rec["p"]))
        if step % every == 0:
            ema64 = [decay * e + (1.0 - decay) * p.double() for e, p in zip(ema64, rec["p"])]
            n_upd += 1
        else:
            assert all(torch.equal(x, y) for x, y in zip(rec["ema"], rec["ema_before"])), step
        err = max(float((e.double() - r).abs().max()) for e, r in zip(rec["ema"], ema64))
        worst = max(worst, err / _ulp(M))
        assert err <= 2 * n_upd * _ulp(M), (step, err, _ulp(M))
    print(f"\n[fused EMA, decay {decay}, every {every}] worst deviation from float64 {worst:.2f} ulp(max|p|) after {n_upd} updates")


def test_fused_ema_exact_ends():
    """decay 0: the average is the parameters, bit for bit, after every update; decay 1: it stays the values before the first step."""
    _, recs, _ = _flat_run(0.0, 1)
    for rec in recs:
        assert all(torch.equal(e, p) for e, p in zip(rec["ema"], rec["p"]))
    init, recs, _ = _flat_run(1.0, 1)
    for rec in recs:
        assert all(torch.equal(e, i) for e, i in zip(rec["ema"], init))
    assert not torch.equal(recs[-1]["p"][0], init[0])


def _train(m, batch, timestep, noise, steps, decay=0.9, snap=False):
    from arreau_amd.train import configure_training, optimizer_step
    opt, _ = configure_training(m, 10, ema_decay=decay)
    for grp in opt.param_groups:
        grp["lr"] = 1e-3
    losses, snaps = [], []
    for _ in range(steps):
        losses.append(m.training_step(batch, timestep=timestep, noise=noise).detach().clone())
        if snap:
            snaps.append([p.detach().clone() for p in opt.all_parameters()])
        optimizer_step(m, opt, world_size=1)
    return opt, losses, snaps


def test_fused_ema_against_the_foreach_fallback(setup, monkeypatch):
    """The model trained through arreau_amd.train.optimizer_step on ClipAdam (fused update) and on torch's fused Adam
    (ARREAU_TORCH_ADAM=1: step_flat declines, step() runs the _foreach pair).  Each average is a convex combination of its run's
    parameter snapshots, so the two agree within both recurrences' bound (2 n ulp(M) each) plus the largest difference of the two
    runs' parameters at any step."""
    from arreau_amd.optim import ClipAdam
    m, batch, timestep, noise = setup
    steps = 4
    ma = copy.deepcopy(m)
    opt_a, _, snaps_a = _train(ma, batch, timestep, noise, steps, snap=True)
    assert isinstance(opt_a.optimizer, ClipAdam) and opt_a._ema_flat is not None
    monkeypatch.setenv("ARREAU_TORCH_ADAM", "1")
    mb = copy.deepcopy(m)
    opt_b, _, snaps_b = _train(mb, batch, timestep, noise, steps, snap=True)
    assert not isinstance(opt_b.optimizer, ClipAdam) and opt_b._ema_flat is None
    pa, pb = list(opt_a.all_parameters()), list(opt_b.all_parameters())
    M = max(float(t.abs().max()) for t in pa + pb + list(opt_a.ema_params) + [x for s in snaps_a for x in s] if t.numel())
    for i, (ea, eb) in enumerate(zip(opt_a.ema_params, opt_b.ema_params)):
        if ea.numel() == 0:  # (the zero-element edge read-outs of this configuration)
            continue
        drift = max(float((s_a[i] - s_b[i]).abs().max()) for s_a, s_b in zip(snaps_a[1:] + [pa], snaps_b[1:] + [pb]))
        err = float((ea - eb).abs().max())
        assert err <= 4 * steps * _ulp(M) + drift, (i, err, drift)
    assert opt_a.current_step == opt_b.current_step == steps


def test_ema_starts_from_the_calibrated_weights(setup):
    """Decay 1: the average is the parameters as they stand between the first training_step (which applies the conv calibration,
    FiberBundleConv.callibrate) and its optimizer step, bit for bit."""
    m, batch, timestep, noise = setup
    mm = copy.deepcopy(m)
    assert not bool(mm.model.interaction_layers[0].conv.callibrated)
    kernel = mm.model.interaction_layers[0].conv.kernel.weight
    before = kernel.detach().clone()
    opt, _, snaps = _train(mm, batch, timestep, noise, 3, decay=1.0, snap=True)
    assert opt._ema_flat is not None
    assert all(torch.equal(e, s) for e, s in zip(opt.ema_params, snaps[0]))
    i = [id(p) for p in opt.all_parameters()].index(id(kernel))
    assert not torch.equal(opt.ema_params[i], before)  # the calibrated values, not the initial ones
    assert not torch.equal(opt.ema_params[i], kernel)  # (and the optimizer has moved on since)


def _seed_initial_state():
    # the sampler draws its initial state from torch's CPU generator and the cell angles from numpy's; the steps' noise from `seed`
    torch.manual_seed(5)
    np.random.seed(5)


def test_swap_keeps_the_engine_coherent(setup, tmp_path):
    """Run A trains three steps with an average, then inside swap_ema_weights() runs validation_step and a short sample -- the bits
    of a fresh model loaded from the `-EMA` checkpoint --, then two more steps.  Run B trains five steps with nothing in between.
    Losses, every parameter and the average agree bit for bit: the training engine (its own weight copies) was set aside during
    the swap, not repacked from the averaged values."""
    from arreau_amd.checkpoint import save_ema_checkpoint
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    from arreau_amd.train import optimizer_step
    m, batch, timestep, noise = setup
    ma, mb = copy.deepcopy(m), copy.deepcopy(m)
    opt_a, losses_a, _ = _train(ma, batch, timestep, noise, 3)
    path = save_ema_checkpoint(str(tmp_path / "a.ckpt"), ma, opt_a)
    kw = dict(num_atoms_per_sample=4, num_samples_in_batch=2, num_steps=5, seed=1234)
    train_eng = ma._engine
    with opt_a.swap_ema_weights():
        val_a = ma.validation_step(batch, timestep=timestep, noise=noise).clone()
        _seed_initial_state()
        smp_a = ma.sample(**kw)
    assert ma._engine is train_eng
    fresh = PONITA_DIFFUSION.load_from_checkpoint(path)
    val_f = fresh.validation_step(batch, timestep=timestep, noise=noise)
    _seed_initial_state()
    smp_f = fresh.sample(**kw)
    assert torch.equal(val_a, val_f)
    for key in ("frac_x", "atomic_numbers", "lattice", "num_atoms"):
        assert np.array_equal(getattr(smp_a, key), getattr(smp_f, key)), key
    for _ in range(2):
        losses_a.append(ma.training_step(batch, timestep=timestep, noise=noise).detach().clone())
        optimizer_step(ma, opt_a, world_size=1)
    opt_b, losses_b, _ = _train(mb, batch, timestep, noise, 5)
    assert all(torch.equal(a, b) for a, b in zip(losses_a, losses_b))
    assert all(torch.equal(p, q) for p, q in zip(ma.parameters(), mb.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(opt_a.ema_params, opt_b.ema_params))
    # and the average really differs from the trained weights (the swap was not a no-op)
    assert not all(torch.equal(p, e) for p, e in zip(opt_a.all_parameters(), opt_a.ema_params))


def test_two_rank_training_with_ema_writes_the_ema_checkpoint(tmp_path):
    """arreau_amd.train with --ema_decay on two data-parallel ranks (gloo, sharing this box's GPU): both checksum lines agree across
    the replicas, X-EMA.ckpt is written next to X.ckpt with other weights, and it loads and samples."""
    import os
    import socket
    import subprocess
    import sys
    from arreau_amd.checkpoint import load_lightning_checkpoint
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(ARREAU_TRAIN_BACKEND="gloo", ARREAU_TRAIN_ONE_DEVICE="1", PYTHONPATH=root)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "trained.ckpt")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "-m", "arreau_amd.train", "--num_synthetic", "66", "--epochs",
                        "3", "--warmup", "1", "--batch_size", "8", "--lr", "2e-3", "--ema_decay", "0.9", "--out", out], env=env,
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    for what in ("parameter", "EMA"):
        sums = [ln for ln in p.stdout.splitlines() if ln.startswith(f"replica {what} checksums:")]
        assert len(sums) == 1, p.stdout
        a, b = (float(v) for v in sums[0].split(":")[1].split())
        assert a == b, sums
    ema_path = str(tmp_path / "trained-EMA.ckpt")
    assert os.path.exists(out) and os.path.exists(ema_path)
    main, ema = load_lightning_checkpoint(out)["state_dict"], load_lightning_checkpoint(ema_path)["state_dict"]
    assert set(main) == set(ema)
    assert not torch.equal(main["model.interaction_layers.0.linear_1.weight"], ema["model.interaction_layers.0.linear_1.weight"])
    assert torch.equal(main["model.interaction_layers.0.conv.callibrated"], ema["model.interaction_layers.0.conv.callibrated"])
    m = PONITA_DIFFUSION.load_from_checkpoint(ema_path)
    res = m.sample(num_atoms_per_sample=4, num_samples_in_batch=2, num_steps=5, seed=3)
    assert np.isfinite(res.frac_x).all() and np.isfinite(res.lattice).all()
