"""Training runs on the device: the keyed forward noising (arreau_diffusion_noise_keyed), per-crystal loss rows
(arreau_diffusion_loss_rows), their binned reduction (arreau_loss_rows_reduce), PONITA_DIFFUSION.evaluate, exact resume and the
command line.  Crystals of 1, 2, 64, 65, 256, 257 and 300 atoms in one batch, S = 90 and S = 124, T = 10.  Needs an MI355X."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import training_run_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 10
U = 2.0 ** -24  # unit roundoff of float32


@pytest.fixture(scope="module", params=[90, 124])
def setup(request):
    """a synthetic model of S species at T = 10, its engine and the hand-built crystals"""
    from arreau_amd.checkpoint import make_synthetic_model
    from arreau_amd.diffusion.diffusion_helpers import crystal_offsets
    S = request.param
    dev = torch.device("cuda", 0)
    m = make_synthetic_model(S=S, seed=1234, num_timesteps=T, pooled_readout_scale=1 / 32).to(dev)
    eng = m.engine()
    items = C.crystals(S)
    return SimpleNamespace(m=m, eng=eng, S=S, dev=dev, items=items, offsets=crystal_offsets)


def _device_batch(su, order=None, copy=None):
    b = C.batch_of(su.items, C.IDS, order)
    f32 = dict(device=su.dev, dtype=torch.float32)
    d = SimpleNamespace(host=b, frac=torch.tensor(b.X0, **f32), types=torch.tensor(b.A0, device=su.dev, dtype=torch.int32),
                        cell=torch.tensor(b.L0, **f32).reshape(-1, 3, 3), off=su.offsets(torch.tensor(b.num_atoms), su.dev),
                        ids=torch.tensor(b.index, device=su.dev))
    d.copy = None if copy is None else torch.tensor(copy, device=su.dev, dtype=torch.int32)
    return d


def _keyed(su, d, copies=1):
    return su.eng.diffusion_noise_keyed(d.frac, d.types, d.cell, d.off, C.NOISE_SEED, d.ids, copies, d.copy)


NOISED = ("noisy_frac", "target_eps", "noisy_types", "noisy_lengths", "lengths", "angles", "t")


def _draw_arrays(su, d, t):
    """the draws of the batch as arrays, from arreau_philox_fill_keyed per crystal"""
    zf, ut, zl = [], [], []
    for n, cid, tb in zip(d.host.num_atoms, d.host.index, t):
        zf.append(su.eng.philox_fill_keyed(C.NOISE_SEED, tb, C.KIND_Z_FRAC, cid, 3 * int(n)).reshape(-1, 3))
        ut.append(su.eng.philox_fill_keyed(C.NOISE_SEED, tb, C.KIND_U_TYPES, cid, int(n) * su.S).reshape(-1, su.S))
        zl.append(su.eng.philox_fill_keyed(C.NOISE_SEED, tb, C.KIND_Z_LENGTHS, cid, 3).reshape(1, 3))
    return torch.cat(zf).contiguous(), torch.cat(ut).contiguous(), torch.cat(zl).contiguous()


# ------------------------------------------------------------------------------------------------------------------------ 6
def test_keyed_noise_is_the_array_path_fed_the_same_draws_bitwise(setup):
    su = setup
    d = _device_batch(su)
    got = _keyed(su, d)
    t = [int(v) for v in got["t"].cpu()]
    # the timestep rule restated: kind 9 at counter timestep 0, word3 = id; both ends of 1..T occur in this batch
    for cid, tb in zip(d.host.index, t):
        _, raw = su.eng.philox_fill_keyed(C.NOISE_SEED, 0, C.KIND_T, cid, 1, raw=True)
        w0 = int(raw[0, 0].cpu()) & 0xFFFFFFFF
        assert w0 == int(C.words(C.NOISE_SEED, 0, 0, C.KIND_T, int(cid))[0])
        assert tb == C.keyed_timestep(w0 >> 8, 0, 1, T)
    assert min(t) == 1 and max(t) == T, t
    z_frac, u_types, z_len = _draw_arrays(su, d, t)
    want = su.eng.diffusion_noise(d.frac, d.types, d.cell, got["t"], d.off, z_frac, u_types, z_len)
    for k in NOISED[:-1]:
        assert torch.equal(got[k], want[k]), k
    su.eng.check_status()
    # a caller's own timesteps: kind 9 is not drawn, the rest is keyed by them
    mine = torch.tensor([T, 1, 3, 3, 7, 2, 9], device=su.dev, dtype=torch.int32)
    own = su.eng.diffusion_noise_keyed(d.frac, d.types, d.cell, d.off, C.NOISE_SEED, d.ids, 1, None, t_crystal=mine.clone())
    assert torch.equal(own["t"], mine)
    z_frac, u_types, z_len = _draw_arrays(su, d, mine.tolist())
    want = su.eng.diffusion_noise(d.frac, d.types, d.cell, mine, d.off, z_frac, u_types, z_len)
    for k in NOISED[:-1]:
        assert torch.equal(own[k], want[k]), k


# ------------------------------------------------------------------------------------------------------------------------ 7
def _per_crystal(d, out):
    """{crystal id: its slices of the noised state}"""
    first = np.concatenate([[0], np.cumsum(d.host.num_atoms)])
    res = {}
    for b, cid in enumerate(d.host.index):
        a, e = int(first[b]), int(first[b + 1])
        res[int(cid)] = {k: (out[k][a:e] if k in ("noisy_frac", "target_eps", "noisy_types") else out[k][b]).cpu() for k in NOISED}
    return res


def test_keyed_noise_of_a_crystal_does_not_depend_on_the_batch(setup):
    su = setup
    B = len(C.SIZES)
    noised = lambda order: (lambda d: _per_crystal(d, _keyed(su, d)))(_device_batch(su, order=order))
    full, rev = noised(None), noised(range(B - 1, -1, -1))
    for b in range(B):
        alone = noised([b])
        cid = C.IDS[b]
        for k in NOISED:
            assert torch.equal(alone[cid][k], full[cid][k]), (cid, k)
            assert torch.equal(rev[cid][k], full[cid][k]), (cid, k)
    # two copies of one crystal (R = 2): different timesteps, each in its stratum, and different draws
    d = _device_batch(su, order=[3, 3], copy=[0, 1])
    two = _keyed(su, d, copies=2)
    t0, t1 = (int(v) for v in two["t"].cpu())
    assert C.stratum(0, 2, T)[0] <= t0 <= C.stratum(0, 2, T)[1] < C.stratum(1, 2, T)[0] <= t1 <= C.stratum(1, 2, T)[1]
    assert (t0, t1) == (C.keyed_t(C.NOISE_SEED, C.IDS[3], 0, 2, T), C.keyed_t(C.NOISE_SEED, C.IDS[3], 1, 2, T))
    n = C.SIZES[3]
    assert not torch.equal(two["noisy_frac"][:n], two["noisy_frac"][n:])
    assert not torch.equal(two["noisy_lengths"][0], two["noisy_lengths"][1])
    # the same row again in another batch: a function of (seed, id, copy, R)
    again = _keyed(su, _device_batch(su, order=[0, 3], copy=[0, 1]), copies=2)
    assert torch.equal(again["noisy_frac"][1:], two["noisy_frac"][n:]) and int(again["t"][1]) == t1
    su.eng.check_status()
    from arreau_amd import _hip
    with pytest.raises(_hip.ArreauHipError):  # R > T
        _keyed(su, _device_batch(su), copies=T + 1)


# ------------------------------------------------------------------------------------------------------------------------ 8
def test_keyed_noise_matches_the_float64_oracle_fed_the_restated_draws(setup):
    from oracle import training as TR
    from tests.helpers import oracle_from_module
    su = setup
    om = oracle_from_module(su.m, torch.float64)
    d = _device_batch(su)
    got = _keyed(su, d)
    t = [C.keyed_t(C.NOISE_SEED, cid, 0, 1, T) for cid in C.IDS]
    assert t == [int(v) for v in got["t"].cpu()]
    draws = [C.keyed_draws(C.NOISE_SEED, cid, tb, n, su.S) for cid, tb, n in zip(C.IDS, t, C.SIZES)]
    z_frac, u_types, z_len = (np.concatenate([np.atleast_2d(dr[j]) for dr in draws]) for j in range(3))
    # the inputs leave no species to chance: every atom's winning Gumbel score leads the runner-up's by more than 1e-5 in float64
    q = om.q_mats.double().numpy()
    margins = [C.gumbel_margin(q[tb - 1, int(x0)], u) for tb, n, a0, us in zip(t, C.SIZES, (it.A0 for it in su.items),
                                                                              (dr[1] for dr in draws)) for x0, u in zip(a0, us)]
    assert min(margins) > 1e-5, min(margins)
    b = d.host
    f64 = lambda a: torch.tensor(a, dtype=torch.float64)
    want = TR.noise_inputs(om, f64(b.X0.astype(np.float32)), torch.tensor(b.A0), f64(b.L0.astype(np.float32)).reshape(-1, 3, 3),
                           torch.tensor(b.num_atoms), torch.tensor(t), f64(z_frac), f64(u_types), f64(z_len))
    # (the tolerances of test_forward_noising_matches_oracle)
    np.testing.assert_allclose(got["noisy_frac"].cpu().numpy(), want["noisy_frac"].numpy(), atol=1e-6, rtol=0)
    dd = (got["target_eps"].cpu().double() - want["target_eps"]).abs()
    assert torch.minimum(dd, 1 - dd).max() <= 1e-5
    assert torch.equal(got["noisy_types"].cpu().long(), want["noisy_types"])
    np.testing.assert_allclose(got["noisy_lengths"].cpu().numpy(), want["noisy_lengths"].numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(got["lengths"].cpu().numpy(), want["lengths"].numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(got["angles"].cpu().numpy(), want["angles"].numpy(), atol=2e-6, rtol=0)


# ------------------------------------------------------------------------------------------------------------------- 9, 10
@pytest.fixture(scope="module")
def rows_case(setup):
    """One evaluation of the batch and both loss entry points on it; the row table has 3 rows per crystal, every third written."""
    su = setup
    d = _device_batch(su)
    nz = _keyed(su, d)
    eps, logits, len0 = su.eng.predict_scores(nz["noisy_frac"], nz["noisy_types"], nz["noisy_lengths"], nz["angles"], nz["t"], d.off)
    args = (eps, nz["target_eps"], logits, d.types, nz["noisy_types"], nz["t"], len0, nz["lengths"], d.off)
    B = len(C.SIZES)
    table = su.eng.loss_row_table(3 * B)
    index = torch.tensor([3 * b + 1 for b in range(B)], device=su.dev)
    losses, grads, terms = su.eng.diffusion_loss_rows(*args, index, table, with_grads=True)
    plain, plain_grads = su.eng.diffusion_losses(*args, with_grads=True)
    su.eng.check_status()
    return SimpleNamespace(su=su, d=d, nz=nz, len0=len0, table=table, losses=losses, grads=grads, terms=terms, plain=plain,
                           plain_grads=plain_grads, args=args)


def test_loss_rows_against_float64_sums_of_the_kernels_own_terms(rows_case):
    rc = rows_case
    B = len(C.SIZES)
    # everything arreau_diffusion_losses writes, bitwise
    assert torch.equal(rc.losses, rc.plain)
    for a, b in zip(rc.grads, rc.plain_grads):
        assert torch.equal(a, b)
    sums, n_atoms, t = (v.cpu().numpy() for v in rc.su.eng.rows_to_fields(rc.table))
    written = np.arange(B) * 3 + 1
    assert (n_atoms[written] == np.array(C.SIZES)).all() and (t[written] == rc.nz["t"].cpu().numpy()).all()
    mask = np.ones(3 * B, bool)
    mask[written] = False
    assert (n_atoms[mask] == 0).all() and (sums[mask] == 0).all()  # the rest of the table is untouched
    terms = rc.terms.cpu().numpy()
    first = np.concatenate([[0], np.cumsum(C.SIZES)])
    # the length errors as the kernel forms them: float32 d = pred - length / n, e = d * d rounded once
    n32 = np.array(C.SIZES, dtype=np.float32)[:, None]
    dl = rc.len0.cpu().numpy() - rc.nz["lengths"].cpu().numpy() / n32
    e = (dl * dl).astype(np.float32)
    assert dl.dtype == np.float32
    for b, n in enumerate(C.SIZES):
        x = terms[first[b]:first[b + 1]].astype(np.float64)
        row = sums[written[b]].astype(np.float64)
        # any-order float32 summation of n terms: at most n - 1 roundings, each at most u times a partial sum <= sum |term|
        for j in range(3):
            bound = (n - 1) * U * np.abs(x[:, j]).sum()
            print(f"S={rc.su.S} crystal of {n}: term {j} row {row[j]:.9e} float64 {x[:, j].sum():.9e} bound {bound:.2e}")
            assert abs(row[j] - x[:, j].sum()) <= bound, (n, j)
        el = e[b].astype(np.float64)
        assert abs(row[3] - el.sum()) <= 2 * U * np.abs(el).sum(), n
    # the batch loss recombined from the rows against losses[0..5]: both are float32 sums of the same N (3 B) terms in different
    # orders, each within (N - 1) u sum|term| of the exact sum; the means and the final additions add a few roundings of the result
    N = int(first[-1])
    rs = sums[written].astype(np.float64).sum(0)
    got = rc.losses.cpu().numpy().astype(np.float64)
    absum = np.abs(terms.astype(np.float64)).sum(0)
    ef, vb, ce, el = rs[0] / N, rs[1] / N, rs[2] / N, rs[3] / (3 * B)
    b_ef, b_vb, b_ce = (2 * (N - 1) * U * absum[j] / N + 2 * U * abs(v) for j, v in enumerate((ef, vb, ce)))
    b_el = 2 * (3 * B - 1) * U * np.abs(e.astype(np.float64)).sum() / (3 * B) + 2 * U * abs(el)
    et, b_et = 0.001 * vb + ce, 0.001 * b_vb + b_ce + 3 * U * abs(0.001 * vb + ce)
    for name, g, w, bound in (("error_frac_x", got[1], ef, b_ef), ("error_atomic_type", got[2], et, b_et), ("error_lattice", got[3], el, b_el),
                              ("vb", got[4], vb, b_vb), ("ce", got[5], ce, b_ce),
                              ("loss", got[0], ef + et + el, b_ef + b_et + b_el + 3 * U * abs(ef + et + el))):
        print(f"S={rc.su.S} {name}: losses {g:.9e} rows {w:.9e} bound {bound:.2e}")
        assert abs(g - w) <= bound, name


def test_binned_reduction_of_the_rows(rows_case):
    rc = rows_case
    eng = rc.su.eng
    B = len(C.SIZES)
    sums, n_atoms, t = (v.cpu().numpy() for v in eng.rows_to_fields(rc.table))
    for n_bins in (4, 10):
        got_s, got_c, got_u = eng.loss_rows_reduce(rc.table, n_bins, T)
        want_s, want_c, want_u = C.reduce_rows(sums, n_atoms, t, n_bins, T)
        np.testing.assert_allclose(got_s.cpu().numpy(), want_s, rtol=1e-12, atol=0)  # n 2^-53 with room
        assert (got_c.cpu().numpy() == want_c).all()
        assert int(got_u) == want_u == 2 * B  # the unwritten rows are counted
        again = eng.loss_rows_reduce(rc.table, n_bins, T)
        assert all(torch.equal(a, b) for a, b in zip((got_s, got_c, got_u), again))
        assert int(got_c[n_bins, 1]) == B and int(got_c[n_bins, 0]) == sum(C.SIZES)
    # the total record is the reference's batch loss of the batch
    total = C.set_loss(got_s[-1].cpu().numpy(), got_c[-1].cpu().numpy())
    assert abs(total - float(rc.losses[0])) <= 1e-5 * abs(total)


# ----------------------------------------------------------------------------------------------------------------------- 11
class _ListDataset:
    """the hand-built crystals as a dataset (the fields of CrystalDataset.__getitem__)"""

    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        it = self.items[i]
        f64 = lambda a: torch.tensor(a, dtype=torch.float64)
        return SimpleNamespace(pos=f64(it.X0 @ it.L0), X0=f64(it.X0), A0=torch.tensor(it.A0), L0=f64(it.L0), num_atoms=it.num_atoms)


def _components(r):
    return np.array([r[k] for k in ("loss", "error_frac_x", "error_atomic_type", "error_lattice", "vb", "ce")])


def test_evaluate_is_the_loss_of_the_set_as_one_batch(setup):
    from arreau_amd.diffusion.lattice_dataset import collate
    su = setup
    m, ds, R, seed = su.m, _ListDataset(su.items), 3, 41
    n = len(ds)
    a = m.evaluate(ds, 2, seed, copies=R, n_bins=5)   # 21 pairs in batches of 2: a ragged last batch
    b = m.evaluate(ds, 2, seed, copies=R, n_bins=5)
    assert a == b                                      # twice with one batch size: the same bits, bins included
    assert a["num_crystals"] == n * R and a["num_atoms"] == R * sum(C.SIZES) and len(a["bins"]) == 5
    assert sum(r["num_crystals"] for r in a["bins"]) == n * R
    c = m.evaluate(ds, 7, seed, copies=R, n_bins=5)
    print("evaluate, batches of 2 and of 7:", a["loss"], c["loss"])
    # (another batch size may give the network another launch plan: the project's parity tolerance)
    np.testing.assert_allclose(_components(c), _components(a), rtol=1e-5, atol=0)
    # the whole set as ONE batch through validation_step, fed the same keyed noise
    k = np.arange(n * R)
    idx, cp = k // R, k % R
    whole = collate([ds[int(i)] for i in idx], index=idx)
    s = m.evaluate(ds, 4, seed, copies=R, kernels="sampling")
    one = float(m.validation_step(whole, noise="philox", seed=seed, copies=R, copy=cp))
    print("evaluate on the sampling kernels:", s["loss"], "validation_step on the whole set:", one)
    assert abs(s["loss"] - one) <= 1e-5 * abs(one)
    # training forward against sampling kernels: their outputs agree to TOL * max(1, max |output|) each
    # (test_training_forward_matches_sampling_kernels); to first order the loss then moves by at most sum |d loss / d output| * that
    _, parts = m.diffusion_loss(m, whole, None, noise="philox", seed=seed, copies=R, copy=cp, return_parts=True)
    TOL = 1e-5
    bound = sum(float(parts[g].abs().sum()) * TOL * max(1.0, float(parts[o].abs().max()))
                for g, o in (("grad_eps", "pred_eps"), ("grad_logits", "logits"), ("grad_lengths", "pred_lengths")))
    print("training forward:", a["loss"], "sampling kernels:", s["loss"], "first-order bound", bound)
    assert abs(a["loss"] - s["loss"]) <= 2 * bound + 1e-5 * abs(s["loss"])  # (twice first order, plus the sums' own tolerance)
    with pytest.raises(ValueError):
        m.evaluate(ds, 4, seed, copies=T + 1)


# ----------------------------------------------------------------------------------------------------------------------- 12
class _Stop(Exception):
    pass


def _fresh_run(ds, seed, epochs=3):
    from arreau_amd.checkpoint import default_args
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    from arreau_amd.train import configure_training
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    m = PONITA_DIFFUSION(default_args(lr=1e-3, epochs=epochs, warmup=1, num_timesteps=T), ds.z_table).to("cuda:0")
    torch.random.set_rng_state(state)
    opt, sched = configure_training(m, epochs, ema_decay=0.99)
    return m, opt, sched


CHECKPOINTS = ((0, 0), (1, 2))  # (epoch, batches done; 0: the epoch's end): after epoch 1, and after step 2 of epoch 2


def _segment(m, opt, sched, ds, noise, path, stop=None, **where):
    """train_epochs to the end, or to `stop` (one of CHECKPOINTS), where the run ends.  Every run writes its checkpoint at each of
    CHECKPOINTS, as a driver with that cadence does, and goes on from a rebuilt engine (arreau_amd.train.rebuild_engine).  Returns
    (the step losses of this segment, whether it reached the end)."""
    from arreau_amd.checkpoint import save_training_checkpoint
    from arreau_amd.train import rebuild_engine, train_epochs
    record = []

    def checkpoint(at, epoch, step, epochs_completed, batch):
        if at in CHECKPOINTS:
            save_training_checkpoint(path, m, opt, sched, epoch, step, batch, {"noise": noise}, epochs_completed=epochs_completed)
            rebuild_engine(m)
            if at == stop:
                raise _Stop()

    orig = m.training_step

    def step_and_record(batch, **kw):
        loss = orig(batch, **kw)
        record.append(loss.detach().clone())
        return loss

    m.training_step = step_and_record
    done = True
    try:
        train_epochs(m, ds, 3, 4, seed=2, optimizer=opt, scheduler=sched, noise=noise, log=lambda *a: None,
                     on_step=lambda epoch, batches, step: checkpoint((epoch, batches), epoch, step, epoch, batches),
                     on_epoch=lambda epoch, step: checkpoint((epoch, 0), epoch, step, epoch + 1, 0), **where)
    except _Stop:
        done = False
    finally:
        del m.training_step
    return [float(v) for v in torch.stack(record).cpu()], done


def _final_state(m, opt, sched):
    inner = opt.optimizer
    moments = [(inner.state[p]["exp_avg"].clone(), inner.state[p]["exp_avg_sq"].clone(), float(inner.state[p]["step"]))
               for g in inner.param_groups for p in g["params"] if p in inner.state and inner.state[p]]
    return dict(params=[p.detach().clone() for p in m.parameters()], moments=moments, ema=[e.clone() for e in opt.ema_params],
                current_step=opt.current_step, lr=[g["lr"] for g in inner.param_groups], last_epoch=sched.last_epoch)


@pytest.mark.parametrize("noise", ["host", "philox"])
def test_exact_resume_in_process(noise, tmp_path, monkeypatch):
    from arreau_amd import engine as engine_mod
    from arreau_amd.checkpoint import load_training_state
    from arreau_amd.diffusion.lattice_dataset import CrystalDataset, synthetic_alexandria_like
    ds = CrystalDataset(configs=synthetic_alexandria_like(12, 3, max_atoms=12))
    calls = []
    conv_stats = engine_mod.HipEngine.conv_stats
    monkeypatch.setattr(engine_mod.HipEngine, "conv_stats", lambda self: (calls.append(1), conv_stats(self))[1])
    # 3 epochs of 3 steps straight
    m, opt, sched = _fresh_run(ds, seed=7)
    torch.manual_seed(5)
    straight, done = _segment(m, opt, sched, ds, noise, str(tmp_path / "straight.ckpt"))
    assert done and len(straight) == 9 and len(calls) == 1  # the calibration of the first forward, once
    want = _final_state(m, opt, sched)
    # the same, stopped after epoch 1 (index 0) and again after step 2 of epoch 2 (index 1), each time rebuilt from the file alone
    path = str(tmp_path / "run.ckpt")
    m, opt, sched = _fresh_run(ds, seed=7)
    torch.manual_seed(5)
    got, done = _segment(m, opt, sched, ds, noise, path, stop=(0, 0))
    assert not done and len(got) == 3
    for stop in ((1, 2), None):
        del m, opt, sched
        m, opt, sched = _fresh_run(ds, seed=1000)  # other initial weights: everything comes from the file
        torch.manual_seed(999)
        st = load_training_state(path, m, opt, sched)
        part, done = _segment(m, opt, sched, ds, noise, path, stop=stop, start_epoch=st["epochs_completed"],
                              start_batch=st["batch_position"], global_step=st["global_step"])
        got += part
    assert done and len(calls) == 2  # ... and never again after a resume (the second call is the segmented run's first step)
    have = _final_state(m, opt, sched)
    print(f"noise={noise}: straight losses {straight}\n resumed losses {got}")
    assert got == straight
    assert have["current_step"] == want["current_step"] == 9 and have["lr"] == want["lr"] and have["last_epoch"] == want["last_epoch"]
    for key in ("params", "ema"):
        assert len(have[key]) == len(want[key])
        for i, (a, b) in enumerate(zip(have[key], want[key])):
            assert torch.equal(a, b), (key, i)
    assert len(have["moments"]) == len(want["moments"]) > 0
    for i, (a, b) in enumerate(zip(have["moments"], want["moments"])):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == 9, ("moments", i)


# ----------------------------------------------------------------------------------------------------------------------- 13
def _train_cli(args, tmp_path, ranks=1, limit=240):
    """python -m arreau_amd.train in fresh processes, under a time limit of its own, its exit status checked"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(PYTHONPATH=ROOT)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable]
    if ranks > 1:
        import socket
        env.update(ARREAU_TRAIN_BACKEND="gloo", ARREAU_TRAIN_ONE_DEVICE="1")
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1", "--master-port", str(port)]
    p = subprocess.run(cmd + ["-m", "arreau_amd.train"] + [str(a) for a in args], env=env, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return p.stdout


COMMON = ["--num_synthetic", 16, "--batch_size", 4, "--num_timesteps", T, "--warmup", 1, "--lr", "1e-3", "--ema_decay", "0.99"]


def test_command_line_run_resume_and_defaults(tmp_path):
    import json
    D = tmp_path / "ckpt"
    run = ["--epochs", 2, "--val_fraction", 0.25, "--val_interval", 1, "--checkpoint_dir", D, "--keep_best"]
    out = _train_cli(COMMON + run, tmp_path)
    names = sorted(os.listdir(D))
    print(out, names)
    for must in ("epoch=0.ckpt", "epoch=1.ckpt", "best.ckpt", "best-EMA.ckpt", "epoch=0.json", "best.json"):
        assert must in names, names
    table = json.load(open(D / "epoch=0.json"))
    assert len(table["weights"]["bins"]) == 10 and len(table["ema"]["bins"]) == 10 and table["weights"]["num_crystals"] == 4 * 4
    valid = [ln for ln in out.splitlines() if "valid loss" in ln]
    assert len(valid) == 4 and all(w in valid[0] for w in ("coordinates", "species", "lattice"))  # weights and EMA, two epochs
    final = [ln for ln in out.splitlines() if ln.startswith("final ")]
    assert len(final) == 2  # parameters and EMA
    resumed = _train_cli(COMMON + run + ["--resume", D / "epoch=0.ckpt"], tmp_path)
    assert [ln for ln in resumed.splitlines() if ln.startswith("final ")] == final
    assert [ln for ln in resumed.splitlines() if ln.startswith("epoch 1")] == [ln for ln in out.splitlines() if ln.startswith("epoch 1")]
    assert not any(ln.startswith("epoch 0") for ln in resumed.splitlines())
    # without any new flag: the driver's lines as they were -- one per epoch, nothing else
    plain = _train_cli(["--num_synthetic", 16, "--batch_size", 4, "--num_timesteps", T, "--warmup", 1, "--epochs", 2], tmp_path)
    lines = plain.splitlines()
    assert len(lines) == 2 and all(ln.startswith(f"epoch {e}: 4 steps, loss per crystal ") and ", last loss " in ln and ", lr " in ln
                                   for e, ln in enumerate(lines)), plain


def test_two_rank_validation_total_is_the_one_rank_total(tmp_path):
    import json
    from arreau_amd.diffusion.lattice_dataset import CrystalDataset, Subset, split_indices, synthetic_alexandria_like
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    D = tmp_path / "ckpt"
    out = _train_cli(COMMON + ["--epochs", 1, "--val_fraction", 0.25, "--val_interval", 1, "--checkpoint_dir", D, "--val_seed", 9], tmp_path,
                     ranks=2)
    valid = [ln for ln in out.splitlines() if "valid loss" in ln]
    assert len(valid) == 2 and all("the same on all 2 ranks" in ln for ln in valid), out  # (the driver compares the ranks' bits)
    table = json.load(open(D / "epoch=0.json"))
    # one rank, the same set, the weights that were validated (the epoch's checkpoint)
    ds = CrystalDataset(configs=synthetic_alexandria_like(16, 0))
    val = Subset(ds, split_indices(16, 0.25, 0)[1])
    m = PONITA_DIFFUSION.load_from_checkpoint(str(D / "epoch=0.ckpt"))
    one = m.evaluate(val, 4, 9, copies=4)
    print("two ranks:", table["weights"]["loss"], "one rank:", one["loss"])
    assert table["weights"]["num_crystals"] == one["num_crystals"] == 16
    np.testing.assert_allclose(_components(table["weights"]), _components(one), rtol=1e-5, atol=0)
