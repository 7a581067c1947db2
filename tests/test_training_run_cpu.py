"""Training runs without a GPU: the Philox restatement and the keyed timestep rule, batch iteration from a position, the seeded
validation split, the training-state round trip of a checkpoint, the binned reduction's rule and the rejections of --resume."""
import ctypes
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import training_run_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PHILOX_HOST = r"""
#define __host__
#define __device__
#include "philox.h"
#include <cstdio>
int main() {
    unsigned c0, c1, c2, c3, k0, k1;
    while (std::scanf("%u %u %u %u %u %u", &c0, &c1, &c2, &c3, &k0, &k1) == 6) {
        const Philox4 r = philox4x32_10(c0, c1, c2, c3, k0, k1);
        const unsigned long long seed = ((unsigned long long)k1 << 32) | k0;
        std::printf("%u %u %u %u %.17g\n", r.x[0], r.x[1], r.x[2], r.x[3], (double)philox_uniform(seed, c1, c2, c0, c3));
    }
    return 0;
}
"""


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = name and shutil.which(name)
        if path:
            return path
    pytest.fail("no host C++ compiler found (set CXX)")


# ------------------------------------------------------------------------------------------------------------------------ 1
def test_philox_restatement_against_known_answers_and_the_header(tmp_path):
    for ctr, key, res in C.KAT:
        assert tuple(int(v) for v in C.philox4x32_10(*ctr, *key)) == res
    src = tmp_path / "philox_host.cpp"
    src.write_text(PHILOX_HOST)
    exe = str(tmp_path / "philox_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "arreau_amd", "csrc"), str(src), "-o", exe],
                   check=True, capture_output=True, text=True)
    rng = np.random.RandomState(0)
    rows = rng.randint(0, 2 ** 32, size=(64, 6), dtype=np.uint64)
    rows[:3] = [list(ctr) + list(key) for ctr, key, _ in C.KAT]
    rows[3] = [0, 0, C.KIND_T, 4000000000, 3, 0]  # a keyed draw: (element 0, timestep 0, kind 9, id), seed 3
    out = subprocess.run([exe], input="\n".join(" ".join(str(int(v)) for v in r) for r in rows) + "\n", check=True,
                         capture_output=True, text=True).stdout.split("\n")
    for r, line in zip(rows, out):
        got = line.split()
        want = C.philox4x32_10(*[int(v) for v in r])
        assert [int(v) for v in got[:4]] == [int(v) for v in want]
        assert float(got[4]) == float(C.uniform(want))
    w = C.words(3, 0, 0, C.KIND_T, 4000000000)
    assert [int(v) for v in out[3].split()[:4]] == [int(v) for v in w]
    # the normal restatement is a standard normal (Box-Muller of two words)
    z = C.normal(C.words(9, np.arange(200000), 4, C.KIND_Z_FRAC, 17))
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("T", [10, 1000])
def test_integer_timestep_rule(R, T):
    from arreau_amd import _hip, build
    build.build(verbose=False)
    L = _hip.lib()

    def lib_rule(u24, copy):
        t = ctypes.c_int32()
        _hip.check(L.arreau_keyed_timestep(u24, copy, R, T, ctypes.byref(t)), "arreau_keyed_timestep")
        return t.value

    top = 0
    for copy in range(R):
        lo, hi = C.stratum(copy, R, T)
        # the strata cover 1..T in order without a gap; neighbours share their boundary timestep only where R does not divide T
        assert lo in ((top, top + 1) if T % R else (top + 1,)) and hi >= lo and (lo, hi) == (1 + copy * T // R, ((copy + 1) * T - 1) // R + 1)
        top = hi
        us = [0, 1, 2 ** 24 - 1, 2 ** 23] + [int(v) for v in np.random.RandomState(copy).randint(0, 2 ** 24, size=200)]
        for u24 in us:
            t = C.keyed_timestep(u24, copy, R, T)
            assert lo <= t <= hi and t == lib_rule(u24, copy)
            assert t == 1 + int(np.floor((copy + u24 / 2 ** 24) * T / R))  # (exact in float64 at these sizes)
            # the copies of one crystal share u24: their timesteps are strictly increasing, so never equal
            ts = [C.keyed_timestep(u24, c, R, T) for c in range(R)]
            assert all(a < b for a, b in zip(ts, ts[1:]))
    assert C.stratum(0, R, T)[0] == 1 and top == T  # both ends are reached: u24 = 0 of copy 0, u24 = 2^24 - 1 of the last copy
    with pytest.raises(ValueError):
        C.keyed_timestep(0, 0, T + 1, T)
    with pytest.raises(_hip.ArreauHipError):
        R_bad = ctypes.c_int32()
        _hip.check(L.arreau_keyed_timestep(0, 0, T + 1, T, ctypes.byref(R_bad)), "arreau_keyed_timestep")


# ------------------------------------------------------------------------------------------------------------------------ 2
def _dataset(n, seed=0):
    from arreau_amd.diffusion.lattice_dataset import CrystalDataset, synthetic_alexandria_like
    return CrystalDataset(configs=synthetic_alexandria_like(n, seed, max_atoms=6))


@pytest.mark.parametrize("n,batch,world,drop_last", [(23, 4, 1, False), (23, 4, 1, True), (23, 5, 2, True), (31, 3, 3, False), (8, 4, 1, True)])
def test_iterate_batches_from_a_position_is_the_tail_of_the_full_iteration(n, batch, world, drop_last):
    from arreau_amd.diffusion.lattice_dataset import iterate_batches
    ds = _dataset(n)
    order = np.arange(n)
    np.random.RandomState(7).shuffle(order)
    if world > 1:
        order = order[:n - n % world]
    for rank in range(world):
        kw = dict(shuffle=True, seed=7, rank=rank, world_size=world, drop_last=drop_last)
        full = list(iterate_batches(ds, batch, **kw))
        mine = order[rank::world]
        assert np.concatenate([b.index.numpy() for b in full]).tolist() == mine[:sum(len(b.index) for b in full)].tolist()
        assert all(b.index.dtype == torch.int64 for b in full)
        for k in range(len(full) + 2):
            tail = list(iterate_batches(ds, batch, start=k, **kw))
            assert len(tail) == max(len(full) - k, 0)
            for a, b in zip(tail, full[k:]):
                for f in ("X0", "A0", "L0", "num_atoms", "index", "batch", "ptr", "pos"):
                    assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_iterate_batches_with_a_start_builds_none_of_the_skipped_batches():
    from arreau_amd.diffusion.lattice_dataset import iterate_batches
    ds = _dataset(20)
    seen = []

    class Spy:
        def __len__(self):
            return len(ds)

        def __getitem__(self, i):
            seen.append(i)
            return ds[i]

    tail = list(iterate_batches(Spy(), 4, shuffle=True, seed=1, start=3))
    assert sorted(seen) == sorted(int(i) for b in tail for i in b.index) and len(seen) == 8


def test_validation_split_is_a_seeded_partition():
    from arreau_amd.diffusion.lattice_dataset import Subset, split_indices
    for n, f in ((12, 0.25), (101, 0.1), (2, 0.5)):
        tr, va = split_indices(n, f, seed=5)
        assert len(set(tr) & set(va)) == 0 and sorted(list(tr) + list(va)) == list(range(n)) and len(va) >= 1 and len(tr) >= 1
        for _ in range(3):  # every rank, every repeat
            tr2, va2 = split_indices(n, f, seed=5)
            assert (tr2 == tr).all() and (va2 == va).all()
    assert len(split_indices(12, 0.25, 0)[1]) == 3
    assert not np.array_equal(split_indices(101, 0.1, seed=5)[1], split_indices(101, 0.1, seed=6)[1])
    ds = _dataset(12)
    sub = Subset(ds, split_indices(12, 0.25, 0)[1])
    assert len(sub) == 3 and torch.equal(sub[1].X0, ds[int(sub.indices[1])].X0) and sub.z_table is ds.z_table
    with pytest.raises(ValueError):
        split_indices(12, 1.0)


# ------------------------------------------------------------------------------------------------------------------------ 3
def _small_model(seed=1):
    from arreau_amd.checkpoint import make_synthetic_model
    return make_synthetic_model(S=5, seed=seed, hidden_dim=16, basis_dim=16, layers=1, widening_factor=2, num_timesteps=10)


def _trained_state(m, steps=3, epochs=3):
    """Adam with the module's two groups under an EMAOptimizer, `steps` CPU steps on made-up gradients, the scheduler at `epochs`"""
    from arreau_amd.optim import EMAOptimizer
    from arreau_amd.lightning_wrappers.scheduler import CosineWarmupScheduler
    cfg = m.configure_optimizers(max_epochs=10)
    inner = cfg["optimizer"]
    assert len(inner.param_groups) == 2
    opt = EMAOptimizer(inner, 0.9, module=m)
    sched = CosineWarmupScheduler(inner, 2, 10)
    g = torch.Generator().manual_seed(11)
    for _ in range(steps):
        for p in m.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=g) * 1e-2
        opt.step()
    for _ in range(epochs):
        sched.step()
    return opt, sched


def test_training_state_round_trip(tmp_path):
    from arreau_amd import checkpoint as ck
    from arreau_amd.lightning_wrappers.diffusion import PONITA_DIFFUSION
    m = _small_model()
    opt, sched = _trained_state(m)
    m._train_full_range = True
    torch.manual_seed(123)
    torch.rand(5)
    path = str(tmp_path / "run.ckpt")
    run_args = {"world_size": 1, "batch_size": 4, "noise": "host", "dataset_lengths": [9, 3], "model": {"hidden_dim": 16}}
    ck.save_training_checkpoint(path, m, opt, sched, epoch=2, global_step=7, batch_position=1, run_args=run_args, best_val_loss=0.25,
                                epochs_completed=2)
    expect = torch.rand(4)  # the generator's next draws after the save
    # a fresh module, optimizer and scheduler, from the file alone
    m2 = _small_model(seed=2)
    from arreau_amd.optim import EMAOptimizer
    from arreau_amd.lightning_wrappers.scheduler import CosineWarmupScheduler
    inner2 = m2.configure_optimizers(max_epochs=10)["optimizer"]
    opt2, sched2 = EMAOptimizer(inner2, 0.5, module=m2), CosineWarmupScheduler(inner2, 2, 10)
    torch.manual_seed(999)
    st = ck.load_training_state(path, m2, opt2, sched2)
    assert torch.equal(torch.rand(4), expect)
    assert (st["epoch"], st["global_step"], st["epochs_completed"], st["batch_position"]) == (2, 7, 2, 1)
    assert st["run_args"] == run_args and st["best_val_loss"] == 0.25 and st["train_full_range"] is True and m2._train_full_range
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert opt2.decay == 0.9 and opt2.current_step == opt.current_step == 3
    assert len(opt2.ema_params) == len(opt.ema_params) > 0
    for a, b in zip(opt.ema_params, opt2.ema_params):
        assert torch.equal(a, b)
    for ga, gb in zip(opt.optimizer.param_groups, opt2.optimizer.param_groups):
        assert ga["lr"] == gb["lr"] and ga["weight_decay"] == gb["weight_decay"] and len(ga["params"]) == len(gb["params"])
        for pa, pb in zip(ga["params"], gb["params"]):
            sa, sb = opt.optimizer.state[pa], opt2.optimizer.state[pb]
            assert sa.keys() == sb.keys()
            if sa:
                assert float(sa["step"]) == float(sb["step"]) == 3
                assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert sched2.last_epoch == sched.last_epoch == 3 and sched2.get_last_lr() == sched.get_last_lr()
    # ... and both continue alike
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for mm, oo, gg in ((m, opt, g1), (m2, opt2, g2)):
        for p in mm.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=gg) * 1e-2
        oo.step()
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    # load_from_checkpoint reads a training checkpoint as it reads any
    m3 = PONITA_DIFFUSION.load_from_checkpoint(path)
    sd = ck.load_lightning_checkpoint(path)["state_dict"]
    assert len(m3.state_dict()) > 0
    for k, v in m3.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k


def test_plain_checkpoint_is_what_it_was_and_holds_no_training_state(tmp_path):
    from arreau_amd import checkpoint as ck
    m = _small_model()
    plain = ck.load_lightning_checkpoint(ck.save_lightning_checkpoint(str(tmp_path / "plain.ckpt"), m))
    assert set(plain) == {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "loops", "callbacks", "optimizer_states",
                          "lr_schedulers", "hparams_name", "hyper_parameters"}
    assert (plain["epoch"], plain["global_step"], plain["loops"], plain["callbacks"], plain["optimizer_states"], plain["lr_schedulers"],
            plain["hparams_name"], plain["pytorch-lightning_version"]) == (0, 0, {}, {}, [], [], "kwargs", "2.2.1")
    with pytest.raises(ValueError, match="no training state"):
        ck.load_training_state(plain)
    opt, sched = _trained_state(m)
    full = ck.load_lightning_checkpoint(ck.save_training_checkpoint(str(tmp_path / "run.ckpt"), m, opt, sched, 0, 3))
    assert set(full) == set(plain)  # the same slots, filled
    assert set(full["state_dict"]) == set(plain["state_dict"])


# ------------------------------------------------------------------------------------------------------------------------ 4
def test_binned_reduction_rule_on_hand_made_rows():
    T, n_bins = 10, 4
    # uneven bins: t = 1..10 -> (t - 1) * 4 // 10 = 0 0 0 1 1 2 2 2 3 3
    assert [C.bin_of(t, n_bins, T) for t in range(1, 11)] == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3]
    sums = np.array([[1, 2, 3, 4], [0, 0, 0, 0], [10, 20, 30, 40], [0.5, 0.25, 0.125, 1], [0, 0, 0, 0], [7, 7, 7, 7]], dtype=np.float32)
    atoms = np.array([2, 0, 5, 1, 0, 3])
    t = np.array([1, 0, T, 4, 0, 3])
    out, cnt, unwritten = C.reduce_rows(sums, atoms, t, n_bins, T)
    assert unwritten == 2
    assert out[0].tolist() == [8, 9, 10, 11] and cnt[0].tolist() == [5, 2]       # t = 1 and t = 3
    assert out[1].tolist() == [0.5, 0.25, 0.125, 1] and cnt[1].tolist() == [1, 1]  # t = 4
    assert out[2].tolist() == [0, 0, 0, 0] and cnt[2].tolist() == [0, 0]
    assert out[3].tolist() == [10, 20, 30, 40] and cnt[3].tolist() == [5, 1]      # t = T
    assert out[4].tolist() == [18.5, 29.25, 40.125, 52] and cnt[4].tolist() == [11, 4]
    assert (out[:n_bins].sum(0) == out[n_bins]).all() and (cnt[:n_bins].sum(0) == cnt[n_bins]).all()
    # the set loss from the total record: (coord + 0.001 vb + ce) / N + lattice / (3 B)
    assert C.set_loss(out[4], cnt[4]) == pytest.approx((18.5 + 0.001 * 29.25 + 40.125) / 11 + 52 / 12, rel=1e-15)


# ------------------------------------------------------------------------------------------------------------------------ 5
def _run_args(**over):
    args = SimpleNamespace(batch_size=4, noise="host", hidden_dim=128, basis_dim=256, layers=5, widening_factor=4, num_timesteps=1000,
                           radius=5, max_neighbors=8, lr=3e-4, warmup=10, weight_decay=1e-10, seed=0, ema_decay=None, ema_every_n_steps=1)
    world, lengths = over.pop("world_size", 1), over.pop("dataset_lengths", (9, 3))
    for k, v in over.items():
        setattr(args, k, v)
    from arreau_amd.train import run_arguments
    return run_arguments(args, world, *lengths)


@pytest.mark.parametrize("change,what", [(dict(world_size=2), "world size"), (dict(batch_size=8), "batch size"), (dict(noise="philox"), "noise mode"),
                                         (dict(dataset_lengths=(10, 3)), "dataset lengths"), (dict(dataset_lengths=(9, 2)), "dataset lengths"),
                                         (dict(hidden_dim=64), "model arguments"), (dict(num_timesteps=100), "model arguments")])
def test_resume_rejections(change, what):
    from arreau_amd.train import check_resume
    state = {"run_args": _run_args()}
    check_resume(state, _run_args())
    with pytest.raises(ValueError, match=what):
        check_resume(state, _run_args(**change))


def test_resume_is_rejected_before_a_device_is_touched(tmp_path, monkeypatch, capsys):
    """the command line: a file without training state, then a run that disagrees with the checkpoint's -- both end before
    torch.cuda.set_device, the driver's first device call"""
    from arreau_amd import checkpoint as ck, train
    m = _small_model()
    plain = ck.save_lightning_checkpoint(str(tmp_path / "plain.ckpt"), m)
    opt, sched = _trained_state(m)
    args = SimpleNamespace(batch_size=4, noise="host", hidden_dim=128, basis_dim=256, layers=5, widening_factor=4, num_timesteps=1000,
                           radius=5.0, max_neighbors=8, lr=3e-4, warmup=10, weight_decay=1e-10, seed=0, ema_decay=None, ema_every_n_steps=1)
    run = ck.save_training_checkpoint(str(tmp_path / "run.ckpt"), m, opt, sched, 0, 3, run_args=train.run_arguments(args, 1, 12, 0))

    def touched(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(torch.cuda, "set_device", touched)
    for argv, msg in ((["--resume", plain], "no training state"), (["--resume", run, "--num_synthetic", "12", "--batch_size", "8"], "batch size"),
                      (["--resume", run, "--num_synthetic", "13", "--batch_size", "4"], "dataset lengths"),
                      (["--resume", run, "--num_synthetic", "12", "--batch_size", "4", "--noise", "philox"], "noise mode"),
                      (["--resume", run, "--num_synthetic", "12", "--batch_size", "4", "--hidden_dim", "64"], "model arguments")):
        monkeypatch.setattr(sys, "argv", ["arreau_amd.train"] + argv)
        monkeypatch.setenv("WORLD_SIZE", "1")
        with pytest.raises(SystemExit) as e:
            train.main()
        assert msg in (str(e.value) + capsys.readouterr().err), (argv, e.value)
    monkeypatch.setattr(sys, "argv", ["arreau_amd.train", "--resume", run, "--num_synthetic", "12", "--batch_size", "4"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        train.main()
    assert "world size" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(AssertionError, match="the device was touched"):  # a run that agrees gets as far as the device
        train.main()
