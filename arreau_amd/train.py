"""Data-parallel training driver for the score-matching step (BASELINE config 5: global batch 512 over 8 GPUs).

The role of main_diffusion.py:293-310 + Lightning's DDP, without pytorch_lightning: one process per GPU, every rank
takes a disjoint slice of each global batch (arreau_amd.diffusion.lattice_dataset.iterate_batches), runs
PONITA_DIFFUSION.training_step (forward + backward in libarreau_hip.so), the gradients are averaged with ONE all-reduce
of a flat fp32 bucket (1.17 M parameters = 4.7 MB; RCCL when the process group is "nccl"), clipped to norm 0.5
(main_diffusion.py:297) and applied by Adam (decay / no-decay groups) with the cosine warm-up schedule stepped per epoch.

    python -m torch.distributed.run --nproc-per-node 8 -m arreau_amd.train --epochs 2 --batch_size 64

`--ema_decay D` keeps an exponential moving average of the weights (arreau_amd.optim.EMAOptimizer, updated inside the optimizer's
launch); with `--out X.ckpt` rank 0 then also writes the averaged weights to `X-EMA.ckpt`, the checkpoint to sample from.

Training runs: `--val_data FILES` or `--val_fraction F` holds crystals out and `--val_interval E` logs their loss every E epochs
(PONITA_DIFFUSION.evaluate: keyed noise, the loss of the set as one batch, the same on every rank); `--checkpoint_dir D` with
`--checkpoint_every_n_epochs` / `--checkpoint_every_n_steps` writes training checkpoints (checkpoint.save_training_checkpoint),
`--keep_best` keeps the one with the lowest validation loss, and `--resume CKPT` continues a run from one bit for bit.
`--noise philox` draws the training noise in the kernels, keyed by (seed, epoch, crystal), instead of on the host.
"""
import argparse
import os
from typing import Iterable, Optional

import torch

GRAD_CLIP = 0.5  # main_diffusion.py:297 gradient_clip_val


def all_reduce_gradients(parameters: Iterable[torch.nn.Parameter], world_size: int, group=None):
    """Average `.grad` over the ranks with one collective on a flat bucket (what DDP does with its single 4.7 MB bucket
    for this model).  Parameters without a gradient on this rank contribute zeros.  Returns the number of elements."""
    params = [p for p in parameters if p.requires_grad and p.numel() > 0]
    if not params:
        return 0
    if world_size <= 1:  # nothing to exchange: leave the gradients where they are
        return sum(p.numel() for p in params)
    dev, dt = params[0].device, torch.float32
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).to(dt) for p in params])
    if world_size > 1:
        import torch.distributed as dist
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat /= world_size
    off = 0
    for p in params:
        n = p.numel()
        p.grad = flat[off:off + n].reshape(p.shape).to(device=dev, dtype=p.dtype)
        off += n
    return off


def _trainable_parameters(model):
    cache = model.__dict__.get("_trainable_parameter_cache")
    if cache is None:
        cache = model.__dict__["_trainable_parameter_cache"] = [p for p in model.parameters()]
    return cache


def optimizer_step(model, optimizer, world_size: int = 1, clip: Optional[float] = GRAD_CLIP, always_reduce: bool = False):
    """all-reduce -> clip -> Adam step -> invalidate the engine's packed weights.  Returns the gradient norm.

    When PONITA_DIFFUSION.training_step left every gradient as a view of the engine's flat buffer (`model._grad_flat`), the
    collective, the norm and the clip run on that ONE buffer: no gather into a bucket and no scatter back, one norm instead of a
    multi-tensor norm over 70 tensors (torch.nn.utils.clip_grad_norm_'s arithmetic: total 2-norm, coefficient
    max_norm / (norm + 1e-6) clamped to 1)."""
    flat = getattr(model, "_grad_flat", None)
    params = _trainable_parameters(model)
    if flat is not None and all(p.grad is None or p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for p in params):
        if world_size > 1 or always_reduce:  # (always_reduce: a one-rank group still runs the collective -- bench.py's RCCL rehearsal)
            import torch.distributed as dist
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
            flat /= world_size
        norm = None
        if hasattr(optimizer, "step_flat"):
            # arreau_amd.optim.ClipAdam: norm, clip coefficient, non-finite guard and the update of every tensor in two launches
            # ... and, where the module's engine keeps its own fp32 copy of a tensor, the update lands there in the same pass (then
            # only the two weights the engine reads in a derived form are rebuilt, instead of copying all 70 tensors twice)
            eng = getattr(model, "_engine", None)
            mirrors = eng.train_weight_mirrors(model) if eng is not None and hasattr(eng, "train_weight_mirrors") else None
            norm = optimizer.step_flat(flat, clip, mirrors)
            if norm is not None:
                optimizer.zero_grad(set_to_none=True)
                model._grad_flat = None
                if mirrors:
                    eng.refresh_derived_train_weights(model)
                else:
                    model.notify_parameters_changed()
                return norm
        if clip:
            norm = torch.linalg.vector_norm(flat, 2)
            flat.mul_(torch.clamp(clip / (norm + 1e-6), max=1.0))
            # A non-finite gradient (an activation beyond the fp16 range of the split-precision forward: ADVICE round 4) must not
            # reach Adam's moments before the periodic status check has switched the engine to the full-range products
            # (PONITA_DIFFUSION.training_step): such a step becomes a no-op -- on the device, no host synchronisation.
            flat.copy_(torch.where(torch.isfinite(norm), flat, torch.zeros_like(flat)))
    else:
        all_reduce_gradients(params, world_size)
        norm = torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], clip) if clip else None
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    model._grad_flat = None
    model.notify_parameters_changed()
    return norm


def configure_training(model, epochs: int, ema_decay: Optional[float] = None, ema_every_n_steps: int = 1):
    """(optimizer, LR scheduler) of configure_optimizers; with `ema_decay`, the optimizer is wrapped in an EMAOptimizer
    (arreau_amd.optim) -- the role of the reference's EMA callback -- and the scheduler stays on the inner one."""
    opt = model.configure_optimizers(max_epochs=epochs)
    optimizer, scheduler = opt["optimizer"], opt["lr_scheduler"]
    if ema_decay is not None:
        from .optim import EMAOptimizer
        optimizer = EMAOptimizer(optimizer, ema_decay, every_n_steps=ema_every_n_steps, module=model)
    return optimizer, scheduler


PHILOX_EPOCH_STRIDE = 0x9E3779B97F4A7C15  # the keyed training noise of epoch e runs under seed + e * this, mod 2^64


def epoch_noise_seed(seed: int, epoch: int) -> int:
    return (int(seed) + int(epoch) * PHILOX_EPOCH_STRIDE) % 2 ** 64


def train_epochs(model, dataset, epochs: int, batch_size: int, rank: int = 0, world_size: int = 1, seed: int = 0,
                 log=print, optimizer=None, scheduler=None, noise: str = "host", start_epoch: int = 0, start_batch: int = 0,
                 global_step: int = 0, on_step=None, on_epoch=None):
    """`batch_size` is per rank (global batch = batch_size * world_size).  Returns the list of per-step losses.
    `optimizer` / `scheduler`: from configure_training (default: configure_optimizers' own, no EMA).
    `noise`: "host" draws the step's noise from torch's CPU generator (the reference's order); "philox" draws it in the kernels,
    keyed by (epoch_noise_seed(seed, epoch), the crystal's dataset index).  `start_epoch` / `start_batch` / `global_step`: where a
    resumed run continues (the batches before start_batch of its first epoch are skipped by index arithmetic).
    `on_step(epoch, batches_done, global_step)` after every optimizer step and `on_epoch(epoch, global_step)` after every epoch's
    scheduler step: the driver's checkpoints and validation."""
    from .diffusion.lattice_dataset import iterate_batches
    from .diffusion.diffusion_loss import DiffusionLossMetric
    if noise not in ("host", "philox"):
        raise ValueError("noise must be 'host' or 'philox'")
    if optimizer is None:
        optimizer, scheduler = configure_training(model, epochs)
    losses = []
    for epoch in range(start_epoch, epochs):
        metric = DiffusionLossMetric()  # (diffusion_loss.py:52-65; the reference logs it per epoch with sync_dist)
        step_losses = []                # device scalars: read back once per epoch, not per step (no host sync in the loop)
        first = start_batch if epoch == start_epoch else 0
        keyed = dict(noise="philox", seed=epoch_noise_seed(seed, epoch)) if noise == "philox" else {}
        for step, batch in enumerate(iterate_batches(dataset, batch_size, shuffle=True, seed=seed + epoch, rank=rank,
                                                     world_size=world_size, drop_last=True, start=first), first):
            loss = model.training_step(batch, **keyed)
            optimizer_step(model, optimizer, world_size)
            global_step += 1
            step_losses.append(loss.detach())
            metric.update(loss, batch)
            if on_step is not None:
                on_step(epoch, step + 1, global_step)
        scheduler.step()
        if step_losses:
            losses += [float(v) for v in torch.stack(step_losses).cpu()]
        mean = float(metric.sync().compute())  # two scalar all-reduces: loss sum and crystal count over the ranks
        if getattr(model, "_engine", None) is not None:
            model._engine.check_status()  # sticky device flags of the whole epoch
        if rank == 0:
            log(f"epoch {epoch}: {len(step_losses)} steps, loss per crystal {mean:.5f} (all ranks), last loss "
                f"{losses[-1] if losses else float('nan'):.5f}, lr {scheduler.get_last_lr()[0]:.3e}")
        if on_epoch is not None:
            on_epoch(epoch, global_step)
    return losses


# the arguments of a run that must agree when it is resumed (checkpoint.save_training_checkpoint's run_args)
MODEL_ARGS = ("hidden_dim", "basis_dim", "layers", "widening_factor", "num_timesteps", "radius", "max_neighbors", "lr", "warmup",
              "weight_decay", "seed", "ema_decay", "ema_every_n_steps")


def run_arguments(args, world_size, train_len, val_len):
    """What a training checkpoint records of the run, and check_resume compares."""
    return {"world_size": int(world_size), "batch_size": int(args.batch_size), "noise": str(args.noise),
            "dataset_lengths": [int(train_len), int(val_len)], "model": {k: getattr(args, k) for k in MODEL_ARGS}}


def check_resume(state, run_args):
    """Reject, before any work, a resume the checkpoint's run does not continue: `state` is load_training_state's dict (ValueError
    there for a file without training state), `run_args` the present run's run_arguments."""
    saved = state.get("run_args") or {}
    for key, what in (("world_size", "world size"), ("batch_size", "batch size"), ("noise", "noise mode"),
                      ("dataset_lengths", "dataset lengths (training, validation)"), ("model", "model arguments")):
        if saved.get(key) != run_args[key]:
            raise ValueError(f"--resume: the checkpoint was written by a run with another {what}: {saved.get(key)!r}, now "
                             f"{run_args[key]!r}")


def rebuild_engine(model):
    """Drop the module's HIP engine and pack a fresh one from the parameters as they are -- what a run resumed from a checkpoint
    written now starts with.  An engine that has lived through optimizer steps is not that engine bit for bit (it chose its operand
    bounds when it was created, from the weights of that time), so the driver calls this on every rank wherever a training checkpoint
    is written: the run that goes on and the run that is resumed from the file are then the same computation."""
    model._engine = None
    model._drop_transient()
    eng = model.engine(for_training=True)
    if getattr(model, "_train_full_range", False):  # the run had left the fp16x3 forward products for the full-range ones
        eng.set_variant(3 if eng.fused_shape else -1, 1)
    return eng


class TrainingRun:
    """The driver's validation, checkpoints and best-so-far bookkeeping, as the two callbacks of train_epochs."""

    def __init__(self, model, optimizer, scheduler, args, run_args, rank, world_size, val_set=None, best_val_loss=None, log=print):
        self.model, self.optimizer, self.scheduler, self.args, self.run_args = model, optimizer, scheduler, args, run_args
        self.rank, self.world_size, self.val_set, self.best, self.log = rank, world_size, val_set, best_val_loss, log
        self.written = []
        if args.checkpoint_dir and rank == 0:
            os.makedirs(args.checkpoint_dir, exist_ok=True)

    def _rng_states(self):
        mine = torch.random.get_rng_state()
        if self.world_size <= 1:
            return [mine]
        import torch.distributed as dist
        states = [None] * self.world_size
        dist.all_gather_object(states, mine)
        return states

    def checkpoint(self, name, epoch, global_step, epochs_completed, batch_position):
        """every rank takes part (the generator states are gathered); rank 0 writes"""
        from .checkpoint import save_training_checkpoint
        states = self._rng_states()
        path = None
        if self.rank == 0:
            path = os.path.join(self.args.checkpoint_dir, name)
            save_training_checkpoint(path, self.model, self.optimizer, self.scheduler, epoch, global_step, batch_position,
                                     self.run_args, self.best, states, epochs_completed)
            self.written.append(path)
            self.log("wrote", path)
        rebuild_engine(self.model)  # every rank: what a resumed run starts with
        return path

    def on_step(self, epoch, batches_done, global_step):
        n = self.args.checkpoint_every_n_steps
        if self.args.checkpoint_dir and n and global_step % n == 0:
            self.checkpoint(f"epoch={epoch}-step={global_step}.ckpt", epoch, global_step, epoch, batches_done)

    def validate(self, epoch):
        a = self.args
        ev = dict(batch_size=a.batch_size, seed=a.val_seed, copies=a.val_copies, rank=self.rank, world_size=self.world_size)
        res = {"epoch": epoch, "weights": self.model.evaluate(self.val_set, **ev)}
        decides = res["weights"]
        if a.ema_decay is not None and len(self.optimizer.ema_params):
            with self.optimizer.swap_ema_weights():
                res["ema"] = decides = self.model.evaluate(self.val_set, **ev)
        if self.world_size > 1:  # every rank ran the one reduction on the summed table: the totals are the same bits
            import torch.distributed as dist
            totals = [None] * self.world_size
            dist.all_gather_object(totals, [res[k]["loss"] for k in sorted(res) if k != "epoch"])
            if any(t != totals[0] for t in totals):
                raise SystemExit(f"rank {self.rank}: the ranks hold different validation totals: {totals}")
        if self.rank == 0:
            for name in ("weights", "ema"):
                if name in res:
                    r = res[name]
                    self.log(f"epoch {epoch}: valid loss{' (EMA)' if name == 'ema' else ''} {r['loss']:.9g} (coordinates "
                             f"{r['error_frac_x']:.6g}, species {r['error_atomic_type']:.6g}, lattice {r['error_lattice']:.6g}; "
                             f"{r['num_crystals']} crystal-copies" + (f", the same on all {self.world_size} ranks)" if self.world_size > 1 else ")"))
        return res, decides["loss"]

    def on_epoch(self, epoch, global_step):
        import json
        a = self.args
        improved, res = False, None
        if self.val_set is not None and (epoch + 1) % a.val_interval == 0:
            res, loss = self.validate(epoch)
            improved = self.best is None or loss < self.best
            if improved:
                self.best = loss
        n = a.checkpoint_every_n_epochs
        path = None
        if a.checkpoint_dir and n and (epoch + 1) % n == 0:
            path = self.checkpoint(f"epoch={epoch}.ckpt", epoch, global_step, epoch + 1, 0)
        if a.checkpoint_dir and res is not None and self.rank == 0:
            table = os.path.splitext(path)[0] + ".json" if path else os.path.join(a.checkpoint_dir, f"epoch={epoch}.json")
            with open(table, "w") as fh:
                json.dump(res, fh, indent=1)
        if a.checkpoint_dir and a.keep_best and improved:
            best = self.checkpoint("best.ckpt", epoch, global_step, epoch + 1, 0)
            if self.rank == 0:
                with open(os.path.join(a.checkpoint_dir, "best.json"), "w") as fh:
                    json.dump(res, fh, indent=1)
                if a.ema_decay is not None:
                    from .checkpoint import save_ema_checkpoint
                    self.log("wrote", save_ema_checkpoint(best, self.model, self.optimizer))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", nargs="*", default=None, help="dataset files (lattice_dataset layout); synthetic if omitted")
    ap.add_argument("--num_synthetic", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch_size", type=int, default=64, help="crystals per rank")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=0)
    # network / diffusion flags of the reference's training CLI (main_diffusion.py:63-148; `make train`: --hidden_dim=200)
    ap.add_argument("--hidden_dim", type=int, default=128)
    ap.add_argument("--basis_dim", type=int, default=256)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--widening_factor", type=int, default=4)
    ap.add_argument("--num_timesteps", type=int, default=1000)
    ap.add_argument("--radius", type=float, default=5)
    ap.add_argument("--max_neighbors", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--weight_decay", type=float, default=1e-10)
    ap.add_argument("--out", type=str, default=None, help="write a Lightning-format checkpoint here (rank 0)")
    ap.add_argument("--ema_decay", type=float, default=None,
                    help="keep an exponential moving average of the weights with this decay; --out then also writes X-EMA.ckpt")
    ap.add_argument("--ema_every_n_steps", type=int, default=1, help="update the average every N optimizer steps")
    # training runs: validation, checkpoints, resume
    ap.add_argument("--val_data", nargs="*", default=None, help="validation set files (lattice_dataset layout)")
    ap.add_argument("--val_fraction", type=float, default=None,
                    help="hold this fraction of the data out for validation (a split by index seeded with --seed: the same on every "
                         "rank and in every run)")
    ap.add_argument("--val_interval", type=int, default=5, help="validate every E epochs (the reference's default)")
    ap.add_argument("--val_copies", type=int, default=4, help="noisings per validation crystal, at stratified timesteps")
    ap.add_argument("--val_seed", type=int, default=0, help="seed of the validation noise")
    ap.add_argument("--noise", choices=("host", "philox"), default="host",
                    help="training-step draws: torch's CPU generator, or keyed Philox draws in the kernels under the seed "
                         "seed + epoch * 0x9E3779B97F4A7C15 mod 2^64")
    ap.add_argument("--checkpoint_dir", type=str, default=None, help="where training checkpoints go")
    ap.add_argument("--checkpoint_every_n_epochs", type=int, default=1, help="with --checkpoint_dir: a checkpoint every N epochs (0: none)")
    ap.add_argument("--checkpoint_every_n_steps", type=int, default=0, help="with --checkpoint_dir: a checkpoint every N optimizer steps (0: none)")
    ap.add_argument("--keep_best", action="store_true",
                    help="with --checkpoint_dir and a validation set: best.ckpt (and best-EMA.ckpt with --ema_decay) whenever the "
                         "validation loss improves; with --ema_decay the average decides")
    ap.add_argument("--resume", type=str, default=None, help="continue from this training checkpoint")
    args = ap.parse_args()
    if args.val_data and args.val_fraction is not None:
        ap.error("give --val_data or --val_fraction, not both")
    if args.val_interval < 1 or args.val_copies < 1 or args.checkpoint_every_n_epochs < 0 or args.checkpoint_every_n_steps < 0:
        ap.error("--val_interval and --val_copies must be at least 1, the checkpoint cadences at least 0")
    if args.keep_best and not (args.checkpoint_dir and (args.val_data or args.val_fraction is not None)):
        ap.error("--keep_best needs --checkpoint_dir and a validation set")
    resumed = None
    if args.resume:  # rejected before any work: a file without training state
        from .checkpoint import load_lightning_checkpoint, load_training_state
        resumed = load_lightning_checkpoint(args.resume)
        try:
            load_training_state(resumed, restore_rng=False)
        except ValueError as e:
            ap.error(f"--resume {args.resume}: {e}")
    if args.ema_decay is not None and not 0.0 <= args.ema_decay <= 1.0:
        ap.error("--ema_decay must lie in [0, 1]")
    if args.ema_every_n_steps < 1:
        ap.error("--ema_every_n_steps must be at least 1")
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("ARREAU_TRAIN_ONE_DEVICE", "0") == "1":
        local_rank = 0
    from .checkpoint import default_args, save_ema_checkpoint, save_lightning_checkpoint
    from .diffusion.lattice_dataset import CrystalDataset, synthetic_alexandria_like
    from .lightning_wrappers.diffusion import PONITA_DIFFUSION
    ds = CrystalDataset(args.data) if args.data else CrystalDataset(configs=synthetic_alexandria_like(args.num_synthetic, args.seed))
    train_set, val_set = ds, None
    if args.val_fraction is not None:
        from .diffusion.lattice_dataset import Subset, split_indices
        train_idx, val_idx = split_indices(len(ds), args.val_fraction, args.seed)
        train_set, val_set = Subset(ds, train_idx), Subset(ds, val_idx)
    elif args.val_data:
        val_set = CrystalDataset(args.val_data)
        if not val_set.unique_atomic_numbers <= ds.unique_atomic_numbers:
            raise SystemExit("--val_data holds elements the training data does not")
        val_set.z_table = ds.z_table  # one class table: the model's
    run_args = run_arguments(args, world, len(train_set), len(val_set) if val_set is not None else 0)
    state = None
    if resumed is not None:  # rejected before any work: a run the checkpoint does not continue
        state = load_training_state(resumed, restore_rng=False)
        try:
            check_resume(state, run_args)
        except ValueError as e:
            raise SystemExit(str(e))
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("ARREAU_TRAIN_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    torch.manual_seed(args.seed)  # same initial weights on every rank
    net_args = default_args(lr=args.lr, epochs=args.epochs, hidden_dim=args.hidden_dim, basis_dim=args.basis_dim,
                            layers=args.layers, widening_factor=args.widening_factor, num_timesteps=args.num_timesteps,
                            radius=args.radius, max_neighbors=args.max_neighbors, warmup=args.warmup,
                            weight_decay=args.weight_decay)
    model = PONITA_DIFFUSION(net_args, ds.z_table).to(f"cuda:{local_rank}")
    torch.manual_seed(args.seed + 1000 + rank)  # different noise per rank
    optimizer, scheduler = configure_training(model, args.epochs, args.ema_decay, args.ema_every_n_steps)
    run = None
    if resumed is not None or val_set is not None or args.checkpoint_dir:
        where = dict(start_epoch=0, start_batch=0, global_step=0)
        if resumed is not None:
            state = load_training_state(resumed, model, optimizer, scheduler, rank=rank)
            where = dict(start_epoch=state["epochs_completed"], start_batch=state["batch_position"], global_step=state["global_step"])
            rebuild_engine(model)
            if rank == 0:
                print(f"resumed {args.resume}: epoch {where['start_epoch']}, batch {where['start_batch']}, step {where['global_step']}")
        run = TrainingRun(model, optimizer, scheduler, args, run_args, rank, world, val_set,
                          state["best_val_loss"] if state is not None else None)
        train_epochs(model, train_set, args.epochs, args.batch_size, rank, world, args.seed, optimizer=optimizer, scheduler=scheduler,
                     noise=args.noise, on_step=run.on_step, on_epoch=run.on_epoch, **where)
    else:
        train_epochs(model, ds, args.epochs, args.batch_size, rank, world, args.seed, optimizer=optimizer, scheduler=scheduler,
                     noise=args.noise)
    # data-parallel invariant: the replicas hold the same weights (same initial weights, same averaged gradients, ONE set
    # of calibration ratios); a drift here means a rank applied something its peers did not.  Each rank keeps its own average
    # of the weights (no collective): the averages of identical weights agree too.
    checks = [("parameter", list(model.parameters()))]
    if args.ema_decay is not None:
        checks.append(("EMA", list(optimizer.ema_params)))
    for what, tensors in checks:
        check = torch.stack([t.detach().double().sum() for t in tensors]).sum().reshape(1)
        if world > 1:
            sums = [torch.zeros_like(check) for _ in range(world)]
            if dist.get_backend() == "nccl":
                dist.all_gather(sums, check)
            else:
                host = [s.cpu() for s in sums]
                dist.all_gather(host, check.cpu())
                sums = host
            vals = [float(s) for s in sums]
            if rank == 0:
                print(f"replica {what} checksums:", " ".join(f"{v:.12e}" for v in vals))
            if max(vals) - min(vals) > 1e-9 * max(1.0, abs(vals[0])):
                raise SystemExit(f"rank {rank}: data-parallel replicas diverged ({what}): {vals}")
        elif run is not None:  # a training run: the line two runs that should agree are compared by
            print(f"final {what} checksum: {float(check):.17e}")
    if rank == 0 and args.out:
        print("wrote", save_lightning_checkpoint(args.out, model))
        if args.ema_decay is not None:
            print("wrote", save_ema_checkpoint(args.out, model, optimizer))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
