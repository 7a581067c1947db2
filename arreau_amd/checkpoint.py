"""Lightning-format checkpoint I/O without pytorch_lightning, plus a synthetic-checkpoint writer.

The reference's checkpoints are Lightning 2.2.1 dicts: `state_dict`,
`hyper_parameters` = {args: argparse.Namespace, z_table: AtomicNumberTable} (pickled by
save_hyperparameters, lightning_wrappers/diffusion.py:34) and trainer bookkeeping.  The pickled
class path is `diffusion.tools.atomic_number_table.AtomicNumberTable`; it is remapped onto this
package's class when loading and restored when saving, so files round-trip with the reference.
"""
import argparse
import contextlib
import os
import pickle
import sys
import types

import torch

from .diffusion.tools import atomic_number_table as _ant

_REF_ANT_MODULE = "diffusion.tools.atomic_number_table"


class _Stub:
    """Placeholder for classes of packages that are not installed (trainer/callback state)."""

    def __init__(self, *a, **kw):
        pass

    def __setstate__(self, state):
        self.__dict__["state"] = state


class _RemapUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module == _REF_ANT_MODULE or module.endswith(".atomic_number_table"):
            return getattr(_ant, name)
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            return _Stub


_pickle_module = types.ModuleType("arreau_amd._ckpt_pickle")
_pickle_module.__dict__.update({k: getattr(pickle, k) for k in dir(pickle) if not k.startswith("__")})
_pickle_module.Unpickler = _RemapUnpickler
_pickle_module.load = lambda f, **kw: _RemapUnpickler(f, **kw).load()


def load_lightning_checkpoint(path):
    """Read a Lightning checkpoint dict on the CPU (weights stay in their stored dtype)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_pickle_module)
    if "state_dict" not in ckpt or "hyper_parameters" not in ckpt:
        raise ValueError(f"{path} is not a Lightning checkpoint (needs state_dict and hyper_parameters)")
    hp = ckpt["hyper_parameters"]
    if not isinstance(hp, dict):
        hp = dict(getattr(hp, "__dict__", hp))
        ckpt["hyper_parameters"] = hp
    return ckpt


@contextlib.contextmanager
def _reference_class_paths():
    """Pickle AtomicNumberTable under the reference's module path."""
    saved_mods = {}
    chain = ["diffusion", "diffusion.tools", _REF_ANT_MODULE]
    for name in chain:
        saved_mods[name] = sys.modules.get(name)
        if name == _REF_ANT_MODULE:
            sys.modules[name] = _ant
        elif name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    old = _ant.AtomicNumberTable.__module__
    _ant.AtomicNumberTable.__module__ = _REF_ANT_MODULE
    try:
        yield
    finally:
        _ant.AtomicNumberTable.__module__ = old
        for name, mod in saved_mods.items():
            if mod is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = mod


def save_lightning_checkpoint(path, module, include_ori_grid=True, weights=None, trainer_state=None):
    """Write `module` (a PONITA_DIFFUSION) as a Lightning-format checkpoint.  `weights` {state_dict key: tensor}: values written in
    place of the module's own (save_ema_checkpoint).  `trainer_state`: entries that replace the empty trainer bookkeeping (epoch,
    global_step, loops, optimizer_states, lr_schedulers: save_training_checkpoint)."""
    from .lightning_wrappers.diffusion import ORI_GRID_KEY
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    for k, v in (weights or {}).items():
        if k not in sd or tuple(v.shape) != tuple(sd[k].shape):
            raise ValueError(f"{k}: not an entry of the module's state_dict with shape {tuple(v.shape)}")
        sd[k] = v.detach().to("cpu", sd[k].dtype).clone()
    if include_ori_grid:
        sd[ORI_GRID_KEY] = module.model.ori_grid.detach().cpu().clone()
    ckpt = {
        "epoch": 0, "global_step": 0, "pytorch-lightning_version": "2.2.1", "state_dict": sd,
        "loops": {}, "callbacks": {}, "optimizer_states": [], "lr_schedulers": [],
        "hparams_name": "kwargs",
        "hyper_parameters": {"args": module.hparams.args, "z_table": module.hparams.z_table},
    }
    ckpt.update(trainer_state or {})
    with _reference_class_paths():
        torch.save(ckpt, path)
    return path


TRAINING_LOOP_KEY = "arreau_amd.training"  # the entry of `loops` that holds what arreau_amd.train needs to continue a run


def _to_cpu(obj):
    """Tensors of a nested state_dict as CPU copies with storage of their own (an optimizer's moments are views of flat buffers)."""
    if torch.is_tensor(obj):
        return obj.detach().to("cpu", copy=True)
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def save_training_checkpoint(path, module, optimizer, scheduler, epoch, global_step, batch_position=0, run_args=None,
                             best_val_loss=None, rng_states=None, epochs_completed=None):
    """save_lightning_checkpoint's file with the trainer slots filled, so that a run can continue from it bit for bit:
    `epoch`, `global_step`; `optimizer_states` = [optimizer.state_dict()] (a torch optimizer's, or an EMAOptimizer's with the
    average inside); `lr_schedulers` = [scheduler.state_dict()]; and under loops[TRAINING_LOOP_KEY] what the driver itself needs:
    the epochs completed and the batch position inside the epoch in progress, torch's CPU generator state (`rng_states`: one per
    rank; default this process's), the run's arguments that must agree on resume (`run_args`, a dict), the engine's full-range
    switch and status cadence (module._train_full_range, module._train_steps) and the best validation loss so far.
    PONITA_DIFFUSION.load_from_checkpoint reads the file as it reads any checkpoint."""
    loop = {"epochs_completed": int(epoch if epochs_completed is None else epochs_completed), "batch_position": int(batch_position),
            "cpu_rng_states": [s.clone() for s in (rng_states if rng_states is not None else [torch.random.get_rng_state()])],
            "run_args": dict(run_args or {}), "train_full_range": bool(getattr(module, "_train_full_range", False)),
            "train_steps": int(getattr(module, "_train_steps", 0)),
            "best_val_loss": None if best_val_loss is None else float(best_val_loss)}
    state = {"epoch": int(epoch), "global_step": int(global_step), "optimizer_states": [_to_cpu(optimizer.state_dict())],
             "lr_schedulers": [_to_cpu(scheduler.state_dict())] if scheduler is not None else [], "loops": {TRAINING_LOOP_KEY: loop}}
    return save_lightning_checkpoint(path, module, trainer_state=state)


def load_training_state(checkpoint, module=None, optimizer=None, scheduler=None, rank=0, restore_rng=True):
    """The training state of a file save_training_checkpoint wrote (a path, or the dict load_lightning_checkpoint returned).
    Raises ValueError for a checkpoint without one.  Given `module` / `optimizer` / `scheduler`, their state is restored from it
    (weights and buffers strictly; moments, step counts, the average, LRs; the full-range switch), and with restore_rng torch's
    CPU generator is set to the state saved for `rank`.  Returns the loops[TRAINING_LOOP_KEY] dict plus epoch and global_step."""
    ckpt = load_lightning_checkpoint(checkpoint) if not isinstance(checkpoint, dict) else checkpoint
    loop = (ckpt.get("loops") or {}).get(TRAINING_LOOP_KEY)
    if loop is None or not ckpt.get("optimizer_states"):
        raise ValueError("the checkpoint holds no training state (it was not written by save_training_checkpoint)")
    state = dict(loop, epoch=int(ckpt["epoch"]), global_step=int(ckpt["global_step"]))
    if module is not None:
        module.load_state_dict(ckpt["state_dict"], strict=True)
        module._train_full_range = bool(loop["train_full_range"])
        module._train_steps = int(loop["train_steps"])
    if optimizer is not None:
        optimizer.load_state_dict(ckpt["optimizer_states"][0])
    if scheduler is not None and ckpt.get("lr_schedulers"):
        scheduler.load_state_dict(ckpt["lr_schedulers"][0])
    if restore_rng:
        states = loop["cpu_rng_states"]
        if rank >= len(states):
            raise ValueError(f"the checkpoint holds the generator states of {len(states)} rank(s), not of rank {rank}")
        torch.random.set_rng_state(states[rank])
    return state


def ema_checkpoint_path(path):
    """Where the EMA twin of checkpoint `path` goes: the extension replaced by `-EMA` plus the extension (the reference's EMA
    callback, lightning_wrappers/callbacks.py:113-170: `model.ckpt` -> `model-EMA.ckpt`)."""
    root, ext = os.path.splitext(os.fspath(path))
    return f"{root}-EMA{ext}"


def save_ema_checkpoint(path, module, ema_optimizer):
    """Write the EMA twin of checkpoint `path` (ema_checkpoint_path) for `module` trained with `ema_optimizer`
    (arreau_amd.optim.EMAOptimizer): its state_dict holds the average of every parameter the optimizer steps; buffers, the
    orientation grid and the hyper-parameters are the module's.  PONITA_DIFFUSION.load_from_checkpoint reads it as it reads any
    checkpoint.  Returns the path written."""
    names = {id(p): k for k, p in module.named_parameters()}
    weights = {names[id(p)]: e for p, e in zip(ema_optimizer.all_parameters(), ema_optimizer.ema_params) if id(p) in names}
    return save_lightning_checkpoint(ema_checkpoint_path(path), module, weights=weights)


def default_args(**overrides):
    """argparse.Namespace with the defaults of the reference's training CLI (main_diffusion.py:34-148)
    and the Makefile preset for the sampler-relevant flags (radius 5, max_neighbors 8, T 1000)."""
    d = dict(epochs=10000, warmup=10, batch_size=100, lr=1e-3, weight_decay=1e-10, log=True,
             enable_progress_bar=False, num_workers=0, seed=0, val_interval=5, train_augm=False,
             dataset="alexandria", radius=5, loop=True, num_ori=16, hidden_dim=128, basis_dim=256, degree=3,
             layers=5, widening_factor=4, layer_scale=1e-6, multiple_readouts=True, num_timesteps=1000,
             max_neighbors=8, experiment_name=None, profiler=False, gpus=1)
    d.update(overrides)
    return argparse.Namespace(**d)


def make_synthetic_model(S=90, seed=1234, trained_like=True, ori_grid=None, pooled_readout_scale=None, **arg_overrides):
    """Random-weight PONITA_DIFFUSION in the reference's layout (the real checkpoint is a download
    that is unavailable offline).  Default PyTorch initialisers under torch.manual_seed(seed), like
    the reference constructors.  `trained_like=True` additionally randomises the tensors whose
    initial values hide the network from a parity test (layer_scale = 1e-6 scales every ConvNext
    branch to nothing; zero conv bias; unit LayerNorm): layer_scale ~ U(0.1, 1), conv.bias ~ N(0, 0.1),
    norm.weight ~ U(0.5, 1.5), norm.bias ~ N(0, 0.1).  `pooled_readout_scale` multiplies the read-out rows (and biases) of
    the three per-crystal scalars (split order [S, 1, 0, 3], ponita.py:108-117): random rows make the pooled prediction
    `pred_lengths_0` a sum of ~n values of order 3 (|len0| ~ 58 at 20 atoms), whereas a trained model predicts lengths / n =
    O(1) (diffusion_loss.py:264-267); e.g. 1/32 gives a model whose three outputs are all of order one."""
    from .lightning_wrappers.diffusion import PONITA_DIFFUSION
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(seed)
        zs = list(range(1, S)) + [_ant.AtomicNumberTable.MASK_ATOMIC_NUMBER]
        model = PONITA_DIFFUSION(default_args(**arg_overrides), _ant.AtomicNumberTable(zs), ori_grid=ori_grid)
        if trained_like:
            with torch.no_grad():
                for layer in model.model.interaction_layers:
                    if layer.layer_scale is not None:
                        layer.layer_scale.uniform_(0.1, 1.0)
                    layer.conv.bias.normal_(0.0, 0.1)
                    layer.norm.weight.uniform_(0.5, 1.5)
                    layer.norm.bias.normal_(0.0, 0.1)
        if pooled_readout_scale is not None:
            with torch.no_grad():
                for ro in model.model.read_out_layers:
                    ro.weight[S + 1:S + 4] *= float(pooled_readout_scale)
                    ro.bias[S + 1:S + 4] *= float(pooled_readout_scale)
    finally:
        torch.random.set_rng_state(state)
    return model
