"""DiffusionLoss: the sampling loop of the reference (diffusion/diffusion_loss.py:276-377) and the forward part of
its training loss (`__call__`, :204-274) driving the HIP engine.  The backward pass through the network kernels is not
built yet, so `__call__` returns the loss value (and the gradients with respect to the network outputs), not an
autograd graph."""
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import os

import torch
import torch.nn as nn

from . import corrector as pc
from . import instruments
from . import inversion
from . import keyed as keyed_mod
from . import multistep as multistep_mod
from . import respacing
from . import sample_plan
from . import species as species_mod
from . import contact_guidance as guidance_mod
from . import xrd_guidance as xrd_guidance_mod
from .d3pm import D3PM
from . import lattice_systems
from . import symmetry as sym_mod
from .diffusion_helpers import VE_pbc, VP_lattice, crystal_offsets
from .inference.visualize_crystal import VisualizationSetting, vis_crystal_during_sampling
from .lattice_helpers import lattice_from_params
from .tools.atomic_number_table import AtomicNumberTable, atomic_number_indexes_to_atomic_numbers

pos_sigma_min = 0.001
pos_sigma_max = 1.0
type_power = 2
lattice_power = 2
type_clipmax = 0.999
lattice_clipmax = 0.999


@dataclass
class SampleResult:
    """Same fields as the reference (diffusion_loss.py:39-49)."""
    frac_x: Optional[np.ndarray] = None
    atomic_numbers: Optional[np.ndarray] = None
    lattice: Optional[np.ndarray] = None
    idx_start: Optional[np.ndarray] = None
    num_atoms: Optional[np.ndarray] = None
    # extension (not in the reference): what the library did to produce this batch -- e.g. {"full_range_rerun": True} when an
    # activation left the fp16 range of the default kernels and the batch was re-run on the full-range bf16x6 kernels
    info: Optional[dict] = None
    # extension: the structural screen of the final state (sample(screen=...); diffusion/screening.py) -- numpy arrays min_distance,
    # pair, n_close, volume, number_density, flags and valid, one entry per crystal; None when no screen was asked for
    metrics: Optional[dict] = None
    # extension: duplicate detection on the final state (sample(unique=...); diffusion/uniqueness.py) -- numpy arrays duplicate_of,
    # distance, nearest, nearest_distance, flags and unique, one entry per crystal; None when it was not asked for
    uniqueness: Optional[dict] = None
    # extension: the symmetry search of the final state (sample(find_symmetry=...); diffusion/symmetry_search.py) -- numpy arrays
    # n_lattice, n_ops, n_translations, ops_rotation, ops_translation, ops_residual, residual, point_group, flags, symprec and the
    # float32 lattice the search saw; None when it was not asked for
    symmetry: Optional[dict] = None
    # extension: the cell reduction of the final state (sample(reduce_cell=...); diffusion/cell_reduction.py) -- numpy arrays
    # multiplicity, n_translations, lattice, transform, num_atoms, flags, selling_steps and symprec, one row per crystal, and the
    # reduced crystals' frac_x, atomic_numbers and keep as a dense ragged batch; None when it was not asked for
    reduced: Optional[dict] = None
    # extension: the symmetrization of the final state (sample(symmetrize=...); diffusion/symmetrize.py) -- numpy arrays frac_x,
    # orbit, orbit_size and site_order, one row per atom of the crystals as sampled, and lattice, lengths, angles, n_orbits,
    # max_displacement, rms_displacement, ops_translation and flags, one row per crystal; None when it was not asked for
    symmetrized: Optional[dict] = None
    # extension: keyed sampling (sample(crystal_keys=...); diffusion/keyed.py) -- the int64 key of every crystal; None when the run
    # was not keyed
    crystal_keys: Optional[np.ndarray] = None
    # extension: the structure match of the final state against targets (sample(match_to=...); diffusion/structure_match.py) -- numpy
    # arrays target, n_comparable, rms, rms_norm, max_dist, mapping, translation, n_mappings, n_candidates, n_permutations, matched
    # and flags, one row per crystal, and partner, one row per atom; None when it was not asked for
    match: Optional[dict] = None
    # extension: the conventional cells of the final state (sample(conventional_cell=...); diffusion/conventional_cell.py) -- numpy
    # arrays lattice, lengths, angles, transform, centring, bravais, n_points, num_atoms and flags, one row per crystal, and the
    # conventional crystals' frac_x, atomic_numbers and source as a dense ragged batch; None when it was not asked for
    conventional: Optional[dict] = None
    # extension: the coordination environments of the final state (sample(coordination=...); diffusion/coordination.py) -- numpy
    # arrays n_bonds, n_mutual, min_cn, max_cn, mean_cn and flags, one row per crystal, and cn, neighbors [.., max_neighbors, 4],
    # nearest, farthest, mutual and species, one row per atom; None when it was not asked for
    coordination: Optional[dict] = None
    # extension: the bond angles and Steinhardt order parameters of the final state (sample(bond_order=...);
    # diffusion/bond_order.py) -- numpy arrays mean_q [.., 4], n_angles, angle_hist [.., 37], flags and coord_flags, one row per
    # crystal, and n_used, q and q2 [.., 4], cos_min, cos_max, angles [.., 37] and species, one row per atom; None when it was not
    # asked for
    bond_order: Optional[dict] = None
    # extension: the Voronoi cells of the final state (sample(voronoi=...); diffusion/voronoi.py) -- numpy arrays n_faces, min_cn,
    # max_cn, mean_cn, mean_cn_eff, volume_sum and flags, one row per crystal, and cn, neighbors [.., max_faces, 4], face_weight,
    # face_solid_angle, face_area, face_distance [.., max_faces], volume, omega_sum, max_radius, cn_eff, atom_flags and species,
    # one row per atom; None when it was not asked for
    voronoi: Optional[dict] = None
    # extension: the powder diffraction patterns of the final state (sample(xrd=...); diffusion/xrd.py) -- numpy arrays pattern
    # [.., n_points], n_reflections, volume, weight_sum, flags, max_intensity, two_theta_peak and grid [.., 5] (the grid-defining
    # parameters: the 2 theta values are xrd.grid(row)), one row per crystal; None when it was not asked for
    xrd: Optional[dict] = None
    # extension: the Ewald electrostatics of the final state (sample(ewald=...); diffusion/ewald.py) -- numpy arrays energy, real,
    # reciprocal, self, background (eV), net_charge, alpha, volume, n_pairs, n_reciprocal, flags and energy_per_atom, one row per
    # crystal, and potential (V), charge and species, one row per atom; None when it was not asked for
    ewald: Optional[dict] = None


class _PinnedRing:
    """Page-locked staging buffers owned by the caller and reused round-robin: no pinned allocation per step (hipHostMalloc
    maps the block into the GPU's page tables) and an explicit rule for reuse -- a slot is taken again only after the event
    recorded behind its last copy has completed; with four slots that wait is over long before the slot comes round."""
    SLOTS = 4

    def __init__(self):
        self.slots = {}   # (dtype) -> list of [tensor or None, event or None]
        self.next = {}

    def take(self, dtype, n):
        ring = self.slots.setdefault(dtype, [[None, None] for _ in range(self.SLOTS)])
        i = self.next.get(dtype, 0)
        self.next[dtype] = (i + 1) % self.SLOTS
        slot = ring[i]
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < n:
            slot[0] = torch.empty(max(2 * n, 4096), dtype=dtype, pin_memory=True)
        return slot

_PINNED = _PinnedRing()


def _pack(stage, host, offs):
    """Copy (and cast) the host tensors into their segments of `stage` -- through numpy, on THIS thread.  torch's copy_ splits
    anything above 32768 elements over the intra-op thread pool; under a container CPU quota the pool's spinning workers used the
    quota up and the whole process was throttled for the rest of the 100 ms scheduler period, every third step or so (round 4:
    90 ms stalls of the training loop, 3.2 -> 30 ms per step)."""
    flat = stage.numpy()
    for (_, v), o in zip(host, offs):
        flat[o:o + v.numel()] = v.detach().reshape(-1).numpy()


def stage_to_device(dev, dtype, tensors):
    """`tensors` as contiguous `dtype` tensors on `dev`.  Those that live on the host travel together: they are converted
    into one pinned staging buffer (16-byte aligned segments) and cross in ONE asynchronous copy, so the host never waits
    for the stream.  Tensors already on a device are converted in place."""
    vals = [torch.as_tensor(v) for v in tensors]
    out = [None] * len(vals)
    host = [(i, v) for i, v in enumerate(vals) if v.device.type == "cpu"]
    for i, v in enumerate(vals):
        if v.device.type != "cpu":
            out[i] = v.to(device=dev, dtype=dtype).contiguous()
    if host:
        offs, total = [], 0
        for _, v in host:
            offs.append(total)
            total += -(-v.numel() // 4) * 4
        total = max(total, 4)
        if os.environ.get("ARREAU_H2D", "pinned") == "pinned":
            slot = _PINNED.take(dtype, total)
            stage = slot[0]
            _pack(stage, host, offs)
            d = torch.empty(total, dtype=dtype, device=dev)
            d.copy_(stage[:total], non_blocking=True)
            ev = slot[1] if slot[1] is not None else torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            slot[1] = ev
        else:  # ARREAU_H2D=plain: one pageable copy (the host waits for the stream to drain)
            stage = torch.empty(total, dtype=dtype)
            _pack(stage, host, offs)
            d = stage.to(dev)
        for (i, v), o in zip(host, offs):
            out[i] = d[o:o + v.numel()].view(v.shape)
    return out


class DiffusionLossMetric:
    """diffusion_loss.py:52-65 (a torchmetrics.Metric there): running sum of the step losses and of the crystals seen,
    `compute()` = their ratio.  The two states are what a data-parallel run reduces over the ranks (`dist_reduce_fx="sum"`
    in the reference): `sync()` does those two scalar all-reduces.  States stay on the device of the losses they are fed,
    so updating the metric does not synchronise the training loop."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.total_loss = None
        self.total_samples = 0

    def update(self, loss, batch=None, num_crystals=None):
        loss = torch.as_tensor(loss).detach().sum()
        self.total_loss = loss.clone() if self.total_loss is None else self.total_loss + loss
        if num_crystals is None:
            if hasattr(batch, "num_atoms"):
                num_crystals = int(torch.as_tensor(batch.num_atoms).numel())
            else:  # the reference counts torch.unique(batch.batch)
                num_crystals = int(torch.unique(torch.as_tensor(batch.batch)).numel())
        self.total_samples += int(num_crystals)

    def sync(self, group=None):
        """Sum both states over the ranks of the default (or given) process group; a no-op without one."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        backend = dist.get_backend(group)
        dev = self.total_loss.device if (self.total_loss is not None and backend == "nccl") else torch.device("cpu")
        if backend == "nccl" and dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        tl = (self.total_loss if self.total_loss is not None else torch.zeros(())).to(dev, torch.float64).reshape(1)
        ts = torch.tensor([float(self.total_samples)], device=dev, dtype=torch.float64)
        dist.all_reduce(tl, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(ts, op=dist.ReduceOp.SUM, group=group)
        self.total_loss = tl.reshape(()).to(torch.float32)
        self.total_samples = int(round(float(ts)))
        return self

    def compute(self):
        if self.total_loss is None or self.total_samples == 0:
            return torch.tensor(float("nan"))
        return self.total_loss / self.total_samples


def state_to_device(state, dev):
    """(frac [N,3], types [N] i32, lengths [B,3], angles [B,3], offsets [B+1] i32, a zeroed cell buffer [B,3,3]) of an
    inversion.SamplerState as contiguous tensors on `dev`, float32 unless noted."""
    f32 = dict(device=dev, dtype=torch.float32)
    frac, lengths, angles = (torch.as_tensor(v).to(**f32).contiguous() for v in (state.frac_x, state.lengths, state.angles))
    types = torch.as_tensor(state.species).to(device=dev, dtype=torch.int32).contiguous()
    return frac, types, lengths, angles, crystal_offsets(torch.as_tensor(state.num_atoms), dev), torch.zeros((state.B, 3, 3), **f32)


@dataclass
class _RunBuffers:
    """The device buffers of one sample() call: the state the steps update in place, what holds parts of it, and the option
    tables and structs every call of the run takes."""
    frac_d: torch.Tensor
    types_d: torch.Tensor
    len_d: torch.Tensor
    ang_d: torch.Tensor
    off_d: torch.Tensor
    lattice_d: torch.Tensor
    clipmax: float
    const_d: Optional[torch.Tensor] = None
    tie_d: Optional[torch.Tensor] = None
    sym_d: Optional[dict] = None
    next_d: Optional[torch.Tensor] = None   # the Philox loop's next-timestep table of a schedule
    cond_d: Optional[dict] = None
    seeds_d: Optional[torch.Tensor] = None
    history: Optional[dict] = None          # multistep: empty at first, held through segments and a re-run
    guide: Optional[tuple] = None           # contact guidance: (parameters, the device arrays of its last evaluation)
    species_ctl: Optional[tuple] = None     # (rows, temperature); None (no set, temperature 1) keeps the exports used so far
    xguide: Optional[object] = None         # XRD guidance: the xrd_guidance.DeviceGuidance of the run (target, amplitudes, diagnostics)

    @classmethod
    def upload(cls, dev, plan, state, held, T, clipmax):
        frac_d, types_d, len_d, ang_d, off_d, lattice_d = state_to_device(state, dev)
        species_ctl = None
        if plan.allow_rows is not None or plan.species_temperature != 1.0:
            species_ctl = (species_mod.device_rows(plan.allow_rows, dev) if plan.allow_rows is not None else None,
                           plan.species_temperature)
        return cls(
            frac_d, types_d, len_d, ang_d, off_d, lattice_d, clipmax, const_d=types_d.clone() if held else None,
            tie_d=(torch.as_tensor(state.length_tie, device=dev, dtype=torch.int32).contiguous()
                   if state.length_tie is not None else None),
            sym_d=sym_mod.device_arrays(plan.specs, off_d, dev) if plan.specs is not None else None,
            next_d=respacing.next_table(T, plan.schedule).to(dev) if plan.schedule is not None and plan.noise == "philox" else None,
            history=multistep_mod.allocate_history(plan.N, plan.B, dev) if plan.multistep else None,
            guide=(plan.guidance, guidance_mod.allocate_info(plan.B, dev)) if plan.guidance is not None else None,
            species_ctl=species_ctl)

    def snapshot(self):
        return self.frac_d.clone(), self.types_d.clone(), self.len_d.clone()

    def restore(self, saved):
        self.frac_d.copy_(saved[0]); self.types_d.copy_(saved[1]); self.len_d.copy_(saved[2])
        if self.history is not None:
            multistep_mod.empty_history(self.history)  # the state changed outside a step


def _philox_driver(eng, plan, buf, seed, use_graph, frame):
    """The run as library loops (eng.sample_loop), cut after the steps whose state is a frame (plan.stops).  The noise is a
    function of (seed, timestep), so a run in segments is the same trajectory as a run in one call; a respaced segment starts at
    any scheduled timestep (respacing.next_table)."""
    fixed = buf.len_d.clone() if plan.fixed_cell else None
    start = 0
    for j in plan.stops + [None]:
        end = j + 1 if j is not None else len(plan.steps)
        if end > start:
            eng.sample_loop(buf.frac_d, buf.types_d, buf.len_d, buf.ang_d, buf.off_d, plan.steps[start], end - start, seed, buf.const_d,
                            buf.lattice_d, use_graph=bool(use_graph), fixed_lengths=fixed, condition=buf.cond_d, next_table=buf.next_d,
                            lattice_clipmax=buf.clipmax, corrector=plan.corrector, resampling=plan.resampling, length_tie=buf.tie_d,
                            symmetry=buf.sym_d, eta=plan.eta, multistep=buf.history, species=buf.species_ctl,
                            crystal_seeds=buf.seeds_d, guidance=buf.guide, **({"xrd_guidance": buf.xguide} if buf.xguide is not None else {}))
            start = end
        if j is not None:
            frame(f"_{plan.steps[j]}")


def _host_noise_driver(eng, plan, buf, seed, use_graph, frame):
    """The run as the events of resampling.plan on the host (noise 'device' and 'reference'; `seed` and `use_graph` belong to the
    Philox driver): per step the network evaluation, the corrector moves, each followed by a new evaluation, the three draws --
    lengths, positions, species -- and one predictor step; per jump its three draws and the jump."""
    B, N, S = plan.B, plan.N, plan.S
    f32 = dict(device=buf.frac_d.device, dtype=torch.float32)
    if plan.noise == "device":  # torch's device generator, in float32
        gauss, unif = (lambda *shape: torch.randn(shape, **f32)), (lambda *shape: torch.rand(shape, **f32))
    else:  # the global CPU generator in the default dtype, as the reference draws
        dt = torch.get_default_dtype()
        gauss, unif = (lambda *shape: torch.randn(shape, dtype=dt).to(**f32)), (lambda *shape: torch.rand(shape, dtype=dt).to(**f32))
    t_d = torch.empty(B, device=f32["device"], dtype=torch.int32)
    s_d = torch.empty(B, device=f32["device"], dtype=torch.int32)
    state = (buf.frac_d, buf.types_d, buf.len_d, buf.ang_d)
    corrector_steps, corrector_snr = plan.corrector or (0, None)

    def evaluate():  # the network at t_d on the current state; with guidance its eps is guided in place: contacts, then the pattern
        eps, logits, len0 = eng.predict_scores(*state, t_d, buf.off_d)
        if buf.guide is not None and buf.guide[0].weight > 0:
            eng.contact_guidance_step(buf.frac_d, lattice_from_params(buf.len_d, buf.ang_d), t_d, buf.off_d, eps, buf.guide)
        if buf.xguide is not None and buf.xguide.weight > 0:
            eng.xrd_guidance_step(buf.frac_d, buf.types_d, lattice_from_params(buf.len_d, buf.ang_d), t_d, buf.off_d, eps, buf.xguide)
        return eps, logits, len0
    for ev in plan.events:
        if ev.kind == "jump":  # resampling: the state back up to the block's top, in front of pass ev.r
            z_f, z_l, u_t = gauss(N, 3), gauss(B, 3), unif(N, S)
            s_d.fill_(ev.s)
            t_d.fill_(ev.t)
            eng.resample_jump(*state, s_d, t_d, buf.off_d, z_f, z_l, u_t, buf.lattice_d, const_types=buf.const_d, length_tie=buf.tie_d)
            continue
        t_d.fill_(ev.t)
        eps, logits, len0 = evaluate()
        for _ in range(corrector_steps):  # predictor-corrector: the moves at t, each followed by a new evaluation
            eng.corrector_step(buf.frac_d, t_d, buf.off_d, eps, gauss(N, 3), corrector_snr)
            eps, logits, len0 = evaluate()
        z_l, z_f, u_t = gauss(B, 3), gauss(N, 3), unif(N, S)
        eng.predictor_step(*state, t_d, s_d, buf.off_d, eps, logits, len0, z_l, z_f, u_t, buf.lattice_d, ev.s,
                           scheduled=plan.schedule is not None, length_tie=buf.tie_d, eta=plan.eta, multistep=buf.history,
                           species=buf.species_ctl, lattice_clipmax=buf.clipmax)
        if buf.const_d is not None:
            buf.types_d.copy_(buf.const_d)
        if ev.t != plan.t_first and sample_plan.frame_after(plan.visualization_setting, ev.t):
            frame(f"_{ev.t}")


class DiffusionLoss(nn.Module):
    def __init__(self, args, num_atomic_states: int):
        super().__init__()
        self.cutoff = args.radius
        self.max_neighbors = args.max_neighbors
        self.T = args.num_timesteps
        self.pos_diffusion = VE_pbc(self.T, sigma_min=pos_sigma_min, sigma_max=pos_sigma_max)
        self.d3pm = D3PM(x0_model=None, n_T=args.num_timesteps, num_classes=num_atomic_states, forward_type="mask")
        self.lattice_diffusion = VP_lattice(num_steps=self.T, power=lattice_power, clipmax=lattice_clipmax)
        self.num_atomic_states = num_atomic_states

    def __call__(self, model, batch, t_emb_weights=None, timestep=None, noise=None, return_parts=False,
                 training=False, seed=None, crystal_ids=None, copies=1, copy=None, rows=None, row_index=None):
        """diffusion_loss.py:204-274: sample a timestep per crystal, noise (coordinates, atom types, cell lengths),
        evaluate the score network on the noised batch and return `coord + atom-type + lattice` error (weights 1).

        `batch` carries X0 [N,3] fractional coordinates, A0 [N] class indices, L0 [B*3,3] or [B,3,3] cells and
        num_atoms [B] (the fields of the reference's PyG `Data`, lattice_dataset.py:96-104).  Random draws follow the
        reference's order: randint(1, T+1) [B,1] unless `timestep` is given (:213-221), randn_like(X0) (VE_pbc.forward),
        rand(N,S) (D3PM.get_xt), randn_like(lengths) (VP_lattice.forward), from torch's global CPU generator;
        `noise=(z_frac, u_types, z_lengths)` injects them instead (parity tests).  Everything else runs in
        libarreau_hip.so (arreau_diffusion_noise -> arreau_predict_scores -> arreau_diffusion_losses).

        `noise="philox"` is the keyed path (arreau_diffusion_noise_keyed; rules in include/arreau_hip.h): nothing is drawn on the
        host and nothing but the clean batch and the ids is staged.  The timestep and the three draws of crystal b come from
        Philox keyed by (`seed`, crystal_ids[b]) -- `crystal_ids` [B] integers below 2^32, default batch.index (collate's dataset
        indices) -- so a crystal is noised the same way wherever it lands in a batch.  `copies` = R and `copy` [B] (default 0): R
        noisings of every crystal at stratified timesteps.  A given `timestep` replaces the drawn one.
        `rows` / `row_index` (any noise mode): also write every crystal's loss row into the caller's table
        (HipEngine.loss_row_table; arreau_diffusion_loss_rows) at row_index[b].

        `training=True` evaluates the network with arreau_train_forward (fp32, activations kept) instead of the fused
        sampling kernels, so that HipEngine.train_backward can follow.

        Returns the scalar loss (a 0-d float32 CUDA tensor); with return_parts=True also a dict of the three errors,
        the noised inputs, the network outputs and d(loss)/d(outputs)."""
        eng = model.engine(for_training=training)
        dev = eng.device
        S = self.num_atomic_states
        n_cpu = torch.as_tensor(batch.num_atoms).to("cpu", torch.int64)
        B, N = int(n_cpu.numel()), int(n_cpu.sum())
        frac0 = torch.as_tensor(batch.X0)
        if frac0.shape != (N, 3):
            raise ValueError("batch.X0 must be [sum(num_atoms), 3]")
        keyed = isinstance(noise, str)
        if keyed:
            if noise != "philox":
                raise ValueError("noise must be None (host draws), a tuple of draws or 'philox' (keyed draws in the kernels)")
            if seed is None:
                raise ValueError("noise='philox' needs a seed")
            ids = torch.as_tensor(batch.index if crystal_ids is None else crystal_ids).to("cpu", torch.int64).reshape(-1)
            if ids.numel() != B or (B and (int(ids.min()) < 0 or int(ids.max()) >= 2 ** 32)):
                raise ValueError("crystal_ids must hold one id in 0..2^32-1 per crystal")
            copies = int(copies)
            if not 1 <= copies <= self.T:
                raise ValueError(f"copies must lie in 1..{self.T}")
            copy_h = None
            if copy is not None:
                copy_h = torch.as_tensor(copy).to("cpu", torch.int64).reshape(-1)
                if copy_h.numel() != B or int(copy_h.min()) < 0 or int(copy_h.max()) >= copies:
                    raise ValueError("copy must hold one value in 0..copies-1 per crystal")
        elif seed is not None or crystal_ids is not None or copy is not None or copies != 1:
            raise ValueError("seed, crystal_ids, copies and copy belong to noise='philox'")
        if timestep is None:
            t = None if keyed else torch.randint(1, self.T + 1, size=(B, 1)).long()
        elif torch.is_tensor(timestep) and timestep.numel() == B:
            t = timestep.reshape(B, 1).long().cpu()
        else:
            t = torch.ones((B, 1)).long() * int(timestep)
        if t is not None and (int(t.min()) < 1 or int(t.max()) > self.T):
            raise ValueError(f"timestep must be in 1..{self.T}")
        if keyed:
            z_frac = u_types = z_len = None  # drawn in the kernels
        elif noise is None:
            dt = torch.get_default_dtype()
            z_frac = torch.randn((N, 3), dtype=dt)
            u_types = torch.rand((N, S))
            z_len = torch.randn((B, 3), dtype=dt)
        else:
            z_frac, u_types, z_len = noise
        # Host -> device: ONE pinned staging buffer and one asynchronous copy per element type.  Eight pageable .to(device)
        # copies each block the host until the stream has drained, so the device idled while the host prepared and
        # enqueued the next step (round 4, rocprofv3 kernel trace of the training step: 0.25 ms of 3.2 without the profiler).
        off_host = torch.zeros(B + 1, dtype=torch.int64)
        off_host[1:] = torch.cumsum(n_cpu, 0)
        row_d = None
        if keyed:
            frac_d, cell_d = stage_to_device(dev, torch.float32, [frac0, torch.as_tensor(batch.L0).reshape(-1, 3, 3)])
            ints = [batch.A0, off_host] + ([t.reshape(B)] if t is not None else []) + ([copy_h] if copy_h is not None else [])
            ints = stage_to_device(dev, torch.int32, ints)
            types0, off = ints[0], ints[1]
            longs = stage_to_device(dev, torch.int64, [ids] + ([torch.as_tensor(row_index).reshape(B)] if rows is not None else []))
            nz = eng.diffusion_noise_keyed(frac_d, types0, cell_d, off, seed, longs[0], copies,
                                           ints[-1] if copy_h is not None else None, ints[2] if t is not None else None)
            t_d = nz.pop("t")
            row_d = longs[1] if rows is not None else None
        else:
            frac_d, cell_d, z_frac_d, u_types_d, z_len_d = stage_to_device(
                dev, torch.float32, [frac0, torch.as_tensor(batch.L0).reshape(-1, 3, 3), z_frac, u_types, z_len])
            t_d, types0, off = stage_to_device(dev, torch.int32, [t.reshape(B), batch.A0, off_host])
            nz = eng.diffusion_noise(frac_d, types0, cell_d, t_d, off, z_frac_d, u_types_d, z_len_d)
            if rows is not None:
                row_d, = stage_to_device(dev, torch.int64, [torch.as_tensor(row_index).reshape(B)])
        evaluate = eng.train_forward if training else eng.predict_scores
        run = lambda: evaluate(nz["noisy_frac"], nz["noisy_types"], nz["noisy_lengths"], nz["angles"], t_d, off)
        # (validation: sticky device flags -> raise; non-finite outputs with fp8 operand planes in use -> repeated on fp16 planes: HipEngine.checked.
        # Reading the flags synchronises the stream, so the training step -- whose host work overlaps the device's, and whose
        # forward runs no fp8 product -- leaves that to PONITA_DIFFUSION.training_step, every STATUS_CHECK_EVERY steps.)
        eps, logits, len0 = run() if training else eng.checked(run)
        if rows is not None:
            losses, grads, _ = eng.diffusion_loss_rows(eps, nz["target_eps"], logits, types0, nz["noisy_types"], t_d, len0,
                                                       nz["lengths"], off, row_d, rows, with_grads=True)
        else:
            losses, grads = eng.diffusion_losses(eps, nz["target_eps"], logits, types0, nz["noisy_types"], t_d, len0,
                                                 nz["lengths"], off, with_grads=True)
        if return_parts:
            return losses[0], dict(error_frac_x=losses[1], error_atomic_type=losses[2], error_lattice=losses[3],
                                   vb=losses[4], ce=losses[5], pred_eps=eps, logits=logits, pred_lengths=len0,
                                   grad_eps=grads[0], grad_logits=grads[1], grad_lengths=grads[2], timestep=t_d, **nz)
        return losses[0]

    # ------------------------------------------------------------------------------------------
    def predict_scores(self, noisy_frac_x, noisy_atom_types, t_feat, num_atoms, noisy_lengths, angles, model,
                       batch=None, t_emb_weights=None, edges=None):
        """diffusion_loss.py:112-197.  `noisy_atom_types` may be class indices [N] or one-hot [N,S]
        (the reference passes the one-hot); `t_feat` is the per-atom timestep [N] (or per-crystal [B]).
        Returns (pred_frac_eps_x [N,3], logits [N,S], pred_lengths_0 [B,3]) on the GPU."""
        eng = model.engine()
        dev = eng.device
        frac = noisy_frac_x.to(device=dev, dtype=torch.float32).contiguous()
        ty = noisy_atom_types
        if ty.dim() == 2:
            ty = ty.argmax(dim=1)
        ty = ty.to(device=dev, dtype=torch.int32).contiguous()
        lengths = noisy_lengths.to(device=dev, dtype=torch.float32).contiguous()
        ang = angles.to(device=dev, dtype=torch.float32).contiguous()
        n_cpu = torch.as_tensor(num_atoms).to("cpu", torch.int64)
        off = crystal_offsets(n_cpu, dev)
        t_feat = torch.as_tensor(t_feat)
        if t_feat.numel() == n_cpu.numel():
            t_c = t_feat.reshape(-1)
        else:  # per-atom timestep: constant inside a crystal, take each crystal's first atom
            first = (torch.cumsum(n_cpu, 0) - n_cpu).clamp(max=max(int(t_feat.numel()) - 1, 0))
            t_c = t_feat.reshape(-1).to("cpu")[first]
        t_c = t_c.to(device=dev, dtype=torch.int32).contiguous()
        return eng.predict_scores(frac, ty, lengths, ang, t_c, off, edges=edges)

    _atom_counts = staticmethod(sample_plan.atom_counts)

    def draw_initial_state(self, num_atoms_per_sample, num_samples_in_batch, num_atomic_states=None, constant_atoms=None,
                           lattice_system=None, condition=None, specs=None, seed=None, crystal_keys=None,
                           model=None) -> inversion.SamplerState:
        """The host draw of sample(): the state at level T-1 a run starts from, as an inversion.SamplerState.  The reference's
        generators in the reference's order: numpy's global generator for the angles (lattice_systems.resolve), then torch's
        global CPU generator for randn lengths [B,3] and randn fractional coordinates [N,3] * pos_sigma_max.  Species: the mask
        class S - 1, or constant_atoms.  lattice_system ties the lengths (the codes travel in the state); a condition's known
        cells give their angles (its other known components are imposed on the device, by sample()); `specs` (the resolved
        symmetry specs of sample()) project the leaders onto their sites.  Handing the result to sample(initial_state=...) under
        the generator states this call left is the plain sample() call bit for bit.
        `seed`, `crystal_keys` (keyed sampling; rules in keyed.py): the draws of crystal b come from its own stream instead -- the
        uniforms of its angle draw restated on the host (kind 15), the normals of its lengths and positions written out by the
        device (kinds 13 and 14; `model` gives the engine) -- and the formulas below are applied to them as to the generators'
        values.  The global generators are neither read nor advanced."""
        B = int(num_samples_in_batch)
        streams = None
        if crystal_keys is not None:
            streams = keyed_mod.stream_seeds(seed, keyed_mod.validate_keys(crystal_keys, B, seed))
            if model is None:
                raise ValueError("draw_initial_state: keyed draws need model= (the normals are drawn on the device)")
        S = int(self.num_atomic_states if num_atomic_states is None else num_atomic_states)
        num_atoms = self._atom_counts(num_atoms_per_sample, B)
        N = int(num_atoms.sum())
        dt = torch.get_default_dtype()
        # the angles per crystal (numpy's generator; lattice_system=None: the monoclinic draw in degrees, as the reference)
        angles_np, tie = lattice_systems.resolve(lattice_system, B, condition.lattice_known() if condition is not None else None,
                                                 uniforms=[keyed_mod.angle_uniforms(int(s)) for s in streams] if streams is not None else None)
        angles = torch.tensor(angles_np)
        if condition is not None and condition.lattice_known().any():  # rule 3: the template's angles (radians)
            known = torch.as_tensor(condition.lattice_known())
            angles[known] = torch.as_tensor(condition.known_angles(), dtype=angles.dtype)[known]
        if streams is not None:
            eng = model.engine()
            z_len, z_frac = eng.keyed_initial_draws(keyed_mod.device_seeds(streams, eng.device), crystal_offsets(num_atoms, eng.device))
            lengths = z_len.cpu().to(dt)
        else:
            lengths = torch.randn([B, 3])
        if tie is not None:
            lattice_systems.tie_lengths(lengths, tie)  # the initial state's tie; the device keeps it at every step
        frac_x = (z_frac.cpu().to(dt) if streams is not None else torch.randn([N, 3], dtype=dt)) * pos_sigma_max
        if specs is not None:  # leaders onto their sites, members their images (unwrapped, as the draw)
            fx = frac_x.double().numpy()
            first = np.concatenate([[0], np.cumsum(num_atoms.numpy())])
            for b, s_b in enumerate(specs):
                if s_b is not None:
                    fx[first[b]:first[b + 1]] = s_b.initial_positions(fx[first[b]:first[b + 1]])
            frac_x = torch.as_tensor(fx).to(dt)
        if constant_atoms is not None:
            atom_types = torch.as_tensor(constant_atoms).reshape(-1).long()
            if atom_types.numel() != N:
                raise ValueError("constant_atoms must hold one class index per atom")
        else:
            atom_types = torch.full((N,), S - 1)
        return inversion.SamplerState(frac_x=frac_x.numpy(), species=atom_types.numpy(), lengths=lengths.numpy(),
                                      angles=angles.numpy(), num_atoms=num_atoms.numpy(), t=self.T - 1, length_tie=tie)

    @torch.no_grad()
    def sample(self, *, model, z_table: AtomicNumberTable, t_emb_weights=None, num_atoms_per_sample=None,
               num_samples_in_batch: Optional[int] = None, vis_name: str = "", visualization_setting=VisualizationSetting.NONE,
               show_bonds: bool = False, constant_atoms: Optional[torch.Tensor] = None, noise: str = "philox",
               max_steps: Optional[int] = None, use_graph: Optional[bool] = None, seed: Optional[int] = None,
               fixed_cell: bool = False, condition=None, num_steps: Optional[int] = None,
               timesteps: Optional[Sequence[int]] = None, corrector_steps: int = 0,
               corrector_snr: float = pc.DEFAULT_SNR, resample_passes: int = 1, jump_length: int = 10,
               lattice_system=None, symmetry=None, screen=None, unique=None, find_symmetry=None, reduce_cell=None,
               symmetrize=None, match_to=None, eta: Optional[float] = None, initial_state=None,
               multistep: bool = False, elements=None, species_temperature: float = 1.0, crystal_keys=None,
               conventional_cell=None, coordination=None, bond_order=None, contact_guidance=None, voronoi=None, xrd=None,
               xrd_guidance=None, ewald=None) -> SampleResult:
        """diffusion_loss.py:276-377.  The initial state is drawn on the host exactly like the reference (numpy
        uniforms for the angles, then randn lengths, randn fractional coordinates from torch's global CPU generator):
        draw_initial_state, which a caller may also use on its own.
        Per-step noise:
          noise="philox" (default): the whole loop is ONE library call (arreau_sample_loop): the three draws of a step are
              generated inside the update kernels from Philox4x32-10 keyed by (seed, timestep, draw, element), the
              timestep lives on the device, nothing happens on the host between steps.  `seed` defaults to a draw from
              torch's global CPU generator (so torch.manual_seed makes runs repeatable).  `use_graph=True` replays one
              captured step as a hipGraph (same trajectory bit for bit; measured on MI355X: 1.70 vs 1.765 ms per step at
              256 x 20, nothing at 1 x 8 where the step is the sum of its kernels' durations; default: on for runs of at
              least 200 steps, which amortise the capture).
          noise="reference": randn[B,3], randn[N,3], rand[N,S] from the global CPU generator in the reference's order
              (diffusion_helpers.py:193-197, :79; d3pm.py:206), uploaded every step -- the parity mode.
          noise="device": the same loop with torch's device generator (three RNG launches per step).
        visualization_setting: LAST writes the final state, ALL every 10th timestep + final, ALL_DETAILED every timestep + final
        (the reference's schedule, diffusion_loss.py:351-370), as `<vis_name>_<timestep>.cif` / `<vis_name>_final.cif`
        structure files (inference/visualize_crystal.py; the reference renders PNGs through plotly + pymatgen).
        `fixed_cell=True` (extension, noise="philox" only): fixed-cell sampling -- the initial cell lengths are re-imposed
        after every step (arreau_sample_loop's d_fixed_lengths); coordinates and species are sampled as usual.
        `condition` (extension, noise="philox" only): a conditioning.SampleCondition -- known positions, species and cells held
        to a template while the rest is generated (arreau_sample_loop_conditioned; rules in include/arreau_hip.h).  It defines
        the batch: num_atoms_per_sample / num_samples_in_batch may be omitted or must agree with it.  The initial state is
        drawn exactly as without it; the known components are then overwritten on the device.
        `num_steps` / `timesteps` (extension, every noise mode; mutually exclusive): respaced sampling -- the loop visits only
        the timesteps of a schedule (respacing.respaced_timesteps(T, num_steps), evenly spaced, or an explicit strictly
        descending list from at most T-1 down to 1) and jumps from each to the next in closed form (rules in
        include/arreau_hip.h; arreau_sample_loop_scheduled / arreau_reverse_step_to).  The step at a visited timestep draws
        what a full run draws there.  `max_steps` keeps the schedule's first max_steps steps; frames follow the schedule
        (ALL: the visited multiples of 10, ALL_DETAILED: every visited timestep).  The full schedule T-1, ..., 1 given
        explicitly is the plain loop bit for bit.  No claim on sample quality at a given number of steps is made.
        `corrector_steps` / `corrector_snr` (extension, every noise mode): predictor-corrector sampling -- M = corrector_steps
        (0..16) Langevin moves on the positions at every visited timestep before its predictor step, each after a network
        evaluation, with the SNR step-size rule r = corrector_snr (rules in include/arreau_hip.h; arreau_sample_loop_corrected).
        philox: the moves run in the library loop, their noise is Philox kind 5; reference / device: arreau_corrector_step
        with randn[N,3] from that mode's generator, drawn per move before the step's three predictor draws.  M = 0 is the
        sampler without correctors bit for bit (and draws nothing extra).  No sample-quality claim is made.
        `resample_passes` / `jump_length` (extension, every noise mode): RePaint resampling -- the visited steps (after
        `max_steps` has cut them) in blocks of J = jump_length, every block run R = resample_passes (1..64) times, and every pass
        after the first starts with a forward jump of the whole state from the block's bottom back up to its top (rules in
        include/arreau_hip.h; arreau_sample_loop_resampled).  philox: the blocks run in the library loop; reference / device: the
        events of resampling.plan on the host, each jump (arreau_resample_jump) drawing randn[N,3], randn[B,3], rand[N,S] from
        that mode's generator just before the pass it precedes.  R = 1 is the sampler without resampling bit for bit (and draws
        nothing extra).  With R > 1 only visualization_setting NONE or LAST is accepted (a frame inside a block would be
        overwritten by the next pass).  No sample-quality claim is made.
        `lattice_system` (extension, every noise mode): crystals of a chosen lattice system -- one of lattice_systems.SYSTEMS for
        every crystal, or a sequence with one name (or None) per crystal.  A crystal of a system gets the system's angles in
        radians (np.deg2rad of sample_bravais_angles) and its tied lengths (a = b, or a = b = c) are kept bitwise equal at every
        step on the device (arreau_sample_loop_tied; rules in include/arreau_hip.h), the initial lengths tied on the host.
        None keeps the sampler as it was, bit for bit: monoclinic angles drawn in DEGREES and read as radians, the reference's
        own behaviour -- so None and "monoclinic" differ.  A system on a crystal whose cell a condition knows is rejected.  No
        sample-quality claim is made.
        `symmetry` (extension, noise="philox" only): space-group symmetry -- a symmetry.SymmetrySpec for every crystal of the batch
        (num_samples_in_batch needed), or a sequence with one spec (or None, unconstrained) per crystal.  A constrained crystal's
        atoms sit in the Wyckoff orbits of the spec's group at every step: the leader of each orbit is updated from the orbit's
        pulled-back mean position noise and projected onto its site, the members are its images, and the orbit shares the
        species the leader draws from the orbit's mean logits (arreau_sample_loop_sym; rules in include/arreau_hip.h).  The specs
        decide the atom counts and lattice systems: num_atoms_per_sample and lattice_system, if given, must agree with them (and
        give those of the None crystals).  The initial positions are drawn as without it, then every leader is projected onto
        its site (anchored at the template's leader) and the members expanded, unwrapped.  Constant species must be constant
        per orbit.  Works with graph replay, respaced schedules, fixed cells, max_steps and frames; a condition, corrector steps,
        resampling and the host-noise modes are rejected.  None, or a sequence of None only, is the sampler as it was.  No
        sample-quality claim is made.
        `eta` (extension, every noise mode): DDIM-style sampling (Song, Meng & Ermon 2021) -- a float in [0, 1] that scales the
        noise every step injects into positions and lengths (ddim.py; rules in include/arreau_hip.h; arreau_sample_loop_eta /
        arreau_reverse_step_eta): 1 is the ancestral step (up to rounding, and to the clip of the lengths' beta), 0 injects none,
        so positions and lengths become a function of the initial state alone, whatever the seed.  The species keep the D3PM
        step with its Gumbel draw: they are deterministic only where they are held (constant_atoms, a condition's known
        species) or with species_temperature=0, which removes the draw.  The draws keep their keys; at eta = 0 those of positions and lengths are not read (the host-noise modes
        still draw them, so their generators advance as always).  Works with schedules, conditions, corrector steps, resampling
        (its jumps are unchanged), fixed cells, lattice systems, graph replay and frames; with `symmetry` it is rejected.  None
        is the sampler as it was, bit for bit.  No sample-quality claim is made.
        `initial_state` (extension, every noise mode): an inversion.SamplerState -- what PONITA_DIFFUSION.noise_to (known crystals
        forward-noised to a level), PONITA_DIFFUSION.encode (DDIM inversion) and draw_initial_state (the draw this method makes
        itself) return.  Positions, species, lengths, angles, atom counts and the lattice-system tie come from the state and
        nothing is drawn for them; the loop enters at the state's level t (1..T-1) instead of T-1: num_steps is resolved with
        top = t (respacing), an explicit `timesteps` must start at t, and without either every timestep t, t-1, ..., 1 is
        visited.  Everything after that is the sampler as it is, in every noise mode: eta, correctors, resampling, fixed_cell
        (the state's lengths are held), max_steps, frames and the instruments.  constant_atoms: True holds the state's species; a
        tensor of class indices replaces and holds them.  The state defines the batch: num_atoms_per_sample /
        num_samples_in_batch may be omitted or must agree with it.  Rejected before any work: a state together with `condition`,
        `symmetry` or `lattice_system`, a level outside 1..T-1, a batch that disagrees.  With the state draw_initial_state returns
        under the same generator states the run is the plain one bit for bit; None is the sampler as it was.  No claim on
        reconstruction or sample quality is made.
        `multistep` (extension, every noise mode): second-order multistep sampling (DPM-Solver++ 2M, Lu et al. 2022; multistep.py;
        rules in include/arreau_hip.h; arreau_sample_loop_multistep / arreau_reverse_step_multistep) -- the deterministic eta = 0
        step of positions and lengths, extrapolated with the previous step's prediction (in log sigma and in log-SNR time), at the
        same one network evaluation per step; a move whose step-size ratio leaves [1/3, 3], the first move and the last are first
        order.  The species keep the D3PM step with its draw (species_temperature=0 removes it).  The history lives in four device buffers this call allocates and
        holds through segments (frames) and a re-run.  Works with schedules, lattice systems, fixed cells, constant_atoms,
        initial_state, max_steps, frames, graph replay and the instruments; rejected before any work with `condition`, corrector
        steps, resampling passes > 1, `symmetry` and an eta other than None or 0.  False is the sampler as it was, bit for bit.
        No sample-quality claim is made.
        `elements`, `species_temperature` (extension, every noise mode): species control (species.py; rules in
        include/arreau_hip.h; arreau_sample_loop_species / arreau_reverse_step_species).  `elements` restricts the classes the D3PM
        species step may choose: one collection of element symbols and / or atomic numbers for the whole batch, or a list with one
        entry per crystal, an entry being such a collection or None (unrestricted).  A restricted crystal ends with elements of its
        set only and never with the mask state; an excluded class has probability exactly 0 in every step.
        `species_temperature` >= 0 scales the Gumbel term of the species draw: 1 is the step as it is, 0 takes the arg-max of the
        posterior and draws nothing, so sample(eta=0, species_temperature=0) and multistep runs are functions of the initial state
        in positions, lengths and species.  Both combine with every option above, space-group symmetry included (an orbit draws
        one admitted class).  Rejected before any work: an unknown symbol, an element the table does not hold, an empty set, a list
        of the wrong length, a temperature that is negative or not finite, a held species (constant_atoms, a condition's known
        species) outside its crystal's set.  A given initial_state whose species lie outside is accepted: every sampled atom
        leaves its first step inside.  None and 1.0 are the sampler as it was, bit for bit, through the exports it used.  No
        sample-quality claim is made.
        `screen` (extension, every noise mode and option): a screening.ScreenCriteria, or True for its defaults -- the final
        device state is screened in one launch before it is copied back (arreau_crystal_screen; rules in include/arreau_hip.h):
        shortest contact over all periodic images, cell volume, number density, mask state.  SampleResult.metrics then holds the
        six arrays and `valid`.  A criteria without a mask_type checks for the D3PM mask state S - 1, or for none when
        constant_atoms is given.  None: no launch is added, metrics is None and the results are what they were, bit for bit.
        `unique` (extension, every noise mode and option): a uniqueness.FingerprintParams, or True for its defaults -- two more
        launches on the final device state (arreau_crystal_fingerprint, arreau_fingerprint_match) give every crystal a structure
        fingerprint and the earliest crystal of the batch it duplicates; the class indices are the species ids.
        SampleResult.uniqueness then holds duplicate_of, distance, nearest, nearest_distance, flags and unique.  None: no launch
        is added and uniqueness is None.
        `find_symmetry` (extension, every noise mode and option): a symmetry_search.SymmetrySearchParams, or True for its
        defaults -- one more launch on the final device state (arreau_crystal_symmetry; rules in include/arreau_hip.h) finds the
        operations x' = W x + t every crystal has in its cell and the point group of their rotations; the class indices are the
        species ids.  SampleResult.symmetry then holds the arrays (symmetry_search.contains / stats_of read them).  No space-group
        number, no standardised cell.  None: no launch is added, symmetry is None and the results are what they were, bit for bit.
        `reduce_cell` (extension, every noise mode and option): a cell_reduction.CellReductionParams, or True for its defaults --
        one more launch on the final device state (arreau_crystal_reduce; rules in include/arreau_hip.h) finds every crystal's pure
        translations, its primitive cell, a Delaunay-reduced basis of it and the atoms in that basis.  SampleResult.reduced then
        holds the arrays (cell_reduction.REDUCED_KEYS); frac_x, lattice and every other field stay in the cell as sampled, and
        screen, unique and find_symmetry still read that cell.  No Niggli form, no standardised setting.  None: no launch is added,
        reduced is None and the results are what they were, bit for bit.
        `symmetrize` (extension, every noise mode and option): a symmetrize.SymmetrizeParams (the symmetry search's symprec and
        max_ops), or True for its defaults -- the search's launch (shared with `find_symmetry` when both are given: their
        parameters must then agree) and one more on the final device state (arreau_crystal_symmetrize; rules in
        include/arreau_hip.h) move every crystal's atoms onto sites its found operations map onto each other exactly, average
        its metric over their rotations and report its orbits.  SampleResult.symmetrized then holds the arrays
        (symmetrize.SYMMETRIZED_KEYS); frac_x, lattice and every other field stay as sampled, and screen, unique, find_symmetry and
        reduce_cell still read that state.  No space-group number, no origin search, no standard setting.  None: no launch is
        added, symmetrized is None and the results are what they were, bit for bit.
        `match_to` (extension, every noise mode and option): targets to match the final state against -- a SampleResult, a loaded
        crystals file, or (targets, structure_match.StructureMatchParams) -- in one more launch (arreau_structure_match; rules in
        include/arreau_hip.h): per crystal the change of basis, the translation and the atom-to-atom map under which a target
        falls onto it, the rms displacement in A and normalised, and `matched` (rms_norm <= stol).  As many targets as crystals:
        crystal b is matched against target b; otherwise against every target of its composition, the best one reported.  The
        atomic numbers are the species ids.  SampleResult.match then holds the arrays (structure_match.MATCH_KEYS).  It reads the
        state as sampled, like the other instruments.  The optimal assignment only with StructureMatchParams(assignment="optimal"), no supercells, no volume scaling.  None: no launch
        is added, match is None and the results are what they were, bit for bit.
        `conventional_cell` (extension, every noise mode and option): a conventional_cell.ConventionalCellParams (the symmetry
        search's symprec and max_ops), or True for its defaults -- on the final device state the reduction's launch (shared with
        `reduce_cell` when both are given: their symprec must then agree, as must find_symmetry's and symmetrize's parameters), the
        symmetry search on the REDUCED batch and one more launch (arreau_crystal_conventional; rules in include/arreau_hip.h) give
        every crystal its conventional cell with the atoms in it, the centring, the Bravais lattice (aP .. cF) and, through
        conventional_cell.pearson_symbol, the Pearson symbol.  SampleResult.conventional then holds the arrays
        (conventional_cell.CONVENTIONAL_KEYS); frac_x, lattice and every other field stay as sampled, and the other instruments still
        read that state.  No space-group number, no origin shift, no idealised metric.  None: no launch is added, conventional is
        None and the results are what they were, bit for bit.
        `crystal_keys` (extension, noise="philox" with a `seed`): keyed sampling (keyed.py; rules in include/arreau_hip.h;
        arreau_sample_loop_keyed) -- one integer key in 0..2^63-1 per crystal, no key twice.  Every random number crystal b consumes
        -- its initial angles, lengths and positions, every draw of every step, corrector move and jump, the known components of a
        condition -- comes from a stream of its own derived from (seed, crystal_keys[b]), with elements counted inside the
        crystal.  Its final state is then a function of (model, options, seed, key, its atom count, its own inputs): within one
        score arithmetic bitwise the same alone, in any batch, at any index, eager or replayed, in one call or in segments.
        Limits: batches on different sides of the score network's basis-form threshold, or with and without ARREAU_CROSS_FP8, agree
        only to the bound of the network's batch-independence test; the re-run after an fp16x3 overflow is decided per batch.  The
        host's global generators are neither read nor advanced.  With every option above.  Rejected before any work: keys without
        a seed, with a host-noise mode, out of range, of the wrong count, a key twice.  SampleResult.crystal_keys carries the keys.
        None is the sampler as it was, bit for bit, through the exports it used.
        `coordination` (extension, every noise mode and option): a coordination.CoordinationParams (tol, cutoff, max_neighbors,
        max_shells), or True for its defaults -- one more launch on the final device state (arreau_crystal_coordination; rules in
        include/arreau_hip.h) gives every atom its neighbours -- all atoms and images within (1 + tol) times its nearest distance
        and within the cutoff --, its coordination number and nearest distance, and every crystal their sums and extremes.
        SampleResult.coordination then holds the arrays (coordination.STORED_KEYS).  It reads the state as sampled.  No Voronoi
        weighting (not the reference's CrystalNN), no radii, no chemistry.  A bad value is rejected before any work.  None: no
        launch is added, coordination is None and the results are what they were, bit for bit.
        `bond_order` (extension, every noise mode and option): a bond_order.BondOrderParams (the coordination search's tol, cutoff,
        max_neighbors, max_shells), or True for its defaults -- the coordination launch and one more on its neighbour lists
        (arreau_crystal_bond_order; rules in include/arreau_hip.h) give every atom the histogram of the angles between its bonds
        (37 bins centred on 0, 5, ..., 180 degrees) and the Steinhardt order parameters q_2, q_4, q_6, q_8 of its shell, and every
        crystal the summed histogram and the mean q_l.  SampleResult.bond_order then holds the arrays (bond_order.STORED_KEYS).
        With `coordination` too the coordination launch is shared: their parameters must then agree (ValueError before any work).
        It reads the state as sampled.  No w_l, no neighbour-averaged parameters, no classification of environments, no Voronoi
        weights.  None: no launch is added, bond_order is None and the results are what they were, bit for bit.
        `voronoi` (extension, every noise mode and option): a voronoi.VoronoiParams (tol, cutoff, max_faces, max_candidates,
        max_shells), or True for its defaults -- one more launch on the final device state (arreau_crystal_voronoi; rules in
        include/arreau_hip.h) builds every atom's Voronoi cell over every periodic image: the neighbours behind its faces, each
        with its solid angle, area and distance and its weight (solid angle over the atom's largest), the number of faces of
        weight >= tol, the cell's volume, and the OPEN flag where the cutoff does not close the cell.  SampleResult.voronoi then
        holds the arrays (voronoi.STORED_KEYS).  It reads the state as sampled.  Not CrystalNN: no radii, no electronegativities,
        no distance weighting, no probabilities.  None: no launch is added, voronoi is None and the results are what they were,
        bit for bit.
        `xrd` (extension, every noise mode and option): an xrd.XrdParams (wavelength, two_theta_min, two_theta_max, n_points, fwhm,
        b_iso, scattering, max_index), or True for its defaults -- one more launch on the final device state (arreau_crystal_xrd;
        rules in include/arreau_hip.h) writes every crystal's powder X-ray diffraction pattern on a fixed 2 theta grid: Z-weighted
        point scatterers, Lorentz-polarisation factor, Gaussians of one width.  SampleResult.xrd then holds the arrays
        (xrd.STORED_KEYS).  It reads the state as sampled.  No form-factor tables, no anomalous dispersion, no peak list, no K
        alpha 2.  None: no launch is added, xrd is None and the results are what they were, bit for bit.
        `ewald` (extension, every noise mode and option): an ewald.EwaldParams(charges={"Na": 1, "Cl": -1} or "Na=1,Cl=-1",
        accuracy, alpha, max_shells, max_index) -- one more launch on the final device state (arreau_crystal_ewald; rules in
        include/arreau_hip.h) writes every crystal's Ewald energy of those point charges, its four parts and every atom's site
        potential.  SampleResult.ewald then holds the arrays (ewald.STORED_KEYS).  A crystal with a species that has no charge
        (the mask state included) is flagged UNASSIGNED, one that is not neutral CHARGED (a neutralising background is in its
        number).  It reads the state as sampled.  No forces, no guidance, no oxidation-state guessing, no short-range repulsion.
        There are no default charges: True is rejected.  None: no launch is added, ewald is None and the results are what they
        were, bit for bit.
        `contact_guidance` (extension, every noise mode and option): a contact_guidance.ContactGuidance (min_distance, weight,
        max_shells), or True for its defaults -- training-free guidance away from short contacts (rules in include/arreau_hip.h,
        "contact guidance"; arreau_sample_loop_guided).  Every network evaluation of every step, a corrector's included, is followed
        by one launch that finds every pair of atoms and periodic image closer than min_distance (the screen's exact search) and
        adds the gradient of U = 1/2 sum 1/2 (min_distance - d)^2, preconditioned by the cell and scaled by weight / sigma_t^2, to
        the predicted eps: the step's clean-structure estimate moves `weight` times the overlap apart (0.5 resolves an isolated
        contact).  noise="philox" runs it inside the loop, graph replay included; noise="device" and "reference" run the same
        launch between the evaluation and the step (arreau_contact_guidance_step).  SampleResult.info["contact_guidance"] holds
        the last evaluation's energy, contacts and flags per crystal (contact_guidance.INFO_KEYS).  Positions only: no cell-strain
        term, no radii or species dependence, no weight schedule other than 1 / sigma_t^2; no claim on sample quality.  A bad
        value is rejected before any work.  weight = 0 and None: no launch is added and the results are what they were, bit for
        bit (None also through the exports it used).
        `xrd_guidance` (extension, every noise mode and option): an xrd_guidance.XrdGuidance(target, weight=2.0, params=XrdParams())
        -- training-free guidance of the positions towards a target powder pattern (rules in include/arreau_hip.h, "XRD guidance";
        arreau_sample_loop_xrd_guided): structure solution from a powder pattern with the cell given (fixed_cell, a condition or
        a lattice system) and the composition given.  `target`: patterns [n_points] or [B, n_points] on the grid of `params`, or
        crystals (a SampleResult or a loaded file), whose patterns are computed under the same params before the loop.  Every
        network evaluation is followed, after contact guidance's launch, by one launch that adds the gradient of the distance
        (1 - cos(P, Q)) / 2 between the pattern P of the current positions and the target Q, preconditioned by the cell and
        scaled by weight / sigma_t^2, to the predicted eps.  The amplitude of an atom is that of its current class (Z, or 1 under
        scattering "unit"; 0 for the mask class: a masked atom neither scatters nor is pushed).  noise="philox" runs it inside the
        loop, graph replay included; noise="device" and "reference" run the same launch between the evaluation and the step
        (arreau_xrd_guidance_step).  SampleResult.info["xrd_guidance"] holds the last evaluation's distance, reflections and
        flags per crystal (xrd_guidance.INFO_KEYS).  Positions only: a wrong cell cannot be repaired; no guidance of species, no
        intensity scale or background fit, no weight schedule other than 1 / sigma_t^2, crystals of more than 256 atoms are
        flagged LARGE and not guided; no claim on sample quality.  A bad value, scattering "weights" and a target count other
        than 1 or the batch's are rejected before any work.  weight = 0 and None: no launch is added and the results are what they
        were, bit for bit (None also through the exports it used)."""
        options = {k: v for k, v in locals().items() if k != "self"}  # (first statement: the keywords as given, nothing else)
        sample_plan.check_options(**options)  # (what needs nothing of self, first)
        plan = sample_plan.resolve(self.T, **options)
        eng = model.engine()
        dev = eng.device
        state, constant_atoms = self._starting_state(plan, model, initial_state, constant_atoms, condition, seed)
        if noise == "philox" and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        buf = _RunBuffers.upload(dev, plan, state, constant_atoms is not None, self.T,
                                 float(getattr(self.lattice_diffusion, "clipmax", lattice_clipmax)))
        # the generator states a re-run below starts from (the draws of noise='reference' and of noise='device')
        rng_state = torch.random.get_rng_state()
        cuda_rng_state = torch.cuda.get_rng_state(dev) if noise == "device" else None
        if plan.crystal_keys is not None:  # keyed sampling: the table of stream seeds, held through every call of the run
            buf.seeds_d = keyed_mod.device_seeds(keyed_mod.stream_seeds(seed, plan.crystal_keys), dev)
        if condition is not None:
            # rule 5: the known components of the drawn initial state, at the first timestep t_1 (T - 1 without a schedule;
            # Philox key t_1 + 1); the saved initial state of a re-run below includes them
            buf.cond_d = condition.device_arrays(z_table, dev)
            eng.condition_initial_state(buf.frac_d, buf.types_d, buf.len_d, plan.t_first, seed, buf.cond_d, offsets=buf.off_d,
                                        crystal_seeds=buf.seeds_d)
        if plan.xrd_guidance is not None:  # the target rows (crystals: one xrd launch), the class amplitudes, the diagnostics
            buf.xguide = xrd_guidance_mod.device_guidance(plan.xrd_guidance, z_table, plan.B, dev)
        saved = buf.snapshot()

        def frame(suffix):  # the current state as a frame file
            vis_crystal_during_sampling(z_table, buf.types_d.cpu().numpy(), buf.lattice_d.cpu().numpy(), buf.frac_d.cpu().numpy(),
                                        vis_name + suffix, show_bonds, plan.num_atoms.numpy())
        driver = _philox_driver if noise == "philox" else _host_noise_driver
        driver(eng, plan, buf, seed, plan.use_graph, frame)

        # Range safety without an environment variable: the fp16x3 kernels never clamp -- an activation beyond 65504 reaches the
        # outputs as NaN and sets the sticky NONFINITE flag.  When that happens on the default kernels the batch is re-run HERE,
        # from its saved initial state and with the same draws (same Philox seed / same host and device generator states), on
        # the full-range bf16x6 kernels; the engine stays on them if that run came out finite, and the result says so
        # (SampleResult.info).  Before that, when fp8 operand planes were in use (basis stash residual, cross products of the layer
        # projections): a basis value beyond e4m3's range turns into NaN there (the hardware conversion does not saturate), so the
        # batch is first re-run with two fp16 planes and three fp16 products, which the engine then keeps.
        def rerun():
            eng.status(reset=True)
            buf.restore(saved)
            torch.random.set_rng_state(rng_state)
            if cuda_rng_state is not None:
                torch.cuda.set_rng_state(cuda_rng_state, dev)
            driver(eng, plan, buf, seed, False, frame)

        info = eng.rerun_if_out_of_range(rerun)  # (shared with PONITA_DIFFUSION.encode)
        eng.check_status()  # sticky device flags (non-finite outputs, clamped indices): raise instead of returning them
        if buf.guide is not None:
            info = dict(info or {}, contact_guidance=guidance_mod.info_to_numpy(buf.guide[1]))
        if buf.xguide is not None:
            info = dict(info or {}, xrd_guidance=xrd_guidance_mod.info_to_numpy(buf.xguide.info))
        if visualization_setting != VisualizationSetting.NONE:
            frame("_final")
        # the instruments, by table: each reads the final state where it is and fills its own field
        atomic_numbers = atomic_number_indexes_to_atomic_numbers(z_table, buf.types_d.cpu().numpy())
        final = instruments.DeviceState(eng, buf.frac_d, buf.lattice_d, buf.off_d, buf.types_d, z_table, plan.num_atoms.numpy(),
                                        atomic_numbers, mask_type=-1 if constant_atoms is not None else plan.S - 1)
        fields = {e.field: e.run(final, plan.instruments[e.keyword]) if plan.instruments[e.keyword] is not None else None
                  for e in instruments.COMPLETE}
        return SampleResult(num_atoms=plan.num_atoms.numpy(), frac_x=buf.frac_d.cpu().numpy().astype(np.float64),
                            atomic_numbers=atomic_numbers, lattice=buf.lattice_d.cpu().numpy().astype(np.float64), info=info,
                            crystal_keys=np.array(plan.crystal_keys, dtype=np.int64) if plan.crystal_keys is not None else None,
                            **fields)

    def _starting_state(self, plan, model, initial_state, constant_atoms, condition, seed):
        """(the SamplerState the run starts from, constant_atoms as the run reads it): the draw of draw_initial_state, or the
        given state with its species replaced by the ones to hold when those are given (nothing is drawn)."""
        if initial_state is None:
            state = self.draw_initial_state(plan.num_atoms_per_sample, plan.B, num_atomic_states=plan.S, constant_atoms=constant_atoms,
                                            lattice_system=plan.lattice_system, condition=condition, specs=plan.specs, seed=seed,
                                            crystal_keys=plan.crystal_keys, model=model)
        else:
            state = initial_state
            if constant_atoms is False:
                constant_atoms = None
            if constant_atoms is not None and constant_atoms is not True:  # (its size: sample_plan.resolve)
                held = torch.as_tensor(constant_atoms).reshape(-1).long()
                state = inversion.SamplerState(state.frac_x, held.numpy(), state.lengths, state.angles, state.num_atoms, state.t,
                                               state.length_tie)
        if plan.allow_rows is not None and constant_atoms is True:  # the state's own species are held
            species_mod.check_held(plan.allow_rows, plan.crystal_of, np.asarray(state.species), np.ones(plan.N, bool),
                                   "constant_atoms=True")
        return state, constant_atoms
