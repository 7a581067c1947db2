"""HipEngine: owns the arreau_model handle (packed weights in HBM) and the step workspace.

Host-side plumbing only: tensors are allocated with torch, every arithmetic step on the sampler
state runs in libarreau_hip.so.
"""
import ctypes
import math
import os

import torch

from . import _hip
from .diffusion import (bond_order as bond_order_mod, cell_reduction, conventional_cell as conventional_mod,
                        coordination as coordination_mod, screening, symmetrize as symmetrize_mod, symmetry_search,
                        voronoi as voronoi_mod, xrd as xrd_mod)
from .diffusion import ewald as ewald_mod
from .diffusion import xrd_guidance as xrd_guidance_mod
from .diffusion.contact_guidance import INFO_KEYS, ContactGuidance
from .diffusion.corrector import check_corrector
from .diffusion.ddim import check_eta
from .diffusion.keyed import KIND_INIT_FRAC, KIND_INIT_LENGTHS
from .diffusion.multistep import HISTORY_KEYS, check_multistep
from .diffusion.resampling import check_resampling
from .diffusion.species import validate_temperature


def _f32(t):
    return t.detach().to("cpu", torch.float32).contiguous()


def _byref(struct):
    """A ctypes struct by reference, or NULL for None."""
    return ctypes.byref(struct) if struct is not None else None


def _require(label, name, t, shape, dtype, device, message=None):
    """The tensor contract of the entry points: `t` is a contiguous `dtype` tensor of `shape` (None: any, not empty) on `device`,
    else ValueError.  Under a label the text names the dtype as torch prints it ("condition: x0 must be a contiguous torch.float32
    tensor ..."), without one bare ("length_tie must be a contiguous int32 tensor ..."); `message` replaces the text."""
    if (torch.is_tensor(t) and t.dtype == dtype and t.device == device and t.is_contiguous()
            and (tuple(t.shape) == tuple(shape) if shape is not None else t.numel() > 0)):
        return
    if message is None:
        who, kind = (f"{label}: {name}", dtype) if label else (name, str(dtype).replace("torch.", ""))
        message = (f"{who} must be a contiguous {kind} tensor of shape {tuple(shape)} on {device}" if shape is not None
                   else f"{who} must be a non-empty contiguous {kind} tensor on {device}")
    raise ValueError(message)


# Which export serves an option set of sample_loop: (export, the option that selects it, the option columns it takes after the
# four common ones -- condition, schedule, corrector, resampling), read top to bottom; the first row whose option is given wins.
# "common": any of the four common options; the last row is the plain export, which takes none of them (A/B runs against an
# older library through ARREAU_HIP_LIB call it).  Two irregularities: _eta takes its float by value ("eta") while the species
# family takes it by pointer ("eta_ref", NULL: none), and _multistep skips the symmetry and eta columns.
_SPECIES_COLUMNS = ("tie", "sym", "eta_ref", "multistep", "species")
_LOOP_EXPORTS = (
    ("arreau_sample_loop_guided", "guidance", _SPECIES_COLUMNS + ("seeds", "guidance")),
    ("arreau_sample_loop_keyed", "seeds", _SPECIES_COLUMNS + ("seeds",)),
    ("arreau_sample_loop_species", "species", _SPECIES_COLUMNS),
    ("arreau_sample_loop_multistep", "multistep", ("tie", "multistep")),
    ("arreau_sample_loop_sym", "sym", ("tie", "sym")),
    ("arreau_sample_loop_eta", "eta", ("tie", "eta")),
    ("arreau_sample_loop_tied", "tie", ("tie",)),
    ("arreau_sample_loop_resampled", "common", ()),
    ("arreau_sample_loop", None, None),
)
# XRD guidance: the row read ahead of the table's -- the guided export plus the struct
_XRD_LOOP_EXPORT = ("arreau_sample_loop_xrd_guided", "xrd_guidance", _SPECIES_COLUMNS + ("seeds", "guidance", "xrd_guidance"))


def screen(frac, lattice, offsets, types=None, criteria=None):
    """The structural screen without an engine (arreau_crystal_screen needs no model): diffusion.screening.screen."""
    return screening.screen(frac, lattice, offsets, types, criteria)


def reduce_cells(frac, lattice, offsets, types, params=None):
    """The cell reduction without an engine (arreau_crystal_reduce needs no model): diffusion.cell_reduction.reduce_cells."""
    return cell_reduction.reduce_cells(frac, lattice, offsets, types, params)


def conventional_cell(frac, lattice, offsets, types, params=None, reduced=None):
    """The conventional cells without an engine (arreau_crystal_conventional needs no model): diffusion.conventional_cell.conventional_cell."""
    return conventional_mod.conventional_cell(frac, lattice, offsets, types, params, reduced)


def coordination(frac, lattice, offsets, params=None):
    """The coordination environments without an engine (arreau_crystal_coordination needs no model): diffusion.coordination.coordination."""
    return coordination_mod.coordination(frac, lattice, offsets, params)


def voronoi(frac, lattice, offsets, params=None):
    """The Voronoi cells without an engine (arreau_crystal_voronoi needs no model): diffusion.voronoi.voronoi."""
    return voronoi_mod.voronoi(frac, lattice, offsets, params)


def ewald(frac, lattice, offsets, charges_or_atomic_numbers, params=None):
    """The Ewald sums without an engine (arreau_crystal_ewald needs no model): diffusion.ewald.ewald."""
    return ewald_mod.ewald(frac, lattice, offsets, charges_or_atomic_numbers, params)


def xrd(frac, lattice, offsets, weights_or_atomic_numbers, params=None):
    """The powder diffraction patterns without an engine (arreau_crystal_xrd needs no model): diffusion.xrd.xrd."""
    return xrd_mod.xrd(frac, lattice, offsets, weights_or_atomic_numbers, params)


def bond_order(frac, lattice, offsets, params=None):
    """The bond angles and Steinhardt order parameters without an engine (arreau_crystal_bond_order needs no model): diffusion.bond_order.bond_order."""
    return bond_order_mod.bond_order(frac, lattice, offsets, params)


def symmetrize(frac, lattice, offsets, types, params=None, found=None):
    """The symmetrization without an engine (arreau_crystal_symmetrize needs no model): diffusion.symmetrize.symmetrize."""
    return symmetrize_mod.symmetrize(frac, lattice, offsets, types, params, found)


def find_symmetry(frac, lattice, offsets, types, params=None):
    """The symmetry search without an engine (arreau_crystal_symmetry needs no model): diffusion.symmetry_search.find_symmetry."""
    return symmetry_search.find_symmetry(frac, lattice, offsets, types, params)


def pack_state(module):
    """(Config, host tensors, StateDict of their pointers) of a PONITA_DIFFUSION in the reference's state_dict layout: what
    arreau_model_create and arreau_calibrate_formats take.  Host side only; the tensors must outlive every use of the struct."""
    net = module.model
    sd = module.state_dict()
    L = net.num_layers
    S = module.num_atomic_states
    cfg = _hip.Config(
        num_atomic_states=S, hidden_dim=net.hidden_dim, basis_dim=net.basis_dim, num_layers=L,
        num_ori=net.num_ori, widening_factor=net.widening_factor, degree=net.degree,
        max_neighbors=int(module.diffusion_loss.max_neighbors), num_timesteps=int(module.diffusion_loss.T),
        radius=float(module.diffusion_loss.cutoff),
        has_layer_scale=int(f"model.interaction_layers.0.layer_scale" in sd and
                            sd["model.interaction_layers.0.layer_scale"] is not None))
    il = "model.interaction_layers.{}."
    stack = lambda fmt: torch.stack([_f32(sd[fmt.format(i)]) for i in range(L)], 0).contiguous()
    host = {
        "basis_w1": _f32(sd["model.basis_fn.1.weight"]), "basis_b1": _f32(sd["model.basis_fn.1.bias"]),
        "basis_w2": _f32(sd["model.basis_fn.3.weight"]), "basis_b2": _f32(sd["model.basis_fn.3.bias"]),
        "fiber_w1": _f32(sd["model.fiber_basis_fn.1.weight"]), "fiber_b1": _f32(sd["model.fiber_basis_fn.1.bias"]),
        "fiber_w2": _f32(sd["model.fiber_basis_fn.3.weight"]), "fiber_b2": _f32(sd["model.fiber_basis_fn.3.bias"]),
        "x_embedder_w": _f32(sd["model.x_embedder.weight"]),
        "conv_kernel_w": stack(il + "conv.kernel.weight"), "conv_fiber_w": stack(il + "conv.fiber_kernel.weight"),
        "conv_bias": stack(il + "conv.bias"), "norm_w": stack(il + "norm.weight"), "norm_b": stack(il + "norm.bias"),
        "linear1_w": stack(il + "linear_1.weight"), "linear1_b": stack(il + "linear_1.bias"),
        "linear2_w": stack(il + "linear_2.weight"), "linear2_b": stack(il + "linear_2.bias"),
        "readout_w": stack("model.read_out_layers.{}.weight"), "readout_b": stack("model.read_out_layers.{}.bias"),
        "ori_grid": _f32(net.ori_grid), "t_emb_w": _f32(sd["t_emb.gaussian_fourier_proj_w"]),
        "ve_sigmas": _f32(sd["diffusion_loss.pos_diffusion.sigmas"]),
        "vp_alpha_bars": _f32(sd["diffusion_loss.lattice_diffusion.alpha_bars"]),
        "vp_betas": _f32(sd["diffusion_loss.lattice_diffusion.betas"]),
        "q_one_step_transposed": _f32(sd["diffusion_loss.d3pm.q_one_step_transposed"]),
        "q_mats": _f32(sd["diffusion_loss.d3pm.q_mats"]),
    }
    if cfg.has_layer_scale:
        host["layer_scale"] = stack(il + "layer_scale")
    expect = {"basis_w1": (net.hidden_dim, 258), "x_embedder_w": (net.hidden_dim, S + 78),
              "readout_w": (L, S + 4, net.hidden_dim), "ori_grid": (net.num_ori, 3),
              "q_mats": (cfg.num_timesteps, S, S), "ve_sigmas": (cfg.num_timesteps + 1,)}
    for k, shp in expect.items():
        if tuple(host[k].shape) != shp:
            raise ValueError(f"state_dict entry for {k} has shape {tuple(host[k].shape)}, expected {shp}")
    csd = _hip.StateDict()
    for name in _hip._SD_FIELDS:
        t = host.get(name)
        setattr(csd, name, t.data_ptr() if t is not None else None)
    return cfg, host, csd, S, L


class HipEngine:
    def __init__(self, module, device):
        """module: a PONITA_DIFFUSION (state_dict layout of the reference); device: cuda device."""
        _hip.require_gpu()
        self.device = torch.device(device)
        cfg, host, csd, S, L = pack_state(module)
        self.cfg = cfg
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _hip.check(_hip.lib().arreau_model_create(ctypes.byref(cfg), ctypes.byref(csd),
                                                      _hip.stream_ptr(self.device), ctypes.byref(self._handle)),
                       "arreau_model_create")
        self._host_keepalive = host
        self._ws = None
        self._ws_cap = (0, 0)
        self.S, self.k = S, cfg.max_neighbors
        self.stale_for_sampling = False
        # shapes without fused kernels run on the shape-general fp32 kernels (csrc/train_net.hip), which read the plain
        # weights update_train_weights refreshes: such an engine never goes stale for sampling
        self.fused_shape = (cfg.hidden_dim, cfg.basis_dim, cfg.widening_factor) == (128, 256, 4)
        self._general = not self.fused_shape or bool(os.environ.get("ARREAU_GENERAL_PATH"))

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            _hip.lib().arreau_model_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def status(self, reset=False):
        """Sticky device-side condition flags + the kernel families the last predict_scores launched
        (arreau_model_status; synchronises the stream)."""
        st = _hip.Status()
        _hip.check(_hip.lib().arreau_model_status(self._handle, ctypes.byref(st), int(bool(reset)),
                                                   _hip.stream_ptr(self.device)), "arreau_model_status")
        return {"flags": int(st.flags), "edge_kernel": _hip.EDGE_KERNELS.get(st.edge_kernel, "none"),
                "mlp_kernel": _hip.MLP_KERNELS.get(st.mlp_kernel, "none"), "edge_variant": int(st.edge_kernel),
                "mlp_variant": int(st.mlp_kernel), "conv_variant": int(st.conv_kernel),
                "basis_row_bytes": int(st.basis_row_bytes), "conv_cross_fp8": int(st.conv_cross_fp8), "edge_activation_bound": float(st.edge_activation_bound),
                "node_activation_bound": float(st.node_activation_bound),
                "basis_fp8_share": float(st.basis_fp8_share), "cross_fp8_share": float(st.cross_fp8_share),
                "readout_kernel": int(st.readout_kernel)}

    def check_status(self, reset=True):
        """Raise if a kernel flagged a condition under which its results must not be trusted."""
        st = self.status(reset=reset)
        f = st["flags"]
        if f:
            why = []
            if f & _hip.STATUS_NONFINITE:
                why.append("a network output is inf/NaN (an activation left the fp16 range of the fp16x3 kernels, "
                           "or the inputs/weights are non-finite); ARREAU_EDGE_VARIANT=3 ARREAU_MLP_VARIANT=1 selects the "
                           "full-range bf16x6 kernels")
            if f & _hip.STATUS_BAD_TIMESTEP:
                why.append("a timestep index was outside the schedule")
            if f & _hip.STATUS_BAD_TYPE:
                why.append("an atom-type index was outside [0, num_atomic_states)")
            if f & _hip.STATUS_BAD_TIE:
                why.append("a lattice-system tie code was outside 0..2")
            if f & _hip.STATUS_BAD_SYMMETRY:
                why.append("a space-group symmetry table entry was out of range or inconsistent")
            raise _hip.ArreauHipError("arreau_hip status flags %d: %s" % (f, "; ".join(why)))
        return st

    def set_formats(self, basis_fp8=-1, cross_fp8=-1):
        """Operand formats of the message path for this model (arreau_model_set_formats; -1 keeps the current choice)."""
        _hip.check(_hip.lib().arreau_model_set_formats(self._handle, int(basis_fp8), int(cross_fp8)), "arreau_model_set_formats")

    def fp8_formats_in_use(self, st=None):
        """Did the last evaluation read an fp8 residual plane / run fp8 cross products?  (arreau_model_status)"""
        st = self.status(reset=False) if st is None else st
        return st["conv_variant"] == 2 and (st["basis_row_bytes"] == 768 or st["conv_cross_fp8"] == 1)

    def checked(self, fn):
        """Run `fn()` (one evaluation through this engine), then read the sticky flags.  A NONFINITE flag while fp8 operand
        formats were in use is first taken for what it usually is -- a basis value beyond e4m3's range (the hardware's fp8
        conversion returns NaN above 464; tools/exp/fp8_cvt_check.hip): the model is switched to two fp16 planes and three fp16
        products for good and `fn()` runs once more; its result is the one returned.  Any flag that survives raises."""
        out = fn()
        st = self.status(reset=False)
        if st["flags"] == _hip.STATUS_NONFINITE and self.fp8_formats_in_use(st):
            import warnings
            warnings.warn("arreau_amd: non-finite outputs with fp8 operand planes in use (a basis value beyond e4m3's range?); this "
                          "engine keeps two fp16 planes and three fp16 products from now on and the evaluation is repeated with them")
            self.set_formats(0, 0)
            self.status(reset=True)
            out = fn()
        self.check_status()
        return out

    def rerun_if_out_of_range(self, rerun):
        """After a loop of evaluations on a batch (sample(), encode()): the range fallback both share.  `rerun()` resets the status
        word, restores the batch's saved initial state (and generator states) and runs the loop again, eagerly.  A NONFINITE flag
        with fp8 operand planes in use: the planes are switched to fp16 for good and the batch is re-run.  A NONFINITE flag on the
        default fp16x3 kernels of the fused shape: the batch is re-run on the full-range bf16x6 kernels, which the engine keeps if
        that run came out finite.  Returns what was done (SampleResult.info), or None; the caller reads the flags afterwards."""
        import warnings
        info = None
        st = self.status(reset=False)
        if st["flags"] == _hip.STATUS_NONFINITE and self.fp8_formats_in_use(st):
            warnings.warn("arreau_amd: non-finite outputs with fp8 operand planes in use (a basis value beyond e4m3's range?); "
                          "re-running the batch with two fp16 planes and three fp16 products, which this engine keeps from now on")
            self.set_formats(0, 0)
            rerun()
            info = {"fp16_planes_rerun": True}
            st = self.status(reset=False)
        overflow = (st["flags"] == _hip.STATUS_NONFINITE) and self.fused_shape \
            and (st["edge_kernel"] == "fp16x3" or st["mlp_kernel"].startswith("fp16x3"))
        if overflow:
            warnings.warn("arreau_amd: an activation left the fp16 range of the split-precision kernels (weights with activation "
                          f"bounds edge {st['edge_activation_bound']:.3g} / node {st['node_activation_bound']:.3g}); re-running the "
                          "batch on the full-range bf16x6 kernels, which this engine keeps if they come out finite")
            previous = (st["edge_variant"], st["mlp_variant"])
            self.set_variant(3, 1)
            rerun()
            if self.status(reset=False)["flags"] & _hip.STATUS_NONFINITE:
                self.set_variant(*previous)  # not a range problem (e.g. a degenerate cell): keep the faster kernels; the caller raises
            info = dict(info or {}, full_range_rerun=True, kernels="bf16x6", edge_activation_bound=st["edge_activation_bound"],
                        node_activation_bound=st["node_activation_bound"])
        return info

    def set_batch_layout(self, num_atoms, groups=0):
        """Kept for callers of the former batch-slicing experiment: the library runs the score network as one stream
        over the whole batch, so `groups` 0 and 1 change nothing and larger values raise ValueError.  (Slices on
        separate streams were not reproducible on MI355X, cause unknown: DESIGN.md section 8.)"""
        if int(groups) > 1:
            raise ValueError(f"set_batch_layout: groups={int(groups)} is not supported; the library runs one stream over "
                             "the whole batch")

    def set_variant(self, edge=-1, mlp=-1):
        """Select the arithmetic of the dense kernels (edge: 0 fp32 MFMA, 3 bf16x6, 4 fp16x3; mlp: 0 fp32 MFMA,
        1 (also 2) bf16x6, 3 fp16x3, 4 = always the (bit-identical) small-launch form of 3); -1 keeps.  edge = 5 runs the whole network
        on the shape-general fp32 GEMM kernels (the only choice for shapes other than hidden_dim 128 / basis_dim 256 / widening 4)."""
        _hip.check(_hip.lib().arreau_model_set_variant(self._handle, int(edge), int(mlp)), "arreau_model_set_variant")
        if int(edge) >= 0:
            self._general = int(edge) == _hip.VARIANT_GENERAL

    def ponita_forward(self, x, vec, lattice, offsets, edges):
        """The inner operator seam (PonitaFiberBundle.forward on the reference's batch attributes).
        x [N,S+74], vec [N,4,3], lattice [B,3,3] f32; offsets [B+1] i32; edges = slot arrays (deg, src, dir, dist).
        Returns (logits [N,S], vec_out [N,1,3], global_scalar [B,3])."""
        dev = self.device
        N, B = x.shape[0], lattice.shape[0]
        if x.shape[1] != self.S + 74 or tuple(vec.shape) != (N, 4, 3):
            raise ValueError(f"x must be [N,{self.S + 74}] and vec [N,4,3]; got {tuple(x.shape)}, {tuple(vec.shape)}")
        logits = torch.empty((N, self.S), device=dev, dtype=torch.float32)
        vec_out = torch.empty((N, 1, 3), device=dev, dtype=torch.float32)
        gscalar = torch.empty((B, 3), device=dev, dtype=torch.float32)
        ws = self.workspace(N, B)
        deg, src, direction, dist = edges
        _hip.check(_hip.lib().arreau_ponita_forward(
            self._handle, _hip.ptr(x), _hip.ptr(vec), _hip.ptr(lattice), _hip.ptr(offsets), B, N, _hip.ptr(deg),
            _hip.ptr(src), _hip.ptr(direction), _hip.ptr(dist), _hip.ptr(logits), _hip.ptr(vec_out), _hip.ptr(gscalar),
            _hip.ptr(ws), ws.numel(), _hip.stream_ptr(dev)), "arreau_ponita_forward")
        return logits, vec_out, gscalar

    def sample_loop(self, frac, types, lengths, angles, offsets, t_start, n_steps, seed, const_types, lattice_out,
                    use_graph=False, fixed_lengths=None, condition=None, next_table=None, lattice_clipmax=0.999, corrector=None,
                    resampling=None, length_tie=None, symmetry=None, eta=None, multistep=None, species=None, crystal_seeds=None,
                    guidance=None, xrd_guidance=None):
        """n_steps iterations of the sampling loop in one library call (arreau_sample_loop; with any of the options below
        arreau_sample_loop_resampled, whose NULL options are the loop without them): in-place update of
        (frac, types, lengths); Philox noise keyed by (seed, timestep, draw, element).  `condition`: the device arrays of a
        conditioned run (SampleCondition.device_arrays: x0, pos_mask, a0, type_mask, l0, len_mask; None entries allowed),
        through arreau_sample_loop_conditioned.  `next_table`: a respaced run (arreau_sample_loop_scheduled): the device
        int32 [T+1] table of respacing.next_table, with VP_lattice's clipmax; t_start is then a scheduled timestep.
        `corrector`: (steps, snr) -- predictor-corrector sampling (arreau_sample_loop_corrected): `steps` Langevin corrector
        moves on the positions before every step's predictor; None is the loop without them.
        `resampling`: (passes, jump_length[, timesteps]) -- RePaint resampling (arreau_sample_loop_resampled): the call's steps in
        blocks of jump_length, each run `passes` times with a forward jump back to the block's top in front of every pass after
        the first; `timesteps` is the host list of the schedule behind next_table (required with it).  None or passes == 1 is
        the loop without resampling.
        `length_tie`: lattice systems (arreau_sample_loop_tied): a contiguous int32 [B] tensor on the device, the tie code of every
        crystal's lengths (0 none, 1 a = b, 2 a = b = c; lattice_systems.py); None is the loop without it.
        `symmetry`: space-group symmetry (arreau_sample_loop_sym): the dict of device tables of symmetry.device_arrays; None is
        the loop without it.  Not with `condition`, corrector steps or resampling passes > 1 (the library rejects them).
        `eta`: DDIM-style sampling (arreau_sample_loop_eta): a float in [0, 1] that scales the noise every step injects into
        positions and lengths (0: none, and the draws are not read); None is the loop without it.  Not with `symmetry`.
        `multistep`: second-order multistep sampling (arreau_sample_loop_multistep): the dict of history tensors of
        multistep.allocate_history, read and overwritten by every step and never emptied by a call; None is the loop without it.
        Not with `condition`, corrector steps, resampling passes > 1, `symmetry` or an eta other than 0.
        `species`: species control (arreau_sample_loop_species; see sample_loop_species); None is the loop without it.
        `crystal_seeds`: keyed sampling (arreau_sample_loop_keyed; rules in include/arreau_hip.h): a contiguous int64 [B] tensor on
        the device holding the uint64 stream seeds of keyed.stream_seeds -- every draw of crystal b is then keyed by its seed and
        counted within the crystal.  The export is the species one plus the table, so without `species` the steps run under
        (every class, temperature 1).  None is the loop without it, through the export it used.
        `guidance`: contact guidance (arreau_sample_loop_guided; rules in include/arreau_hip.h): a contact_guidance.ContactGuidance,
        or the pair (ContactGuidance, info) with info the dict of device arrays of contact_guidance.allocate_info, which then hold
        the last evaluation's energy, contacts and flags per crystal.  Every network evaluation of every step is followed by one
        launch that adds the gradient of the contact penalty to its eps.  The export is the keyed one plus the struct, so without
        `species` the steps run under (every class, temperature 1).  None is the loop without it, through the export it used.
        `xrd_guidance`: XRD guidance (arreau_sample_loop_xrd_guided; rules in include/arreau_hip.h): an
        xrd_guidance.DeviceGuidance -- the xrd parameters, the weight, the target patterns [B, n_points], the class amplitudes [S]
        and, when given, the info arrays of xrd_guidance.allocate_info, which then hold the last evaluation's distance,
        reflections and flags per crystal.  Every network evaluation of every step is followed, after contact guidance's launch,
        by one launch that adds the gradient of the pattern distance to its eps.  The export is the guided one plus the struct.
        None is the loop without it, through the export it used."""
        N, B = frac.shape[0], lengths.shape[0]
        guide = self._guidance_struct(guidance, B) if guidance is not None else None
        xguide = self._xrd_guidance_struct(xrd_guidance, B, N) if xrd_guidance is not None else None
        if crystal_seeds is not None:
            self._check_seeds(crystal_seeds, B)
        if (guide is not None or xguide is not None or crystal_seeds is not None) and species is None:
            species = (None, 1.0)
        if multistep is not None:
            check_multistep(True, eta=eta, condition=condition, corrector_steps=corrector[0] if corrector is not None else 0,
                            resample_passes=resampling[0] if resampling is not None else 1, symmetry=symmetry)
            eta = None  # (the multistep export takes none: its steps are the eta = 0 steps)
        if eta is not None:
            eta = check_eta(eta)
            if symmetry is not None:
                raise ValueError("eta is not combined with symmetry tables")
        res = ts_arr = None
        if resampling is not None:
            passes, jump = check_resampling(*resampling[:2])
            ts = list(resampling[2]) if len(resampling) > 2 and resampling[2] is not None else None
            if passes > 1:
                if next_table is not None and ts is None:
                    raise ValueError("resampling on a respaced loop needs the host list of its timesteps")
                ts_arr = (ctypes.c_int32 * len(ts))(*ts) if ts else None  # (alive until the call returns)
                res = _hip.ResamplingC(passes, jump, ctypes.cast(ts_arr, ctypes.POINTER(ctypes.c_int32)) if ts else None,
                                       len(ts) if ts else 0)
        if corrector is not None:
            corrector = check_corrector(*corrector)
        ws = self.workspace(N, B)
        args = (self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(offsets), B, N,
                int(t_start), int(n_steps), int(seed) & (2 ** 64 - 1), _hip.ptr(const_types), _hip.ptr(fixed_lengths),
                _hip.ptr(lattice_out), _hip.ptr(ws), ws.numel(), int(bool(use_graph)))
        sched = None
        if next_table is not None:
            _require("", "next_table", next_table, (int(self.cfg.num_timesteps) + 1,), torch.int32, self.device)
            sched = _hip.SampleScheduleC(_hip.ptr(next_table).value, float(lattice_clipmax))
        cond = self._condition_struct(condition, N, B) if condition is not None else None
        corr = _hip.CorrectorC(corrector[0], corrector[1]) if corrector is not None else None
        self._check_tie(length_tie, B)
        common = (_byref(cond), _byref(sched), _byref(corr), _byref(res))
        eta_c = ctypes.c_float(eta) if eta is not None else None
        columns = {"tie": _hip.ptr(length_tie), "eta": eta_c, "eta_ref": _byref(eta_c), "seeds": _hip.ptr(crystal_seeds),
                   "sym": _byref(self._symmetry_struct(symmetry, N) if symmetry is not None else None),
                   "multistep": _byref(self._multistep_struct(multistep, N, B) if multistep is not None else None),
                   "species": _byref(self._species_struct(species, B) if species is not None else None), "guidance": _byref(guide),
                   "xrd_guidance": _byref(xguide)}
        given = {"xrd_guidance": xguide, "guidance": guide, "seeds": crystal_seeds, "species": species, "multistep": multistep, "sym": symmetry, "eta": eta,
                 "tie": length_tie, "common": next((o for o in common if o is not None), None)}
        name, _, takes = next(row for row in (_XRD_LOOP_EXPORT,) + _LOOP_EXPORTS if row[1] is None or given[row[1]] is not None)
        opts = common + tuple(columns[c] for c in takes) if takes is not None else ()
        _hip.check(getattr(_hip.lib(), name)(*args, *opts, _hip.stream_ptr(self.device)), name)

    def _guidance_struct(self, guidance, B):
        """arreau_contact_guidance of a ContactGuidance or of the pair (ContactGuidance, info), with the info arrays' shape, dtype
        and device checked."""
        params, info = guidance if isinstance(guidance, tuple) else (guidance, None)
        if not isinstance(params, ContactGuidance):
            raise ValueError(f"guidance must be a ContactGuidance or the pair (ContactGuidance, info), got {guidance!r}")
        ptrs = [None, None, None]
        if info is not None:
            if not isinstance(info, dict) or set(info) != set(INFO_KEYS):
                raise ValueError(f"guidance info: expected a dict with exactly the keys {INFO_KEYS}")
            for q, name in enumerate(INFO_KEYS):
                _require("guidance info", name, info[name], (B,), torch.float32 if name == "energy" else torch.int32, self.device)
                ptrs[q] = _hip.ptr(info[name]).value
        return _hip.ContactGuidanceC(params.min_distance, params.weight, params.max_shells, *ptrs)

    def contact_guidance_step(self, frac, lattice, t_crystal, offsets, eps, guidance):
        """Contact guidance on eps [N,3] in place (arreau_contact_guidance_step; rules in include/arreau_hip.h): frac [N,3] f32,
        lattice [B,3,3] f32 (the cells the evaluation saw, rows a, b, c), t_crystal [B] i32, offsets [B+1] i32, `guidance` as in
        sample_loop.  Between predict_scores and a step export it is the guided loop's step bit for bit.  Returns eps."""
        B, N = int(t_crystal.shape[0]), int(frac.shape[0])
        guide = self._guidance_struct(guidance, B)
        for name, t, shape, dtype in (("frac", frac, (N, 3), torch.float32), ("lattice", lattice, (B, 3, 3), torch.float32),
                                      ("t_crystal", t_crystal, (B,), torch.int32), ("offsets", offsets, (B + 1,), torch.int32),
                                      ("eps", eps, (N, 3), torch.float32)):
            _require("contact_guidance_step", name, t, shape, dtype, self.device)
        _hip.check(_hip.lib().arreau_contact_guidance_step(
            self._handle, _hip.ptr(frac), _hip.ptr(lattice), _hip.ptr(t_crystal), _hip.ptr(offsets), B, N, _hip.ptr(eps),
            ctypes.byref(guide), _hip.stream_ptr(self.device)), "arreau_contact_guidance_step")
        return eps

    def _xrd_guidance_struct(self, guidance, B, N, step=False):
        """arreau_xrd_guidance of an xrd_guidance.DeviceGuidance, with its tensors' shape, dtype and device checked; keeps the
        nested parameter struct alive with the result."""
        g = guidance
        if not isinstance(g, xrd_guidance_mod.DeviceGuidance) or not isinstance(g.params, xrd_mod.XrdParams):
            raise ValueError(f"xrd_guidance must be an xrd_guidance.DeviceGuidance, got {guidance!r}")
        p = g.params
        _require("xrd guidance", "target", g.target, (B, p.n_points), torch.float32, self.device)
        if (g.class_weights is None) == (g.atom_weights is None) or (g.atom_weights is not None and not step):
            raise ValueError("xrd guidance: exactly one of class_weights and atom_weights (the step export alone) is required")
        if g.class_weights is not None:
            _require("xrd guidance", "class_weights", g.class_weights, (self.S,), torch.float32, self.device)
        else:
            _require("xrd guidance", "atom_weights", g.atom_weights, (N,), torch.float32, self.device)
        ptrs = [None, None, None]
        if g.info is not None:
            if not isinstance(g.info, dict) or set(g.info) != set(xrd_guidance_mod.INFO_KEYS):
                raise ValueError(f"xrd guidance info: expected a dict with exactly the keys {xrd_guidance_mod.INFO_KEYS}")
            for q, name in enumerate(xrd_guidance_mod.INFO_KEYS):
                _require("xrd guidance info", name, g.info[name], (B,), torch.float32 if name == "distance" else torch.int32, self.device)
                ptrs[q] = _hip.ptr(g.info[name]).value
        params = _hip.XrdParamsC(p.wavelength, p.two_theta_min, p.two_theta_max, p.fwhm, p.b_iso, p.n_points, p.max_index)
        value = lambda t: _hip.ptr(t).value if t is not None else None
        return _hip.XrdGuidanceC(params, g.weight, value(g.target), value(g.class_weights), value(g.atom_weights), *ptrs)

    def xrd_guidance_step(self, frac, types, lattice, t_crystal, offsets, eps, guidance, gradient=None):
        """XRD guidance on eps [N,3] in place (arreau_xrd_guidance_step; rules in include/arreau_hip.h): frac [N,3] f32, types [N]
        i32 (None with atom weights), lattice [B,3,3] f32 (the cells the evaluation saw, rows a, b, c), t_crystal [B] i32, offsets
        [B+1] i32, `guidance` an xrd_guidance.DeviceGuidance (class or atom weights), gradient [N,3] f32 or None: receives g.
        Between predict_scores (and contact_guidance_step) and a step export it is the guided loop's step bit for bit.  Returns eps."""
        B, N = int(t_crystal.shape[0]), int(frac.shape[0])
        guide = self._xrd_guidance_struct(guidance, B, N, step=True)
        want = [("frac", frac, (N, 3), torch.float32), ("lattice", lattice, (B, 3, 3), torch.float32), ("t_crystal", t_crystal, (B,), torch.int32),
                ("offsets", offsets, (B + 1,), torch.int32), ("eps", eps, (N, 3), torch.float32)]
        if types is not None or guidance.atom_weights is None:
            want.append(("types", types, (N,), torch.int32))
        if gradient is not None:
            want.append(("gradient", gradient, (N, 3), torch.float32))
        for name, t, shape, dtype in want:
            _require("xrd_guidance_step", name, t, shape, dtype, self.device)
        _hip.check(_hip.lib().arreau_xrd_guidance_step(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lattice), _hip.ptr(t_crystal), _hip.ptr(offsets), B, N, _hip.ptr(eps),
            ctypes.byref(guide), _hip.ptr(gradient), _hip.stream_ptr(self.device)), "arreau_xrd_guidance_step")
        return eps

    def sample_loop_species(self, frac, types, lengths, angles, offsets, t_start, n_steps, seed, const_types, lattice_out, species,
                            **options):
        """sample_loop under species control (arreau_sample_loop_species; rules in include/arreau_hip.h): `species` is the pair
        (allow, temperature) -- allow the admission rows, a contiguous int32 tensor [B, 4] holding the uint32 words of
        species.pack_rows (None: every class for every crystal), temperature the scale of the species' Gumbel term (>= 0; at 0
        no uniform is drawn).  `options`: every keyword of sample_loop, combined and rejected as there."""
        if species is None:
            raise ValueError("sample_loop_species: species must be the pair (allow, temperature)")
        self.sample_loop(frac, types, lengths, angles, offsets, t_start, n_steps, seed, const_types, lattice_out, species=species,
                         **options)

    def _species_struct(self, species, B):
        """arreau_species_control of the pair (allow, temperature), with the rows' shape, dtype and device checked."""
        allow, tau = species
        tau = validate_temperature(tau)
        if allow is not None:
            _require("", "species control: allow", allow, (B, 4), torch.int32, self.device)
        return _hip.SpeciesControlC(_hip.ptr(allow).value if allow is not None else None, tau)

    def _multistep_struct(self, history, N, B):
        """arreau_multistep of the dict of history tensors of multistep.allocate_history, with shapes, dtypes and device checked."""
        if not isinstance(history, dict) or set(history) != set(HISTORY_KEYS):
            raise ValueError(f"multistep history: expected a dict with exactly the keys {HISTORY_KEYS}")
        want = {"hist_eps": ((N, 3), torch.float32), "hist_x0": ((B, 3), torch.float32), "hist_t_atom": ((N,), torch.int32),
                "hist_t_len": ((B,), torch.int32)}
        for n in HISTORY_KEYS:
            _require("multistep history", n, history[n], *want[n], self.device)
        return _hip.MultistepC(*[_hip.ptr(history[n]).value for n in HISTORY_KEYS])

    def _check_seeds(self, crystal_seeds, B):
        _require("", "crystal_seeds", crystal_seeds, (B,), torch.int64, self.device,
                 f"crystal_seeds must be a contiguous int64 tensor of shape ({B},) on {self.device} (the uint64 stream seeds)")

    def philox_fill_crystals(self, crystal_seeds, offsets, timestep, kind, word3=0, per_atom_width=0, per_crystal_width=0, raw=False):
        """The keyed draws written out in batch layout (arreau_philox_fill_crystals): per_atom_width = w gives [N, w] (row of atom a
        of crystal b: elements a w .. a w + w - 1 of its stream), per_crystal_width = w gives [B, w]; normal or uniform by kind.
        raw=True: also the raw words, int32 [.., w, 4]."""
        B = int(crystal_seeds.shape[0])
        self._check_seeds(crystal_seeds, B)
        if (per_atom_width > 0) == (per_crystal_width > 0):
            raise ValueError("philox_fill_crystals: give either per_atom_width or per_crystal_width")
        w = int(per_atom_width or per_crystal_width)
        rows = int(offsets[-1].item()) if per_atom_width > 0 else B
        out = torch.empty((rows, w), device=self.device, dtype=torch.float32)
        words = torch.empty((rows, w, 4), device=self.device, dtype=torch.int32) if raw else None
        _hip.check(_hip.lib().arreau_philox_fill_crystals(
            _hip.ptr(crystal_seeds), _hip.ptr(offsets), B, int(timestep), int(kind), int(word3) & (2 ** 32 - 1), int(per_atom_width),
            int(per_crystal_width), _hip.ptr(out), _hip.ptr(words), _hip.stream_ptr(self.device)), "arreau_philox_fill_crystals")
        return (out, words) if raw else out

    def keyed_initial_draws(self, crystal_seeds, offsets):
        """Rule 3 of keyed sampling: the standard normals of the initial lengths [B,3] (kind 13) and positions [N,3] (kind 14)."""
        return (self.philox_fill_crystals(crystal_seeds, offsets, 0, KIND_INIT_LENGTHS, per_crystal_width=3),
                self.philox_fill_crystals(crystal_seeds, offsets, 0, KIND_INIT_FRAC, per_atom_width=3))

    def _check_tie(self, length_tie, B):
        if length_tie is not None:
            _require("", "length_tie", length_tie, (B,), torch.int32, self.device)

    def _symmetry_struct(self, tables, N):
        """arreau_symmetry of the dict of device tables of symmetry.device_arrays, with shapes, dtypes and device checked."""
        names = ("leader", "op", "orbit", "orbit_ptr", "orbit_atoms", "stab_ptr", "stab_ops", "rot", "rot_inv", "trans")
        missing = [n for n in names if tables.get(n) is None]
        if missing or set(tables) - set(names):
            raise ValueError(f"symmetry tables: expected exactly {names}")
        for n in names:
            _require("symmetry tables", n, tables[n], None, torch.float32 if n in ("rot", "rot_inv", "trans") else torch.int32,
                     self.device)
        for n in ("leader", "op", "orbit"):
            if tuple(tables[n].shape) != (N,):
                raise ValueError(f"symmetry tables: {n} must have shape ({N},)")
        n_orb = tables["orbit_ptr"].numel() - 1
        if tables["stab_ptr"].numel() != n_orb + 1 or n_orb < 1:
            raise ValueError("symmetry tables: orbit_ptr and stab_ptr must both hold n_orbits + 1 >= 2 entries")
        n_ops = tables["rot"].numel() // 9
        if tuple(tables["rot"].shape) != (n_ops, 9) or tuple(tables["rot_inv"].shape) != (n_ops, 9) or \
                tuple(tables["trans"].shape) != (n_ops, 3):
            raise ValueError("symmetry tables: rot / rot_inv must be [n_ops, 9] and trans [n_ops, 3]")
        return _hip.SymmetryC(*[_hip.ptr(tables[n]).value for n in names], n_orb, tables["orbit_atoms"].numel(),
                              tables["stab_ops"].numel(), n_ops)

    def condition_initial_state(self, frac, types, lengths, t_start, seed, condition, offsets=None, crystal_seeds=None):
        """Rule 5 of conditioned sampling (arreau_condition_initial_state): the known components of an initial state drawn
        for timestep t_start, in place.  `crystal_seeds` (with `offsets`): keyed sampling (arreau_condition_initial_state_keyed)."""
        N, B = frac.shape[0], lengths.shape[0]
        cond = self._condition_struct(condition, N, B)
        name, offs, keyed = "arreau_condition_initial_state", (), ()
        if crystal_seeds is not None:
            self._check_seeds(crystal_seeds, B)
            if offsets is None:
                raise ValueError("condition_initial_state: crystal_seeds need the crystal offsets")
            name, offs, keyed = name + "_keyed", (_hip.ptr(offsets),), (_hip.ptr(crystal_seeds),)
        _hip.check(getattr(_hip.lib(), name)(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), *offs, B, N, int(t_start), int(seed) & (2 ** 64 - 1),
            ctypes.byref(cond), *keyed, _hip.stream_ptr(self.device)), name)

    def _condition_struct(self, condition, N, B):
        """arreau_sample_condition of a dict of device tensors, with their shapes, dtypes and device checked."""
        spec = {"x0": ((N, 3), torch.float32), "pos_mask": ((N,), torch.uint8), "a0": ((N,), torch.int32),
                "type_mask": ((N,), torch.uint8), "l0": ((B, 3), torch.float32), "len_mask": ((B,), torch.uint8)}
        unknown = set(condition) - set(spec)
        if unknown:
            raise ValueError(f"condition: unknown entries {sorted(unknown)}")
        c = _hip.SampleConditionC()
        for name, (shape, dtype) in spec.items():
            t = condition.get(name)
            if t is None:
                continue
            _require("condition", name, t, shape, dtype, self.device)
            setattr(c, name, _hip.ptr(t))
        return c

    def _philox_fill(self, name, n, raw, *key):
        """One of the philox_fill exports: `key`, then n, the normals or uniforms out [n] and, with raw, the words [n, 4]."""
        out = torch.empty(n, device=self.device, dtype=torch.float32)
        words = torch.empty((n, 4), device=self.device, dtype=torch.int32) if raw else None
        _hip.check(getattr(_hip.lib(), name)(*key, int(n), _hip.ptr(out), _hip.ptr(words), _hip.stream_ptr(self.device)), name)
        return (out, words) if raw else out

    def philox_fill(self, seed, timestep, kind, n, raw=False):
        """The sampler's in-kernel noise written out (arreau_philox_fill): kinds 0/1 (and 3/4, the draws of conditioned
        sampling) standard normal, 2 uniform [0,1)."""
        return self._philox_fill("arreau_philox_fill", n, raw, int(seed) & (2 ** 64 - 1), int(timestep), int(kind))

    def philox_fill_word(self, seed, timestep, kind, word3, n, raw=False):
        """arreau_philox_fill with the counter's fourth word (arreau_philox_fill_word): kind 5 with word3 = j is the Langevin
        noise of the loop's j-th corrector move at `timestep`."""
        return self._philox_fill("arreau_philox_fill_word", n, raw, int(seed) & (2 ** 64 - 1), int(timestep), int(kind), int(word3) & (2 ** 32 - 1))

    def corrector_step(self, frac, t_crystal, offsets, eps, z_frac, snr, condition=None):
        """One Langevin corrector move on frac [N,3] in place (arreau_corrector_step): per crystal at timestep t_crystal[b],
        from the network's eps [N,3] and the caller's standard-normal z_frac [N,3].  `condition`: as in sample_loop; its
        position mask keeps those atoms fixed and out of the norms."""
        _, snr = check_corrector(1, snr)
        N, B = frac.shape[0], t_crystal.shape[0]
        cond = self._condition_struct(condition, N, B) if condition is not None else None
        _hip.check(_hip.lib().arreau_corrector_step(
            self._handle, _hip.ptr(frac), _hip.ptr(t_crystal), _hip.ptr(offsets), B, N, _hip.ptr(eps), _hip.ptr(z_frac), snr,
            _byref(cond), _hip.stream_ptr(self.device)), "arreau_corrector_step")

    def diffusion_noise(self, frac0, types0, lattice0, t_crystal, offsets, z_frac, u_types, z_lengths):
        """Forward noising of a clean batch (arreau_diffusion_noise).  Returns dict(noisy_frac, target_eps, noisy_types,
        noisy_lengths, lengths, angles)."""
        dev = self.device
        N, B = frac0.shape[0], lattice0.shape[0]
        f32 = dict(device=dev, dtype=torch.float32)
        out = dict(noisy_frac=torch.empty((N, 3), **f32), target_eps=torch.empty((N, 3), **f32),
                   noisy_types=torch.empty(N, device=dev, dtype=torch.int32), noisy_lengths=torch.empty((B, 3), **f32),
                   lengths=torch.empty((B, 3), **f32), angles=torch.empty((B, 3), **f32))
        inv = torch.empty((B, 3, 3), **f32)
        _hip.check(_hip.lib().arreau_diffusion_noise(
            self._handle, _hip.ptr(frac0), _hip.ptr(types0), _hip.ptr(lattice0), _hip.ptr(t_crystal), _hip.ptr(offsets),
            B, N, _hip.ptr(z_frac), _hip.ptr(u_types), _hip.ptr(z_lengths), _hip.ptr(out["noisy_frac"]),
            _hip.ptr(out["target_eps"]), _hip.ptr(out["noisy_types"]), _hip.ptr(out["noisy_lengths"]),
            _hip.ptr(out["lengths"]), _hip.ptr(out["angles"]), _hip.ptr(inv), _hip.stream_ptr(dev)),
            "arreau_diffusion_noise")
        return out

    def diffusion_losses(self, pred_eps, target_eps, logits, types0, noisy_types, t_crystal, pred_lengths, lengths,
                         offsets, with_grads=False):
        """The three training errors (arreau_diffusion_losses).  Returns losses[6] = (loss, error_frac_x,
        error_atomic_type, error_lattice, vb, ce) [+ (grad_eps, grad_logits, grad_lengths)]."""
        dev = self.device
        N, B = pred_eps.shape[0], pred_lengths.shape[0]
        f32 = dict(device=dev, dtype=torch.float32)
        terms = torch.empty((N, 3), **f32)
        losses = torch.empty(6, **f32)
        g = (torch.empty((N, 3), **f32), torch.empty((N, self.S), **f32), torch.empty((B, 3), **f32)) if with_grads \
            else (None, None, None)
        _hip.check(_hip.lib().arreau_diffusion_losses(
            self._handle, _hip.ptr(pred_eps), _hip.ptr(target_eps), _hip.ptr(logits), _hip.ptr(types0),
            _hip.ptr(noisy_types), _hip.ptr(t_crystal), _hip.ptr(pred_lengths), _hip.ptr(lengths), _hip.ptr(offsets), B, N,
            _hip.ptr(terms), _hip.ptr(losses), _hip.ptr(g[0]), _hip.ptr(g[1]), _hip.ptr(g[2]), _hip.stream_ptr(dev)),
            "arreau_diffusion_losses")
        return (losses, g) if with_grads else losses

    # ---- training runs: keyed noise, per-crystal loss rows, their binned reduction (rules in include/arreau_hip.h) ----
    ROW_WORDS = 6  # arreau_loss_row: four float32 sums, int32 atom count, int32 timestep

    def diffusion_noise_keyed(self, frac0, types0, lattice0, offsets, seed, crystal_ids, copies=1, copy=None, t_crystal=None):
        """Forward noising with the draws made in the kernels, keyed by (seed, crystal id) (arreau_diffusion_noise_keyed).
        crystal_ids [B] int64 on the device; copy [B] int32 or None; t_crystal [B] int32: the caller's timesteps instead of the
        drawn ones.  Returns diffusion_noise's dict plus `t` (int32 [B], the timesteps used)."""
        dev = self.device
        N, B = frac0.shape[0], lattice0.shape[0]
        _require("", "crystal_ids", crystal_ids, (B,), torch.int64, dev, "crystal_ids must be an int64 tensor [B] on the engine's device")
        if copy is not None:
            _require("", "copy", copy, (B,), torch.int32, dev, "copy must be an int32 tensor [B] on the engine's device")
        f32 = dict(device=dev, dtype=torch.float32)
        t = torch.empty(B, device=dev, dtype=torch.int32) if t_crystal is None else t_crystal
        out = dict(noisy_frac=torch.empty((N, 3), **f32), target_eps=torch.empty((N, 3), **f32),
                   noisy_types=torch.empty(N, device=dev, dtype=torch.int32), noisy_lengths=torch.empty((B, 3), **f32),
                   lengths=torch.empty((B, 3), **f32), angles=torch.empty((B, 3), **f32), t=t)
        inv = torch.empty((B, 3, 3), **f32)
        _hip.check(_hip.lib().arreau_diffusion_noise_keyed(
            self._handle, _hip.ptr(frac0), _hip.ptr(types0), _hip.ptr(lattice0), _hip.ptr(offsets), B, N,
            int(seed) & (2 ** 64 - 1), _hip.ptr(crystal_ids), int(copies), _hip.ptr(copy), int(t_crystal is not None), _hip.ptr(t),
            _hip.ptr(out["noisy_frac"]), _hip.ptr(out["target_eps"]), _hip.ptr(out["noisy_types"]), _hip.ptr(out["noisy_lengths"]),
            _hip.ptr(out["lengths"]), _hip.ptr(out["angles"]), _hip.ptr(inv), _hip.stream_ptr(dev)),
            "arreau_diffusion_noise_keyed")
        return out

    def philox_fill_keyed(self, seed, timestep, kind, crystal_id, n, raw=False):
        """The keyed draws written out (arreau_philox_fill_keyed): kinds 10 / 12 standard normal, 9 / 11 uniform [0,1)."""
        return self._philox_fill("arreau_philox_fill_keyed", n, raw, int(seed) & (2 ** 64 - 1), int(timestep), int(kind), int(crystal_id) & (2 ** 32 - 1))

    def loss_row_table(self, n_rows):
        """A zeroed table of n_rows arreau_loss_row (int32 [n_rows, 6]; rows_to_fields views it)."""
        return torch.zeros((int(n_rows), self.ROW_WORDS), device=self.device, dtype=torch.int32)

    @staticmethod
    def rows_to_fields(rows):
        """(float32 [n, 4] coord / vb / ce / lattice sums, int32 [n] atom counts, int32 [n] timesteps) of a row table (copies)."""
        return rows[:, :4].contiguous().view(torch.float32), rows[:, 4].contiguous(), rows[:, 5].contiguous()

    def diffusion_loss_rows(self, pred_eps, target_eps, logits, types0, noisy_types, t_crystal, pred_lengths, lengths, offsets,
                            row_index, rows, with_grads=False):
        """diffusion_losses plus one row per crystal in the caller's table (arreau_diffusion_loss_rows): crystal b goes to
        rows[row_index[b]] (row_index int64 [B] on the device, rows from loss_row_table).  Returns (losses[6], (grad_eps,
        grad_logits, grad_lengths) or Nones, terms [N,3])."""
        dev = self.device
        N, B = pred_eps.shape[0], pred_lengths.shape[0]
        _require("", "row_index", row_index, (B,), torch.int64, dev, "row_index must be an int64 tensor [B] on the engine's device")
        if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != self.ROW_WORDS or rows.device != dev:
            raise ValueError("rows must come from loss_row_table")
        f32 = dict(device=dev, dtype=torch.float32)
        terms = torch.empty((N, 3), **f32)
        losses = torch.empty(6, **f32)
        g = (torch.empty((N, 3), **f32), torch.empty((N, self.S), **f32), torch.empty((B, 3), **f32)) if with_grads \
            else (None, None, None)
        _hip.check(_hip.lib().arreau_diffusion_loss_rows(
            self._handle, _hip.ptr(pred_eps), _hip.ptr(target_eps), _hip.ptr(logits), _hip.ptr(types0),
            _hip.ptr(noisy_types), _hip.ptr(t_crystal), _hip.ptr(pred_lengths), _hip.ptr(lengths), _hip.ptr(offsets), B, N,
            _hip.ptr(terms), _hip.ptr(losses), _hip.ptr(g[0]), _hip.ptr(g[1]), _hip.ptr(g[2]), _hip.ptr(row_index), _hip.ptr(rows),
            int(rows.shape[0]), _hip.stream_ptr(dev)), "arreau_diffusion_loss_rows")
        return losses, g, terms

    def loss_rows_reduce(self, rows, n_bins, T=None):
        """The binned fixed-order float64 reduction of a row table (arreau_loss_rows_reduce).  Returns device tensors
        (sums float64 [n_bins + 1, 4], counts int64 [n_bins + 1, 2], unwritten int64 [1]); the last record is the total."""
        dev = self.device
        T = int(self.cfg.num_timesteps if T is None else T)
        sums = torch.empty((n_bins + 1, 4), device=dev, dtype=torch.float64)
        counts = torch.empty(2 * (n_bins + 1) + 1, device=dev, dtype=torch.int64)
        _hip.check(_hip.lib().arreau_loss_rows_reduce(_hip.ptr(rows), int(rows.shape[0]), int(n_bins), T, _hip.ptr(sums),
                                                      _hip.ptr(counts), _hip.stream_ptr(dev)), "arreau_loss_rows_reduce")
        return sums, counts[:-1].view(n_bins + 1, 2), counts[-1:]

    # ---- training (BASELINE config 5) ---------------------------------------------------------------
    def train_forward(self, frac, types, lengths, angles, t_crystal, offsets):
        """Training-mode network evaluation (arreau_train_forward): fp32, activations kept for train_backward.
        Same inputs / outputs as predict_scores."""
        dev = self.device
        N, B = frac.shape[0], lengths.shape[0]
        eps = torch.empty((N, 3), device=dev, dtype=torch.float32)
        logits = torch.empty((N, self.S), device=dev, dtype=torch.float32)
        len0 = torch.empty((B, 3), device=dev, dtype=torch.float32)
        _hip.check(_hip.lib().arreau_train_forward(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(t_crystal),
            _hip.ptr(offsets), B, N, _hip.ptr(eps), _hip.ptr(logits), _hip.ptr(len0), _hip.stream_ptr(dev)),
            "arreau_train_forward")
        return eps, logits, len0

    def train_backward(self, grad_eps, grad_logits, grad_len0):
        """Backward pass of the last train_forward (arreau_train_backward).  Returns {state_dict key: gradient} for every
        trainable tensor of the score network, on the device, in the reference's parameter names and shapes."""
        dev = self.device
        cfg = self.cfg
        S, C, D, L, W = self.S, cfg.hidden_dim, cfg.basis_dim, cfg.num_layers, cfg.widening_factor
        H = W * C
        shapes = {"basis_w1": (C, 258), "basis_b1": (C,), "basis_w2": (D, C), "basis_b2": (D,), "fiber_w1": (C, 3),
                  "fiber_b1": (C,), "fiber_w2": (D, C), "fiber_b2": (D,), "x_embedder_w": (C, S + 78),
                  "conv_kernel_w": (L, C, D), "conv_fiber_w": (L, C, D), "conv_bias": (L, C), "norm_w": (L, C),
                  "norm_b": (L, C), "linear1_w": (L, H, C), "linear1_b": (L, H), "linear2_w": (L, C, H),
                  "linear2_b": (L, C), "layer_scale": (L, C), "readout_w": (L, S + 4, C), "readout_b": (L, S + 4)}
        # one zero-filled buffer per step, the gradients are views of it (21 fill launches were 0.1 ms of the step); every
        # view starts on a 16-byte boundary (the kernels write some of them as float4 columns)
        sizes = {k: -(-math.prod(v) // 4) * 4 for k, v in shapes.items()}
        flat = torch.zeros(sum(sizes.values()), device=dev, dtype=torch.float32)
        g, o = {}, 0
        for k, shp in shapes.items():
            g[k] = flat[o:o + math.prod(shp)].view(shp)
            o += sizes[k]
        csd = _hip.StateDict()
        for name in _hip._SD_FIELDS:
            t = g.get(name)
            setattr(csd, name, t.data_ptr() if t is not None else None)
        _hip.check(_hip.lib().arreau_train_backward(self._handle, _hip.ptr(grad_eps), _hip.ptr(grad_logits),
                                                    _hip.ptr(grad_len0), ctypes.byref(csd), _hip.stream_ptr(dev)),
                   "arreau_train_backward")
        self.last_grad_flat = flat  # every gradient of the step is a view of this buffer (one all-reduce / norm / scale)
        return {name: (g[field] if l is None else g[field][l]) for name, field, l in self._state_names()}

    def _state_names(self):
        """(state_dict key, C-API field, layer or None) for every trainable tensor of the score network (built once)."""
        names = getattr(self, "_state_names_cache", None)
        if names is None:
            cfg = self.cfg
            names = [("model.basis_fn.1.weight", "basis_w1", None), ("model.basis_fn.1.bias", "basis_b1", None),
                     ("model.basis_fn.3.weight", "basis_w2", None), ("model.basis_fn.3.bias", "basis_b2", None),
                     ("model.fiber_basis_fn.1.weight", "fiber_w1", None), ("model.fiber_basis_fn.1.bias", "fiber_b1", None),
                     ("model.fiber_basis_fn.3.weight", "fiber_w2", None), ("model.fiber_basis_fn.3.bias", "fiber_b2", None),
                     ("model.x_embedder.weight", "x_embedder_w", None)]
            il = "model.interaction_layers.{}."
            per_layer = {"conv.kernel.weight": "conv_kernel_w", "conv.fiber_kernel.weight": "conv_fiber_w", "conv.bias": "conv_bias",
                         "norm.weight": "norm_w", "norm.bias": "norm_b", "linear_1.weight": "linear1_w",
                         "linear_1.bias": "linear1_b", "linear_2.weight": "linear2_w", "linear_2.bias": "linear2_b"}
            if cfg.has_layer_scale:
                per_layer["layer_scale"] = "layer_scale"
            for l in range(cfg.num_layers):
                for key, field in per_layer.items():
                    names.append((il.format(l) + key, field, l))
                names.append((f"model.read_out_layers.{l}.weight", "readout_w", l))
                names.append((f"model.read_out_layers.{l}.bias", "readout_b", l))
            self._state_names_cache = names
        return names

    def update_train_weights(self, module):
        """After an optimizer step: push the module's updated parameters (device tensors) into the plain fp32 weights the
        training entry points read (arreau_model_update_train_weights; device-to-device, no host repack).  The engine is
        then `stale_for_sampling` until it is rebuilt.

        The stacked [L, ...] operands of the C API live in persistent buffers, filled by ONE multi-tensor copy from the
        parameters (round 4: state_dict() + 70 conversions + 13 torch.stack per step were 0.5 ms of host time in a step whose
        host side had become the bottleneck)."""
        dev = self.device
        plan = getattr(self, "_train_weight_plan", None)
        params = getattr(module, "_named_parameter_cache", None)
        if params is None:
            params = dict(module.named_parameters())
        if plan is None or plan["module"] is not module or any(p.data_ptr() != q for p, q in zip(plan["src"], plan["ptrs"])):
            L = self.cfg.num_layers
            bufs, dst, src = {}, [], []
            for name, field, l in self._state_names():
                p = params[name]
                if field not in bufs:
                    bufs[field] = torch.empty(((L,) if l is not None else ()) + tuple(p.shape), device=dev, dtype=torch.float32)
                dst.append(bufs[field] if l is None else bufs[field][l])
                src.append(p)
            csd = _hip.StateDict()
            for name in _hip._SD_FIELDS:
                t = bufs.get(name)
                setattr(csd, name, t.data_ptr() if t is not None else None)
            plan = {"module": module, "bufs": bufs, "dst": dst, "src": src, "ptrs": [p.data_ptr() for p in src], "csd": csd}
            self._train_weight_plan = plan
        with torch.no_grad():
            torch._foreach_copy_(plan["dst"], [p.detach() for p in plan["src"]])
        _hip.check(_hip.lib().arreau_model_update_train_weights(self._handle, ctypes.byref(plan["csd"]), _hip.stream_ptr(dev)),
                   "arreau_model_update_train_weights")
        self.stale_for_sampling = not self._general

    def train_weight_mirrors(self, module):
        """{parameter: device address of the engine's own fp32 copy of it} for the optimizer's second destination
        (arreau_model_train_weight_pointers; arreau_amd/optim.py) -- every trainable tensor of the score network except the two the
        training entry points read in a derived form."""
        cached = getattr(self, "_mirror_cache", None)
        params = getattr(module, "_named_parameter_cache", None)
        if params is None:
            params = dict(module.named_parameters())
        if cached is not None and cached[0] is module and all(p.data_ptr() == q for p, q in cached[2]):
            return cached[1]
        csd = _hip.StateDict()
        _hip.check(_hip.lib().arreau_model_train_weight_pointers(self._handle, ctypes.byref(csd)), "arreau_model_train_weight_pointers")
        mirrors = {}
        for name, field, l in self._state_names():
            base = getattr(csd, field)
            p = params[name]
            if base:
                mirrors[p] = int(base) + 4 * p.numel() * (l or 0)
        self._mirror_cache = (module, mirrors, [(p, p.data_ptr()) for p in mirrors])
        return mirrors

    def refresh_derived_train_weights(self, module):
        """After an optimizer step that wrote the engine's copies itself (ClipAdam.step_flat with `mirrors`): rebuild the folded
        polynomial weight and the transposed embedder from the module's updated tensors (two small launches)."""
        params = getattr(module, "_named_parameter_cache", None)
        if params is None:
            params = dict(module.named_parameters())
        _hip.check(_hip.lib().arreau_model_refresh_derived_train_weights(
            self._handle, _hip.ptr(params["model.basis_fn.1.weight"].detach()), _hip.ptr(params["model.x_embedder.weight"].detach()),
            _hip.stream_ptr(self.device)), "arreau_model_refresh_derived_train_weights")
        self.stale_for_sampling = not self._general

    def conv_stats(self):
        """[L,3] unbiased std of (x, x_1, x_2) per layer from the last train_forward (FiberBundleConv.callibrate)."""
        st = torch.empty((self.cfg.num_layers, 3), device=self.device, dtype=torch.float32)
        _hip.check(_hip.lib().arreau_train_conv_stats(self._handle, _hip.ptr(st), _hip.stream_ptr(self.device)),
                   "arreau_train_conv_stats")
        return st

    def workspace(self, N, B):
        if self._ws is None or N > self._ws_cap[0] or B > self._ws_cap[1]:
            capN, capB = max(N, self._ws_cap[0]), max(B, self._ws_cap[1])
            nbytes = _hip.lib().arreau_workspace_bytes(ctypes.byref(self.cfg), capN, capB)
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws_cap = (capN, capB)
        return self._ws

    def predict_scores(self, frac, types, lengths, angles, t_crystal, offsets, edges=None, return_edges=False):
        """frac [N,3] f32, types [N] i32, lengths/angles [B,3] f32, t_crystal [B] i32, offsets [B+1] i32 (device).
        edges = (deg [N] i32, src [N,k] i32, dir [N,k,3] f32, dist [N,k] f32) teacher-forces the graph.
        Returns (eps [N,3], logits [N,S], len0 [B,3]) [+ edges]."""
        dev = self.device
        N, B = frac.shape[0], lengths.shape[0]
        eps = torch.empty((N, 3), device=dev, dtype=torch.float32)
        logits = torch.empty((N, self.S), device=dev, dtype=torch.float32)
        len0 = torch.empty((B, 3), device=dev, dtype=torch.float32)
        ws = self.workspace(N, B)
        if edges is not None:
            deg, src, direction, dist = edges
            given = 1
        elif return_edges:
            k = self.k
            deg = torch.empty(N, device=dev, dtype=torch.int32)
            src = torch.empty((N, k), device=dev, dtype=torch.int32)
            direction = torch.empty((N, k, 3), device=dev, dtype=torch.float32)
            dist = torch.empty((N, k), device=dev, dtype=torch.float32)
            given = 0
        else:
            deg = src = direction = dist = None
            given = 0
        _hip.check(_hip.lib().arreau_predict_scores(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(t_crystal),
            _hip.ptr(offsets), B, N, given, _hip.ptr(deg), _hip.ptr(src), _hip.ptr(direction), _hip.ptr(dist),
            _hip.ptr(eps), _hip.ptr(logits), _hip.ptr(len0), _hip.ptr(ws), ws.numel(), _hip.stream_ptr(dev)),
            "arreau_predict_scores")
        if return_edges:
            return eps, logits, len0, (deg, src, direction, dist)
        return eps, logits, len0

    def reverse_step(self, frac, types, lengths, angles, t_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                     u_types, lattice_out):
        """In-place update of (frac, types, lengths); lattice_out [B,3,3] receives the new cell."""
        B, N = lengths.shape[0], frac.shape[0]
        _hip.check(_hip.lib().arreau_reverse_step(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(t_crystal),
            _hip.ptr(offsets), B, N, _hip.ptr(eps), _hip.ptr(logits), _hip.ptr(len0), _hip.ptr(z_lattice),
            _hip.ptr(z_frac), _hip.ptr(u_types), _hip.ptr(lattice_out), _hip.stream_ptr(self.device)),
            "arreau_reverse_step")

    def _reverse_step_to(self, name, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                         u_types, lattice_out, lattice_clipmax, *options):
        """arreau_reverse_step_to / _tied / _sym: the arguments they share, then each one's own options."""
        B, N = lengths.shape[0], frac.shape[0]
        _hip.check(getattr(_hip.lib(), name)(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(t_crystal),
            _hip.ptr(s_crystal), _hip.ptr(offsets), B, N, _hip.ptr(eps), _hip.ptr(logits), _hip.ptr(len0), _hip.ptr(z_lattice),
            _hip.ptr(z_frac), _hip.ptr(u_types), _hip.ptr(lattice_out), float(lattice_clipmax), *options,
            _hip.stream_ptr(self.device)), name)

    def reverse_step_to(self, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                        u_types, lattice_out, lattice_clipmax=0.999):
        """reverse_step from timestep t_crystal[b] to s_crystal[b] (arreau_reverse_step_to: a respaced step)."""
        self._reverse_step_to("arreau_reverse_step_to", frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0,
                              z_lattice, z_frac, u_types, lattice_out, lattice_clipmax)

    def reverse_step_tied(self, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                          u_types, lattice_out, length_tie, lattice_clipmax=0.999):
        """reverse_step_to with the lattice-system tie of the lengths (arreau_reverse_step_tied): length_tie [B] int32 codes."""
        self._check_tie(length_tie, lengths.shape[0])
        self._reverse_step_to("arreau_reverse_step_tied", frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0,
                              z_lattice, z_frac, u_types, lattice_out, lattice_clipmax, _hip.ptr(length_tie))

    def reverse_step_sym(self, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                         u_types, lattice_out, length_tie, symmetry, lattice_clipmax=0.999):
        """reverse_step_tied with space-group symmetry (arreau_reverse_step_sym): `symmetry` the dict of symmetry.device_arrays
        (None: the tied step); length_tie may be None."""
        self._check_tie(length_tie, lengths.shape[0])
        sym = self._symmetry_struct(symmetry, frac.shape[0]) if symmetry is not None else None
        self._reverse_step_to("arreau_reverse_step_sym", frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0,
                              z_lattice, z_frac, u_types, lattice_out, lattice_clipmax, _hip.ptr(length_tie), _byref(sym))

    def reverse_step_eta(self, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                         u_types, lattice_out, eta, length_tie=None, lattice_clipmax=0.999):
        """reverse_step_tied as the DDIM-style step (arreau_reverse_step_eta): `eta` in [0, 1] scales the noise of positions and
        lengths; length_tie may be None; at eta = 0 z_lattice and z_frac are not read and may be None."""
        eta = check_eta(eta)
        self._check_tie(length_tie, lengths.shape[0])
        self._reverse_step_to("arreau_reverse_step_eta", frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0,
                              z_lattice, z_frac, u_types, lattice_out, lattice_clipmax, _hip.ptr(length_tie), ctypes.c_float(eta))

    def reverse_step_multistep(self, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, u_types, lattice_out,
                               history, length_tie=None, lattice_clipmax=0.999):
        """reverse_step_eta at eta = 0 as the second-order multistep step (arreau_reverse_step_multistep): `history` the dict of
        multistep.allocate_history, read and overwritten; no position or length draw is read; length_tie may be None."""
        self._check_tie(length_tie, lengths.shape[0])
        ms = self._multistep_struct(history, frac.shape[0], lengths.shape[0])
        self._reverse_step_to("arreau_reverse_step_multistep", frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits,
                              len0, None, None, u_types, lattice_out, lattice_clipmax, _hip.ptr(length_tie), _byref(ms))

    def reverse_step_species(self, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                             u_types, lattice_out, species, length_tie=None, symmetry=None, eta=None, multistep=None,
                             lattice_clipmax=0.999):
        """The step of reverse_step_tied / _sym / _eta / _multistep (whichever `symmetry`, `eta`, `multistep` name) under species
        control (arreau_reverse_step_species): `species` the pair (allow, temperature) of sample_loop_species.  u_types may be
        None at a temperature of 0; z_lattice and z_frac at eta = 0 or with multistep."""
        B, N = lengths.shape[0], frac.shape[0]
        self._check_tie(length_tie, B)
        sym = self._symmetry_struct(symmetry, N) if symmetry is not None else None
        ms = self._multistep_struct(multistep, N, B) if multistep is not None else None
        eta_c = ctypes.c_float(float(eta)) if eta is not None else None
        self._reverse_step_to("arreau_reverse_step_species", frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits,
                              len0, z_lattice, z_frac, u_types, lattice_out, lattice_clipmax, _hip.ptr(length_tie), _byref(sym),
                              _byref(eta_c), _byref(ms), _byref(self._species_struct(species, B)))

    def predictor_step(self, frac, types, lengths, angles, t_crystal, s_crystal, offsets, eps, logits, len0, z_lattice, z_frac,
                       u_types, lattice_out, successor, scheduled=True, length_tie=None, eta=None, multistep=None, species=None,
                       lattice_clipmax=0.999):
        """The predictor step of the host-noise loop through the step export its options name, first match: `species` (whichever
        step the other options name, under it), `multistep`, `eta`, `length_tie`, else reverse_step when the run has no schedule
        (scheduled=False), else reverse_step_to.  `successor`: the level every crystal lands on (t - 1 without a schedule), written
        to the caller's buffer s_crystal [B] i32 for every export but the plain reverse_step, which takes none."""
        state, outputs, draws = (frac, types, lengths, angles, t_crystal), (offsets, eps, logits, len0), (z_lattice, z_frac, u_types)
        if species is None and multistep is None and eta is None and length_tie is None and not scheduled:
            return self.reverse_step(*state, *outputs, *draws, lattice_out)
        s_crystal.fill_(successor)
        if species is not None:
            self.reverse_step_species(*state, s_crystal, *outputs, *draws, lattice_out, species, length_tie=length_tie,
                                      eta=eta if multistep is None else None, multistep=multistep, lattice_clipmax=lattice_clipmax)
        elif multistep is not None:  # (the eta = 0 step extrapolated with the history: no z is read)
            self.reverse_step_multistep(*state, s_crystal, *outputs, u_types, lattice_out, multistep, length_tie, lattice_clipmax)
        elif eta is not None:
            self.reverse_step_eta(*state, s_crystal, *outputs, *draws, lattice_out, eta, length_tie, lattice_clipmax)
        elif length_tie is not None:
            self.reverse_step_tied(*state, s_crystal, *outputs, *draws, lattice_out, length_tie, lattice_clipmax)
        else:
            self.reverse_step_to(*state, s_crystal, *outputs, *draws, lattice_out, lattice_clipmax)

    def resample_jump(self, frac, types, lengths, angles, s_crystal, t_crystal, offsets, z_frac, z_lengths, u_types, lattice_out,
                      const_types=None, fixed_lengths=None, condition=None, length_tie=None):
        """One RePaint jump of the whole state from timestep s_crystal[b] up to t_crystal[b] (arreau_resample_jump), in place,
        with the caller's noise: z_frac [N,3] and z_lengths [B,3] standard normal, u_types [N,S] uniform.  Held: const_types,
        fixed_lengths, and the species of `condition`'s type mask (a dict as in sample_loop).  `length_tie`: the lattice-system
        tie codes [B] int32 (arreau_resample_jump_tied); None is the jump without them."""
        B, N = lengths.shape[0], frac.shape[0]
        cond = self._condition_struct(condition, N, B) if condition is not None else None
        self._check_tie(length_tie, B)
        name, tie = "arreau_resample_jump", ()
        if length_tie is not None:
            name, tie = "arreau_resample_jump_tied", (_hip.ptr(length_tie),)
        _hip.check(getattr(_hip.lib(), name)(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(s_crystal),
            _hip.ptr(t_crystal), _hip.ptr(offsets), B, N, _hip.ptr(z_frac), _hip.ptr(z_lengths), _hip.ptr(u_types),
            _hip.ptr(const_types), _hip.ptr(fixed_lengths), _byref(cond), _hip.ptr(lattice_out), *tie,
            _hip.stream_ptr(self.device)), name)

    def noise_state(self, frac, types, lengths, angles, offsets, t, seed, lattice_out, const_types=None, fixed_lengths=None,
                    length_tie=None, crystal_seeds=None):
        """Forward noising of a clean state to level t in place (arreau_noise_state; rules in include/arreau_hip.h): the jump
        (0, t) of every crystal with Philox draws (seed, t, kinds 6 / 7 / 8, element, word3 = 0).  Held: const_types,
        fixed_lengths; `length_tie` ties the lengths (int32 [B] codes).  `crystal_seeds`: keyed sampling
        (arreau_noise_state_keyed): the draws keyed by every crystal's stream seed, elements counted within it."""
        B, N = lengths.shape[0], frac.shape[0]
        self._check_tie(length_tie, B)
        name, keyed = "arreau_noise_state", ()
        if crystal_seeds is not None:
            self._check_seeds(crystal_seeds, B)
            name, keyed = "arreau_noise_state_keyed", (_hip.ptr(crystal_seeds),)
        _hip.check(getattr(_hip.lib(), name)(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(offsets), B, N, int(t),
            int(seed) & (2 ** 64 - 1), _hip.ptr(const_types), _hip.ptr(fixed_lengths), _hip.ptr(lattice_out), _hip.ptr(length_tie),
            *keyed, _hip.stream_ptr(self.device)), name)

    def invert_step(self, frac, types, lengths, angles, s_crystal, t_crystal, offsets, eps, len0, lattice_out, fixed_lengths=None):
        """One DDIM inversion step in place on (frac, lengths), per crystal from level s_crystal[b] up to t_crystal[b], on the
        network outputs eps [N,3] and len0 [B,3] at s (arreau_invert_step); `types` is neither read nor written."""
        B, N = lengths.shape[0], frac.shape[0]
        _hip.check(_hip.lib().arreau_invert_step(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(s_crystal),
            _hip.ptr(t_crystal), _hip.ptr(offsets), B, N, _hip.ptr(eps), _hip.ptr(len0), _hip.ptr(fixed_lengths),
            _hip.ptr(lattice_out), _hip.stream_ptr(self.device)), "arreau_invert_step")

    def invert_loop(self, frac, types, lengths, angles, offsets, t_first, n_steps, up_table, lattice_out, use_graph=False,
                    fixed_lengths=None):
        """n_steps DDIM inversion steps in one library call (arreau_invert_loop): the state at level t_first climbs along
        `up_table`, the device int32 [T+1] table of inversion.ascending_table; in-place update of (frac, lengths), `types` is
        read only.  One network evaluation per step.  t_first must be a level whose "one below" entry the table holds
        (up_table[t_first - 1] == t_first): ascending_table writes it for every level it is given, so a climb may be cut into
        calls at any of them; another entry is clamped and flagged on the device."""
        _require("", "up_table", up_table, (int(self.cfg.num_timesteps) + 1,), torch.int32, self.device)
        N, B = frac.shape[0], lengths.shape[0]
        ws = self.workspace(N, B)
        _hip.check(_hip.lib().arreau_invert_loop(
            self._handle, _hip.ptr(frac), _hip.ptr(types), _hip.ptr(lengths), _hip.ptr(angles), _hip.ptr(offsets), B, N,
            int(t_first), int(n_steps), _hip.ptr(up_table), _hip.ptr(fixed_lengths), _hip.ptr(lattice_out), _hip.ptr(ws), ws.numel(),
            int(bool(use_graph)), _hip.stream_ptr(self.device)), "arreau_invert_loop")

    def _on_device(self, what, frac):
        if frac.device != self.device:
            raise ValueError(f"{what}: the state must be on {self.device}")

    def screen(self, frac, lattice, offsets, types=None, criteria=None):
        """The structural screen of a batch on this engine's device (arreau_crystal_screen; diffusion/screening.py: `screen`,
        which needs no engine): frac [N,3] f32, lattice [B,3,3] f32, offsets [B+1] i32, types [N] i32 or None, criteria a
        ScreenCriteria (None: the defaults; mask_type None: no species check).  One launch on the current stream; returns the
        dict of device tensors min_distance, pair, n_close, volume, number_density, flags, valid."""
        self._on_device("screen", frac)
        return screening.screen(frac, lattice, offsets, types, criteria)

    def reduce_cells(self, frac, lattice, offsets, types, params=None):
        """The cell reduction of a batch on this engine's device (arreau_crystal_reduce; diffusion/cell_reduction.py:
        `reduce_cells`, which needs no engine): frac [N,3] f32, lattice [B,3,3] f32, offsets [B+1] i32, types [N] i32, params a
        CellReductionParams or None (the defaults).  Returns its dict of device tensors; does not synchronise."""
        self._on_device("reduce_cells", frac)
        return cell_reduction.reduce_cells(frac, lattice, offsets, types, params)

    def symmetrize(self, frac, lattice, offsets, types, params=None, found=None):
        """The symmetrization of a batch on this engine's device (arreau_crystal_symmetrize; diffusion/symmetrize.py: `symmetrize`,
        which needs no engine): the batch as for `find_symmetry`, params a SymmetrizeParams or None (the defaults), found the dict
        of `find_symmetry` on the same tensors or None (the search is then launched here).  Returns its dict of device tensors;
        does not synchronise."""
        self._on_device("symmetrize", frac)
        return symmetrize_mod.symmetrize(frac, lattice, offsets, types, params, found)

    def conventional_cell(self, frac, lattice, offsets, types, params=None, reduced=None):
        """The conventional cells of a batch on this engine's device (arreau_crystal_reduce, arreau_crystal_symmetry on the reduced
        batch, arreau_crystal_conventional; diffusion/conventional_cell.py: `conventional_cell`, which needs no engine): the batch as
        for `reduce_cells`, params a ConventionalCellParams or None (the defaults), reduced the dict of `reduce_cells` on the same
        tensors with the same symprec or None (the reduction is then launched here).  Returns its dict of device tensors."""
        self._on_device("conventional_cell", frac)
        return conventional_mod.conventional_cell(frac, lattice, offsets, types, params, reduced)

    def coordination(self, frac, lattice, offsets, params=None):
        """The coordination environments of a batch on this engine's device (arreau_crystal_coordination;
        diffusion/coordination.py: `coordination`, which needs no engine): frac [N,3] f32, lattice [B,3,3] f32, offsets [B+1] i32,
        params a CoordinationParams or None (the defaults).  Returns its dict of device tensors."""
        self._on_device("coordination", frac)
        return coordination_mod.coordination(frac, lattice, offsets, params)

    def bond_order(self, frac, lattice, offsets, params=None, coordination_result=None):
        """The bond angles and Steinhardt order parameters of a batch on this engine's device (arreau_crystal_bond_order;
        diffusion/bond_order.py: `bond_order`, which needs no engine): the coordination launch with `params`, or the given device
        `coordination_result` of a search with those parameters, then the new launch.  Returns the dict of device tensors
        `bond_order` returns.  Does not synchronise."""
        self._on_device("bond_order", frac)
        p = params if params is not None else bond_order_mod.BondOrderParams()
        if coordination_result is None:
            coordination_result = self.coordination(frac, lattice, offsets, p.coordination())
        return bond_order_mod.from_coordination(frac, lattice, offsets, coordination_result, p.max_neighbors)

    def voronoi(self, frac, lattice, offsets, params=None):
        """The Voronoi cells of a batch on this engine's device (arreau_crystal_voronoi; diffusion/voronoi.py: `voronoi`, which
        needs no engine): frac [N,3] f32, lattice [B,3,3] f32, offsets [B+1] i32, params a VoronoiParams or None (the defaults).
        Returns its dict of device tensors.  Does not synchronise."""
        self._on_device("voronoi", frac)
        return voronoi_mod.voronoi(frac, lattice, offsets, params)

    def xrd(self, frac, lattice, offsets, weights_or_atomic_numbers, params=None):
        """The powder diffraction patterns of a batch on this engine's device (arreau_crystal_xrd; diffusion/xrd.py: `xrd`, which
        needs no engine): frac [N,3] f32, lattice [B,3,3] f32, offsets [B+1] i32, the atomic numbers or amplitudes [N] (what
        params.scattering says), params an XrdParams or None (the defaults).  Returns its dict of device tensors.  Does not
        synchronise."""
        self._on_device("xrd", frac)
        return xrd_mod.xrd(frac, lattice, offsets, weights_or_atomic_numbers, params)

    def ewald(self, frac, lattice, offsets, charges_or_atomic_numbers, params=None):
        """The Ewald sums of a batch on this engine's device (arreau_crystal_ewald; diffusion/ewald.py: `ewald`, which needs no
        engine): frac [N,3] f32, lattice [B,3,3] f32, offsets [B+1] i32, the charges [N] (a floating dtype) or the atomic numbers
        [N] (an integer dtype, turned into charges by params.charges), params an EwaldParams.  Returns its dict of device tensors.
        Does not synchronise."""
        self._on_device("ewald", frac)
        return ewald_mod.ewald(frac, lattice, offsets, charges_or_atomic_numbers, params)

    def find_symmetry(self, frac, lattice, offsets, types, params=None):
        """The symmetry search of a batch on this engine's device (arreau_crystal_symmetry; diffusion/symmetry_search.py:
        `find_symmetry`, which needs no engine): frac [N,3] f32, lattice [B,3,3] f32, offsets [B+1] i32, types [N] i32, params
        a SymmetrySearchParams (None: the defaults).  One launch on the current stream; returns the dict of device tensors."""
        self._on_device("find_symmetry", frac)
        return symmetry_search.find_symmetry(frac, lattice, offsets, types, params)

    def edges_to_slots(self, edge_index, dists, direction, N):
        """Receiver-sorted COO edges -> slot form (deg, src, dir, dist)."""
        dev, k = self.device, self.k
        ei = edge_index.to(device=dev, dtype=torch.int64).contiguous()
        E = ei.shape[1]
        d = dists.to(device=dev, dtype=torch.float32).contiguous()
        dr = direction.to(device=dev, dtype=torch.float32).contiguous()
        deg = torch.empty(N, device=dev, dtype=torch.int32)
        src = torch.empty((N, k), device=dev, dtype=torch.int32)
        sdir = torch.empty((N, k, 3), device=dev, dtype=torch.float32)
        sdist = torch.empty((N, k), device=dev, dtype=torch.float32)
        status = torch.zeros(1, device=dev, dtype=torch.int32)
        _hip.check(_hip.lib().arreau_edges_to_slots(_hip.ptr(ei), _hip.ptr(d), _hip.ptr(dr), E, N, k, _hip.ptr(deg),
                                                     _hip.ptr(src), _hip.ptr(sdir), _hip.ptr(sdist), _hip.ptr(status),
                                                     _hip.stream_ptr(dev)), "arreau_edges_to_slots")
        if int(status.item()) != 0:
            raise ValueError(f"edge list must be receiver-sorted with at most {k} in-edges per node")
        return deg, src, sdir, sdist
