"""ctypes binding of libarreau_hip.so (the C ABI declared in include/arreau_hip.h).

There is NO fallback: if the library is missing or a call fails, an exception is raised.
torch is used only for device memory and streams.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p, POINTER, Structure

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ARREAU_HIP_LIB: load another build of the same library (A/B timing of two kernel versions on one box)
LIB_PATH = os.environ.get("ARREAU_HIP_LIB") or os.path.join(_HERE, "csrc", "libarreau_hip.so")

EXPORTS = [
    "arreau_last_error", "arreau_version", "arreau_model_create", "arreau_model_destroy",
    "arreau_model_config", "arreau_workspace_bytes", "arreau_lattice_from_params", "arreau_frac_to_cart",
    "arreau_radius_graph_pbc", "arreau_compact_edges", "arreau_edges_to_slots", "arreau_predict_scores",
    "arreau_reverse_step", "arreau_profile_edge_kernel", "arreau_edge_kernel_time_ms", "arreau_conv_kernel_time_ms",
    "arreau_model_status", "arreau_model_set_variant", "arreau_ponita_forward",
    "arreau_diffusion_noise", "arreau_diffusion_losses", "arreau_sample_loop", "arreau_philox_fill",
    "arreau_train_forward", "arreau_train_backward", "arreau_train_conv_stats", "arreau_model_update_train_weights",
    "arreau_debug_sgemm", "arreau_optimizer_create", "arreau_optimizer_step", "arreau_optimizer_destroy",
    "arreau_model_train_weight_pointers", "arreau_model_refresh_derived_train_weights",
    "arreau_model_set_formats", "arreau_debug_set_pollution", "arreau_debug_leftover_fraction",
    "arreau_sample_loop_conditioned", "arreau_condition_initial_state",
    "arreau_sample_loop_scheduled", "arreau_reverse_step_to",
    "arreau_sample_loop_corrected", "arreau_corrector_step", "arreau_philox_fill_word",
    "arreau_sample_loop_resampled", "arreau_resample_jump", "arreau_optimizer_step_ema",
    "arreau_sample_loop_tied", "arreau_reverse_step_tied", "arreau_resample_jump_tied",
    "arreau_sample_loop_sym", "arreau_reverse_step_sym", "arreau_crystal_screen",
    "arreau_sample_loop_eta", "arreau_reverse_step_eta",
    "arreau_crystal_fingerprint", "arreau_fingerprint_match", "arreau_crystal_symmetry", "arreau_crystal_reduce",
    "arreau_crystal_symmetrize", "arreau_structure_match", "arreau_structure_match_assigned",
    "arreau_crystal_conventional", "arreau_crystal_coordination", "arreau_crystal_bond_order", "arreau_crystal_voronoi", "arreau_crystal_xrd",
    "arreau_noise_state", "arreau_invert_step", "arreau_invert_loop",
    "arreau_sample_loop_multistep", "arreau_reverse_step_multistep",
    "arreau_sample_loop_species", "arreau_reverse_step_species",
    "arreau_diffusion_noise_keyed", "arreau_philox_fill_keyed", "arreau_keyed_timestep", "arreau_diffusion_loss_rows",
    "arreau_loss_rows_reduce",
    "arreau_sample_loop_keyed", "arreau_noise_state_keyed", "arreau_condition_initial_state_keyed", "arreau_philox_fill_crystals",
    "arreau_sample_loop_guided", "arreau_contact_guidance_step",
    "arreau_sample_loop_xrd_guided", "arreau_xrd_guidance_step",
    "arreau_crystal_ewald",
]

STATUS_NONFINITE, STATUS_BAD_TIMESTEP, STATUS_BAD_TYPE, STATUS_BAD_TIE, STATUS_BAD_SYMMETRY = 1, 2, 4, 8, 16
EDGE_KERNELS = {0: "fp32-mfma", 1: "fp32-mfma", 2: "fp32-mfma", 3: "bf16x6", 4: "fp16x3", 5: "general-fp32-gemm"}
MLP_KERNELS = {0: "fp32-mfma", 1: "bf16x6", 2: "fp16x3-32x32x16", 3: "fp16x3-16x16x32",
               5: "general-fp32-gemm"}
VARIANT_GENERAL = 5  # edge variant selecting the shape-general fp32 network (any hidden_dim / basis_dim / widening)


class ArreauHipError(RuntimeError):
    pass


OPT_MAX_GROUPS = 4


class AdamArgs(Structure):
    """arreau_adam_args (include/arreau_hip.h)"""
    _fields_ = [("step", c_int64), ("lr", c_double * OPT_MAX_GROUPS), ("weight_decay", c_double * OPT_MAX_GROUPS),
                ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("max_norm", c_double)]


class SampleConditionC(Structure):
    """arreau_sample_condition (include/arreau_hip.h): device pointers, each may be NULL."""
    _fields_ = [("x0", c_void_p), ("pos_mask", c_void_p), ("a0", c_void_p), ("type_mask", c_void_p), ("l0", c_void_p),
                ("len_mask", c_void_p)]


class SampleScheduleC(Structure):
    """arreau_sample_schedule: the device next-timestep table [T+1] of a respaced loop and VP_lattice's clipmax."""
    _fields_ = [("d_next", c_void_p), ("lattice_clipmax", ctypes.c_float)]


class CorrectorC(Structure):
    """arreau_corrector: M Langevin corrector steps per visited timestep and the SNR of their step-size rule."""
    _fields_ = [("steps", c_int32), ("snr", ctypes.c_float)]


class ResamplingC(Structure):
    """arreau_resampling: R passes per block of J steps, and the host copy of the schedule (block tops and bottoms)."""
    _fields_ = [("passes", c_int32), ("jump_length", c_int32), ("timesteps", POINTER(c_int32)), ("n_timesteps", c_int32)]


class SymmetryC(Structure):
    """arreau_symmetry: the orbit tables of space-group symmetry (device pointers) and their sizes."""
    _fields_ = [(name, c_void_p) for name in ("leader", "op", "orbit", "orbit_ptr", "orbit_atoms", "stab_ptr", "stab_ops", "rot",
                                                "rot_inv", "trans")] + [(name, c_int32) for name in ("n_orbits", "n_orbit_atoms",
                                                                                                     "n_stab_ops", "n_ops")]


class MultistepC(Structure):
    """arreau_multistep: the four history buffers of second-order multistep sampling (device pointers)."""
    _fields_ = [(name, c_void_p) for name in ("hist_eps", "hist_x0", "hist_t_atom", "hist_t_len")]


class SpeciesControlC(Structure):
    """arreau_species_control: the admission rows [B,4] uint32 (device pointer; NULL: every class) and the species temperature."""
    _fields_ = [("d_allow", c_void_p), ("temperature", c_float)]


class ContactGuidanceC(Structure):
    """arreau_contact_guidance: min_distance, weight and max_shells of contact guidance and its three device diagnostic arrays (each
    may be NULL)."""
    _fields_ = [("min_distance", c_float), ("weight", c_float), ("max_shells", c_int32), ("d_energy", c_void_p),
                ("d_contacts", c_void_p), ("d_flags", c_void_p)]


class ScreenCriteriaC(Structure):
    """arreau_screen_criteria: the thresholds of the structural screen."""
    _fields_ = [("min_distance", c_float), ("min_volume", c_float), ("search_radius", c_float), ("mask_type", c_int32),
                ("max_shells", c_int32)]


class ScreenResultC(Structure):
    """arreau_screen_result: the six device arrays the screen writes, one entry per crystal."""
    _fields_ = [(name, c_void_p) for name in ("min_distance", "pair", "n_close", "volume", "number_density", "flags")]


class CoordinationParamsC(Structure):
    """arreau_coordination_params: the tolerance, cutoff and list width of the coordination search."""
    _fields_ = [("tol", c_float), ("cutoff", c_float), ("max_neighbors", c_int32), ("max_shells", c_int32)]


class CoordinationResultC(Structure):
    """arreau_coordination_result: the six per-crystal and six per-atom device arrays the coordination search writes."""
    _fields_ = [(name, c_void_p) for name in ("n_bonds", "n_mutual", "min_cn", "max_cn", "mean_cn", "flags",
                                                "cn", "neighbors", "nearest", "farthest", "mutual", "nearest_d2")]


class BondOrderParamsC(Structure):
    """arreau_bond_order_params: the row width of the neighbour list and the 36 cosine edges of the angle histogram."""
    _fields_ = [("max_neighbors", c_int32), ("cos_edges", c_float * 36)]


class BondOrderResultC(Structure):
    """arreau_bond_order_result: the four per-crystal and six per-atom device arrays the bond-order launch writes."""
    _fields_ = [(name, c_void_p) for name in ("mean_q", "n_angles", "angle_hist", "flags",
                                                "n_used", "q", "q2", "cos_min", "cos_max", "angles")]


class VoronoiParamsC(Structure):
    """arreau_voronoi_params: the weight threshold, cutoff and caps of the Voronoi construction."""
    _fields_ = [("tol", c_float), ("cutoff", c_float), ("max_faces", c_int32), ("max_candidates", c_int32), ("max_shells", c_int32)]


class VoronoiResultC(Structure):
    """arreau_voronoi_result: the seven per-crystal and eleven per-atom device arrays the Voronoi launch writes."""
    _fields_ = [(name, c_void_p) for name in ("n_faces", "min_cn", "max_cn", "mean_cn", "mean_cn_eff", "volume_sum", "flags",
                                                "cn", "neighbors", "face_weight", "face_solid_angle", "face_area", "face_distance",
                                                "volume", "omega_sum", "max_radius", "cn_eff", "atom_flags")]


class XrdParamsC(Structure):
    """arreau_xrd_params: the wavelength, the 2 theta grid, the peak width, the Debye-Waller B and the index cap of the powder pattern."""
    _fields_ = [("wavelength", c_double), ("two_theta_min", c_double), ("two_theta_max", c_double), ("fwhm", c_double), ("b_iso", c_double),
                ("n_points", c_int32), ("max_index", c_int32)]


class XrdResultC(Structure):
    """arreau_xrd_result: the pattern [B, n_points] and the four per-crystal device arrays the diffraction launch writes."""
    _fields_ = [(name, c_void_p) for name in ("pattern", "n_reflections", "volume", "weight_sum", "flags")]


class EwaldParamsC(Structure):
    """arreau_ewald_params: the accuracy, the splitting parameter (0: per crystal) and the two caps of the Ewald sum."""
    _fields_ = [("accuracy", c_double), ("alpha", c_double), ("max_shells", c_int32), ("max_index", c_int32)]


class EwaldResultC(Structure):
    """arreau_ewald_result: the eleven per-crystal device arrays the Ewald launch writes, the potential [N] and its scratch [N]."""
    _fields_ = [(name, c_void_p) for name in ("energy", "real", "reciprocal", "self", "background", "net_charge", "alpha", "volume",
                                                "n_pairs", "n_reciprocal", "flags", "potential", "work")]


class XrdGuidanceC(Structure):
    """arreau_xrd_guidance: the xrd parameters, the weight, the target patterns [B, n_points], the class or atom amplitudes (one of
    them NULL) and the three device diagnostic arrays (each may be NULL)."""
    _fields_ = [("params", XrdParamsC), ("weight", c_float), ("d_target", c_void_p), ("d_class_weights", c_void_p),
                ("d_atom_weights", c_void_p), ("d_distance", c_void_p), ("d_reflections", c_void_p), ("d_flags", c_void_p)]


class FingerprintParamsC(Structure):
    """arreau_fingerprint_params: the radial grid and smearing of the structure fingerprint."""
    _fields_ = [("r_max", c_float), ("sigma", c_float), ("n_bins", c_int32), ("max_shells", c_int32)]


class FingerprintResultC(Structure):
    """arreau_fingerprint_result: the four device arrays of a fingerprinted set, one row per crystal."""
    _fields_ = [(name, c_void_p) for name in ("fingerprint", "species", "counts", "flags")]


class MatchResultC(Structure):
    """arreau_match_result: the four device arrays the match writes, one entry per crystal of X."""
    _fields_ = [(name, c_void_p) for name in ("duplicate_of", "distance", "nearest", "nearest_distance")]


class SymmetryParamsC(Structure):
    """arreau_symmetry_params: the tolerance of the symmetry search and the operations stored per crystal."""
    _fields_ = [("symprec", c_float), ("max_ops", c_int32)]


class SymmetryResultC(Structure):
    """arreau_symmetry_result: the nine device arrays the symmetry search writes, one row per crystal."""
    _fields_ = [(name, c_void_p) for name in ("n_lattice", "n_ops", "n_translations", "ops_rotation", "ops_translation",
                                                "ops_residual", "residual", "point_group", "flags")]


class ReduceParamsC(Structure):
    """arreau_reduce_params: the tolerance of the cell reduction."""
    _fields_ = [("symprec", c_float)]


class ReduceResultC(Structure):
    """arreau_reduce_result: the seven per-crystal and three per-atom device arrays the cell reduction writes."""
    _fields_ = [(name, c_void_p) for name in ("multiplicity", "n_translations", "lattice_out", "transform", "n_out", "flags",
                                                "selling_steps", "frac_out", "types_out", "keep")]


class SymmetrizeResultC(Structure):
    """arreau_symmetrize_result: the device arrays the symmetrization writes (per crystal, per atom, per operation)."""
    _fields_ = [(name, c_void_p) for name in ("frac_out", "lattice", "lengths", "angles", "orbit", "orbit_size", "site_order", "n_orbits",
                                                "max_displacement", "rms_displacement", "ops_translation", "ops_shift", "partner", "flags")]


class ConventionalResultC(Structure):
    """arreau_conventional_result: the nine per-crystal and three per-atom device arrays the conventional-cell launch writes."""
    _fields_ = [(name, c_void_p) for name in ("lattice", "lengths", "angles", "transform", "centring", "bravais", "n_points", "num_atoms",
                                                "flags", "frac_out", "types_out", "source")]


class StructureMatchParamsC(Structure):
    """arreau_structure_match_params: the tolerances of the structure match and the lattice mappings tried per pair."""
    _fields_ = [("ltol", c_float), ("angle_tol", c_float), ("stol", c_float), ("max_mappings", c_int32)]


class StructureMatchResultC(Structure):
    """arreau_structure_match_result: the device arrays the structure match writes, one row per pair, and the row width of partner."""
    _fields_ = [(name, c_void_p) for name in ("rms", "rms_norm", "max_dist", "mapping", "translation", "partner", "n_mappings",
                                                "n_candidates", "n_permutations", "matched", "flags", "scratch")] + [("partner_stride", c_int32)]


class Config(Structure):
    _fields_ = [
        ("num_atomic_states", c_int32), ("hidden_dim", c_int32), ("basis_dim", c_int32),
        ("num_layers", c_int32), ("num_ori", c_int32), ("widening_factor", c_int32), ("degree", c_int32),
        ("max_neighbors", c_int32), ("num_timesteps", c_int32), ("radius", c_float),
        ("has_layer_scale", c_int32),
    ]


class Status(Structure):
    _fields_ = [("flags", c_int32), ("edge_kernel", c_int32), ("mlp_kernel", c_int32), ("conv_kernel", c_int32),
                ("basis_row_bytes", c_int32), ("conv_cross_fp8", c_int32), ("edge_activation_bound", c_float), ("node_activation_bound", c_float),
                ("basis_fp8_share", c_float), ("cross_fp8_share", c_float), ("readout_kernel", c_int32)]


_SD_FIELDS = [
    "basis_w1", "basis_b1", "basis_w2", "basis_b2", "fiber_w1", "fiber_b1", "fiber_w2", "fiber_b2",
    "x_embedder_w", "conv_kernel_w", "conv_fiber_w", "conv_bias", "norm_w", "norm_b", "linear1_w",
    "linear1_b", "linear2_w", "linear2_b", "layer_scale", "readout_w", "readout_b", "ori_grid", "t_emb_w",
    "ve_sigmas", "vp_alpha_bars", "vp_betas", "q_one_step_transposed", "q_mats",
]


class StateDict(Structure):
    _fields_ = [(name, c_void_p) for name in _SD_FIELDS]


def _prototypes():
    """{symbol: argtypes} of every export.  Each sampling entry point is the one before it plus one option in front of the stream."""
    vp, i32, i64, u32, u64, f32, f64 = c_void_p, c_int32, c_int64, ctypes.c_uint32, ctypes.c_uint64, c_float, c_double
    cond, sched, corr, res, sym = (POINTER(t) for t in (SampleConditionC, SampleScheduleC, CorrectorC, ResamplingC, SymmetryC))
    ms = POINTER(MultistepC)
    spec, f32p, guide, xguide = POINTER(SpeciesControlC), POINTER(c_float), POINTER(ContactGuidanceC), POINTER(XrdGuidanceC)
    loop = [vp] * 6 + [i32] * 4 + [u64] + [vp] * 4 + [c_size_t, i32]
    step_to = [vp] * 8 + [i32, i32] + [vp] * 7 + [f32]
    jump = [vp] * 8 + [i32, i32] + [vp] * 5 + [cond, vp]
    adam = [vp] * 4 + [POINTER(AdamArgs), vp]
    return {
        "arreau_last_error": [], "arreau_version": [],
        "arreau_model_create": [POINTER(Config), POINTER(StateDict), vp, POINTER(vp)],
        "arreau_model_destroy": [vp],
        "arreau_model_config": [vp, POINTER(Config)],
        "arreau_workspace_bytes": [POINTER(Config), i64, i64],
        "arreau_lattice_from_params": [vp, vp, i32, vp, vp],
        "arreau_frac_to_cart": [vp, vp, vp, i32, i32, vp, vp],
        "arreau_radius_graph_pbc": [vp, vp, vp, i32, i32, f32, i32] + [vp] * 6,
        "arreau_compact_edges": [vp] * 5 + [i32, i32] + [vp] * 6,
        "arreau_edges_to_slots": [vp, vp, vp, i64, i32, i32] + [vp] * 6,
        "arreau_predict_scores": [vp] * 7 + [i32, i32, i32] + [vp] * 7 + [vp, c_size_t, vp],
        "arreau_reverse_step": [vp] * 7 + [i32, i32] + [vp] * 8,
        "arreau_model_status": [vp, POINTER(Status), i32, vp],
        "arreau_model_set_variant": [vp, i32, i32],
        "arreau_model_set_formats": [vp, i32, i32],
        "arreau_ponita_forward": [vp] * 5 + [i32, i32] + [vp] * 7 + [vp, c_size_t, vp],
        "arreau_diffusion_noise": [vp] * 6 + [i32, i32] + [vp] * 11,
        "arreau_diffusion_losses": [vp] * 10 + [i32, i32] + [vp] * 6,
        "arreau_diffusion_noise_keyed": [vp] * 5 + [i32, i32, u64, vp, i32, vp, i32] + [vp] * 9,
        "arreau_philox_fill_keyed": [u64, i32, i32, u32, i64, vp, vp, vp],
        "arreau_keyed_timestep": [u32, i32, i32, i32, POINTER(i32)],
        "arreau_diffusion_loss_rows": [vp] * 10 + [i32, i32] + [vp] * 5 + [vp, vp, i64, vp],
        "arreau_loss_rows_reduce": [vp, i64, i32, i32, vp, vp, vp],
        "arreau_sample_loop": loop + [vp],
        "arreau_sample_loop_conditioned": loop + [cond, vp],
        "arreau_sample_loop_scheduled": loop + [cond, sched, vp],
        "arreau_sample_loop_corrected": loop + [cond, sched, corr, vp],
        "arreau_sample_loop_resampled": loop + [cond, sched, corr, res, vp],
        "arreau_sample_loop_tied": loop + [cond, sched, corr, res, vp, vp],
        "arreau_sample_loop_sym": loop + [cond, sched, corr, res, vp, sym, vp],
        "arreau_sample_loop_eta": loop + [cond, sched, corr, res, vp, f32, vp],
        "arreau_sample_loop_multistep": loop + [cond, sched, corr, res, vp, ms, vp],
        "arreau_reverse_step_multistep": step_to + [vp, ms, vp],
        "arreau_sample_loop_species": loop + [cond, sched, corr, res, vp, sym, f32p, ms, spec, vp],
        "arreau_sample_loop_keyed": loop + [cond, sched, corr, res, vp, sym, f32p, ms, spec, vp, vp],
        "arreau_sample_loop_guided": loop + [cond, sched, corr, res, vp, sym, f32p, ms, spec, vp, guide, vp],
        "arreau_contact_guidance_step": [vp] * 5 + [i32, i32, vp, guide, vp],
        "arreau_sample_loop_xrd_guided": loop + [cond, sched, corr, res, vp, sym, f32p, ms, spec, vp, guide, xguide, vp],
        "arreau_xrd_guidance_step": [vp] * 6 + [i32, i32, vp, xguide, vp, vp],
        "arreau_noise_state_keyed": [vp] * 6 + [i32, i32, i32, u64] + [vp] * 6,
        "arreau_condition_initial_state_keyed": [vp] * 5 + [i32, i32, i32, u64, cond, vp, vp],
        "arreau_philox_fill_crystals": [vp, vp, i32, i32, i32, u32, i32, i32, vp, vp, vp],
        "arreau_reverse_step_species": step_to + [vp, sym, f32p, ms, spec, vp],
        "arreau_condition_initial_state": [vp] * 4 + [i32, i32, i32, u64, cond, vp],
        "arreau_reverse_step_to": step_to + [vp],
        "arreau_reverse_step_tied": step_to + [vp, vp],
        "arreau_reverse_step_sym": step_to + [vp, sym, vp],
        "arreau_reverse_step_eta": step_to + [vp, f32, vp],
        "arreau_corrector_step": [vp] * 4 + [i32, i32, vp, vp, f32, cond, vp],
        "arreau_resample_jump": jump + [vp],
        "arreau_resample_jump_tied": jump + [vp, vp],
        "arreau_noise_state": [vp] * 6 + [i32, i32, i32, u64] + [vp] * 5,
        "arreau_invert_step": [vp] * 8 + [i32, i32] + [vp] * 5,
        "arreau_invert_loop": [vp] * 6 + [i32] * 4 + [vp] * 4 + [c_size_t, i32, vp],
        "arreau_philox_fill": [u64, i32, i32, i64, vp, vp, vp],
        "arreau_philox_fill_word": [u64, i32, i32, u32, i64, vp, vp, vp],
        "arreau_crystal_screen": [vp] * 4 + [i32, i32, POINTER(ScreenCriteriaC), POINTER(ScreenResultC), vp],
        "arreau_crystal_coordination": [vp] * 3 + [i32, i32, POINTER(CoordinationParamsC), POINTER(CoordinationResultC), vp],
        "arreau_crystal_bond_order": [vp] * 3 + [i32, i32, vp, vp, POINTER(BondOrderParamsC), POINTER(BondOrderResultC), vp],
        "arreau_crystal_voronoi": [vp] * 3 + [i32, i32, POINTER(VoronoiParamsC), POINTER(VoronoiResultC), vp],
        "arreau_crystal_xrd": [vp] * 4 + [i32, i32, POINTER(XrdParamsC), POINTER(XrdResultC), vp],
        "arreau_crystal_ewald": [vp] * 4 + [i32, i32, POINTER(EwaldParamsC), POINTER(EwaldResultC), vp],
        "arreau_crystal_fingerprint": [vp] * 4 + [i32, i32, POINTER(FingerprintParamsC), POINTER(FingerprintResultC), vp],
        "arreau_fingerprint_match": [POINTER(FingerprintResultC), i32, POINTER(FingerprintResultC), i32, f32, POINTER(MatchResultC), vp],
        "arreau_crystal_symmetry": [vp] * 4 + [i32, i32, POINTER(SymmetryParamsC), POINTER(SymmetryResultC), vp],
        "arreau_crystal_reduce": [vp] * 4 + [i32, i32, POINTER(ReduceParamsC), POINTER(ReduceResultC), vp],
        "arreau_crystal_symmetrize": [vp] * 4 + [i32, i32, POINTER(SymmetryResultC), i32, POINTER(SymmetrizeResultC), vp],
        "arreau_crystal_conventional": [vp] * 4 + [i32, i32, POINTER(SymmetryResultC), i32, POINTER(ConventionalResultC), vp],
        "arreau_structure_match": ([vp] * 4 + [i32, i32]) * 2 + [vp, i32, POINTER(StructureMatchParamsC), POINTER(StructureMatchResultC), vp],
        "arreau_structure_match_assigned": ([vp] * 4 + [i32, i32]) * 2 + [vp, i32, POINTER(StructureMatchParamsC), POINTER(StructureMatchResultC),
                                            i32, vp, vp],
        "arreau_train_forward": [vp] * 7 + [i32, i32] + [vp] * 4,
        "arreau_train_backward": [vp] * 4 + [POINTER(StateDict), vp],
        "arreau_train_conv_stats": [vp, vp, vp],
        "arreau_debug_sgemm": [i32, i32, i32, i32, vp, i64, i64, vp, i64, i64, vp, i32, f32, f32, vp],
        "arreau_model_update_train_weights": [vp, POINTER(StateDict), vp],
        "arreau_model_train_weight_pointers": [vp, POINTER(StateDict)],
        "arreau_model_refresh_derived_train_weights": [vp, vp, vp, vp],
        "arreau_optimizer_create": [i32, POINTER(vp), POINTER(vp), POINTER(i64), POINTER(i64), POINTER(i32), i32, i64, POINTER(vp)],
        "arreau_optimizer_step": adam + [vp],
        "arreau_optimizer_step_ema": adam + [f64, vp, vp],
        "arreau_optimizer_destroy": [vp],
        "arreau_debug_set_pollution": [u32],
        "arreau_debug_leftover_fraction": [u32, POINTER(f64), POINTER(f64), vp],
        "arreau_profile_edge_kernel": [i32],
        "arreau_edge_kernel_time_ms": [POINTER(f64), POINTER(i64)],
        "arreau_conv_kernel_time_ms": [POINTER(f64), POINTER(i64)],
    }


# every other export returns the int32 error code
_RESTYPES = {"arreau_last_error": c_char_p, "arreau_version": c_char_p, "arreau_model_destroy": None,
             "arreau_workspace_bytes": c_size_t, "arreau_optimizer_destroy": None}

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ArreauHipError(
            f"{LIB_PATH} not found: build it with `python -m arreau_amd.build` (hipcc, gfx950). "
            "arreau_amd has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    prototypes = _prototypes()
    for name in EXPORTS:
        # a missing symbol is tolerated only in another build loaded through ARREAU_HIP_LIB (an older one under test: tools/ab.sh)
        if os.environ.get("ARREAU_HIP_LIB") and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes = prototypes[name]
        fn.restype = _RESTYPES.get(name, c_int32)
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        msg = lib().arreau_last_error().decode(errors="replace")
        raise ArreauHipError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device (or host) address of a contiguous tensor, or NULL for None."""
    if t is None:
        return None
    assert t.is_contiguous(), "arreau_amd passes contiguous tensors only"
    return c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu():
    if not torch.cuda.is_available():
        raise ArreauHipError("arreau_amd needs an AMD GPU (gfx950); there is no CPU fallback.")
