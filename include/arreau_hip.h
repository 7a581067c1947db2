/*
 * arreau_hip.h -- C ABI of libarreau_hip.so: the MI355X (gfx950) implementation of
 * arreau's reverse-diffusion sampling step.
 *
 * The reference (curtischong/arreau) is pure Python; its seams for this path are
 * Python calls.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference checkout).  Conventions:
 *
 *   - all pointers named d_* are DEVICE pointers (HBM), contiguous row-major;
 *     h_* are HOST pointers.  float = fp32, index arrays = int32.
 *   - every launch function enqueues on `stream` (a hipStream_t passed as void*)
 *     and never synchronises, allocates or frees; scratch memory comes from a
 *     caller-owned workspace (arreau_workspace_bytes).
 *   - return value: 0 on success, a negative ARREAU_E* code otherwise;
 *     arreau_last_error() gives a message for the calling thread.
 *   - crystals are described CSR-style by d_crystal_offsets[B+1] (first atom of
 *     each crystal; atoms of one crystal are contiguous, as in the reference's
 *     `num_atoms` convention, diffusion/diffusion_loss.py:308,330-335).
 *   - the neighbour list is kept receiver-major in fixed-width slots:
 *     slot (i, s), s < deg[i] <= k, holds the s-th in-edge of receiver atom i in
 *     the reference's enumeration order (sender, image).  Unused slots hold
 *     src = -1, dir = 0, dist = 0.
 */
#ifndef ARREAU_HIP_H
#define ARREAU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARREAU_OK 0
#define ARREAU_EINVAL (-1)      /* bad argument / unsupported hyper-parameter */
#define ARREAU_EHIP (-2)        /* a HIP runtime call failed */
#define ARREAU_ECAPACITY (-3)   /* workspace too small / slot overflow */

/* Hyper-parameters read from the checkpoint's `args` (lightning_wrappers/diffusion.py:42-54,
 * 86-102; diffusion/diffusion_loss.py:70-72) plus S = len(z_table). */
typedef struct arreau_config {
    int32_t num_atomic_states;  /* S, including the mask state (last class)          */
    int32_t hidden_dim;         /* C  (args.hidden_dim)                              */
    int32_t basis_dim;          /* D  (args.basis_dim)                               */
    int32_t num_layers;         /* L  (args.layers)                                  */
    int32_t num_ori;            /* O  (args.num_ori), must be 16                     */
    int32_t widening_factor;    /* W  (args.widening_factor)                         */
    int32_t degree;             /* polynomial degree (args.degree), must be 3        */
    int32_t max_neighbors;      /* k  (args.max_neighbors), <= ARREAU_MAX_K          */
    int32_t num_timesteps;      /* T  (args.num_timesteps)                           */
    float radius;               /* R  (args.radius)                                  */
    int32_t has_layer_scale;    /* 0 when args.layer_scale == 0 (convnext.py:14-17)  */
} arreau_config;

#define ARREAU_MAX_K 8
#define ARREAU_T_EMB_DIM 64      /* lightning_wrappers/diffusion.py:23 */
#define ARREAU_N_CRYSTAL_FEATS 10 /* n, lengths(3), angles(3), |lengths/n|(3): diffusion_loss.py:139-149 */

/* The network's parameters and the diffusion buffers in the reference's state_dict
 * layout, as HOST fp32 arrays (SURVEY.md section 5 lists the keys).  Per-layer
 * tensors are stacked along a leading L axis. */
typedef struct arreau_state_dict {
    const float* basis_w1;      /* model.basis_fn.1.weight            [C, 258]      */
    const float* basis_b1;      /* model.basis_fn.1.bias              [C]           */
    const float* basis_w2;      /* model.basis_fn.3.weight            [D, C]        */
    const float* basis_b2;      /* model.basis_fn.3.bias              [D]           */
    const float* fiber_w1;      /* model.fiber_basis_fn.1.weight      [C, 3]        */
    const float* fiber_b1;      /* model.fiber_basis_fn.1.bias        [C]           */
    const float* fiber_w2;      /* model.fiber_basis_fn.3.weight      [D, C]        */
    const float* fiber_b2;      /* model.fiber_basis_fn.3.bias        [D]           */
    const float* x_embedder_w;  /* model.x_embedder.weight            [C, S+78]     */
    const float* conv_kernel_w; /* ...interaction_layers.i.conv.kernel.weight        [L, C, D] */
    const float* conv_fiber_w;  /* ...interaction_layers.i.conv.fiber_kernel.weight  [L, C, D] */
    const float* conv_bias;     /* ...interaction_layers.i.conv.bias                 [L, C]    */
    const float* norm_w;        /* ...interaction_layers.i.norm.weight               [L, C]    */
    const float* norm_b;        /* ...interaction_layers.i.norm.bias                 [L, C]    */
    const float* linear1_w;     /* ...interaction_layers.i.linear_1.weight           [L, W*C, C] */
    const float* linear1_b;     /* ...interaction_layers.i.linear_1.bias             [L, W*C]  */
    const float* linear2_w;     /* ...interaction_layers.i.linear_2.weight           [L, C, W*C] */
    const float* linear2_b;     /* ...interaction_layers.i.linear_2.bias             [L, C]    */
    const float* layer_scale;   /* ...interaction_layers.i.layer_scale               [L, C] (NULL if absent) */
    const float* readout_w;     /* model.read_out_layers.i.weight                    [L, S+4, C] */
    const float* readout_b;     /* model.read_out_layers.i.bias                      [L, S+4]  */
    const float* ori_grid;      /* PositionOrientationGraph.ori_grid_s2 (not in the state_dict) [O, 3] */
    const float* t_emb_w;       /* t_emb.gaussian_fourier_proj_w                     [32]      */
    const float* ve_sigmas;     /* diffusion_loss.pos_diffusion.sigmas               [T+1]     */
    const float* vp_alpha_bars; /* diffusion_loss.lattice_diffusion.alpha_bars       [T+1]     */
    const float* vp_betas;      /* diffusion_loss.lattice_diffusion.betas            [T+1]     */
    const float* q_one_step_transposed; /* diffusion_loss.d3pm.q_one_step_transposed [T, S, S] */
    const float* q_mats;        /* diffusion_loss.d3pm.q_mats                        [T, S, S] */
} arreau_state_dict;

typedef struct arreau_model arreau_model; /* opaque: packed weights resident in HBM */

const char* arreau_last_error(void);
const char* arreau_version(void);

/* Replaces PonitaFiberBundle.__init__ + load_state_dict (ponita/models/ponita.py:31-86) and the
 * buffer set-up of DiffusionLoss.__init__ (diffusion/diffusion_loss.py:68-93): folds the 258
 * polynomial columns onto their 83 distinct monomials, repacks every Linear for the MFMA
 * fragment order, uploads, and evaluates the input-independent fiber kernels
 * fiber_kernel(fiber_basis_fn(o_a . o_b)) (ponita.py:95, conv.py:113) once on the GPU.
 * Allocates device memory (the only entry point besides arreau_model_destroy that does).
 * Shapes: the fused sampling kernels exist for hidden_dim 128, basis_dim 256, widening_factor 4 (the shipped
 * checkpoint).  Any other shape with hidden_dim, basis_dim multiples of 4 and widening_factor * hidden_dim <= 1024
 * (e.g. the reference's `make train` preset hidden_dim = 200, Makefile:7) is accepted and runs every entry point --
 * scores, inner seam, sampling loop, training -- on the shape-general fp32 kernels (exact fp32 MFMA GEMMs +
 * element-wise kernels): same results, no fusion.  num_ori = 16, degree = 3, max_neighbors <= 8 are fixed. */
int arreau_model_create(const arreau_config* cfg, const arreau_state_dict* h_sd, void* stream,
                        arreau_model** out_model);
void arreau_model_destroy(arreau_model* model);
int arreau_model_config(const arreau_model* model, arreau_config* out_cfg);

/* Sticky condition bits collected on the device while kernels run (nothing is checked on the host per call, so
 * the launch functions stay asynchronous).  A set bit means results since the last reset must not be trusted:
 *   NONFINITE    a network output (eps, logits, pred_lengths_0) was inf/NaN -- this is how an activation beyond the
 *                fp16 range of the split-precision kernels (|v| >= 65520) surfaces: the planes overflow to inf and the
 *                value propagates as NaN instead of being clamped silently;
 *   BAD_TIMESTEP a timestep outside [0, T] (predict_scores) / [1, T] (reverse_step) was clamped, or a respaced step's
 *                target s outside its range (arreau_reverse_step_to, arreau_sample_loop_scheduled);
 *   BAD_TYPE     an atom-type index outside [0, S) was clamped;
 *   BAD_TIE      a lattice-system tie code outside 0..2 was treated as 0 (arreau_sample_loop_tied and its step / jump);
 *   BAD_SYMMETRY a symmetry table entry was out of range or inconsistent: the atoms it names were updated without symmetry
 *                (arreau_sample_loop_sym, arreau_reverse_step_sym).
 * edge_kernel / mlp_kernel / conv_kernel name the kernel family the last arreau_predict_scores really launched
 * (edge: 0-2 fp32 MFMA, 3 bf16x6, 4 fp16x3; mlp: 0 fp32 MFMA, 1 bf16x6, 2 fp16x3 32x32x16, 3 fp16x3 16x16x32;
 * conv: 0 register form, 1 streamed form, 2 fused into the MLP kernel) -- e.g. 3/1 instead of 4/3 when a weight does not
 * fit fp16.  readout_kernel names the read-out the last arreau_predict_scores launched: 1 the fp32-MFMA kernel (S + 4 <= 96),
 * 0 the vector kernel (readout_nodes_kernel: wider species tables, or ARREAU_READOUT_VARIANT=0), 5 the shape-general path's
 * train_outputs_kernel; -1 none yet.  The reference has no counterpart (Python raises on bad indices: F.one_hot, tensor indexing). */
#define ARREAU_STATUS_NONFINITE 1
#define ARREAU_STATUS_BAD_TIMESTEP 2
#define ARREAU_STATUS_BAD_TYPE 4
#define ARREAU_STATUS_BAD_TIE 8
#define ARREAU_STATUS_BAD_SYMMETRY 16
typedef struct arreau_status {
    int32_t flags;
    int32_t edge_kernel;
    int32_t mlp_kernel;
    int32_t conv_kernel;
    int32_t basis_row_bytes; /* conv_kernel == 2: bytes of the stashed basis per (edge, orientation) row the kernels really used
                              * (768: fp16 plane + fp8 e4m3 residual plane; 1024: two fp16 planes -- ARREAU_BASIS_FP8=0, or a model whose
                              * calibration dropped the fp8 plane); 0 otherwise */
    int32_t conv_cross_fp8;  /* conv_kernel == 2: 1 when the layer projections ran their two cross products on the fp8 matrix instruction
                              * (round 4 default; e4m3 operands, twice the fp16 rate), 0 for three fp16 products (ARREAU_CROSS_FP8=0) */
    float edge_activation_bound; /* bounds, from the weights alone, of every fp16 operand of the split-precision edge chain */
    float node_activation_bound; /* (monomials, hidden units, basis) resp. ConvNext chain (LayerNorm output, hidden units): at most
                                  * 65504 = the fp16x3 kernels provably cannot overflow; up to 64 x that the library keeps them
                                  * and relies on NONFINITE (the host re-runs on bf16x6); beyond, the model starts on bf16x6 */
    float basis_fp8_share;   /* round 5: what arreau_model_create measured on its calibration batch -- the share of the parity bounds
                              * (1e-5 max(1, |eps|), 1e-5 max(1, |logits| / 8)) the fp8 residual plane of the stash, resp. that plane + */
    float cross_fp8_share;   /* the fp8 cross products used up against two fp16 planes + three fp16 products; a format above 0.1 is not
                              * used for this model (basis_row_bytes 1024 / conv_cross_fp8 0 then); -1: not measured */
    int32_t readout_kernel;  /* 1 fp32-MFMA read-out, 0 readout_nodes_kernel, 5 the general path's train_outputs_kernel, -1 not run */
} arreau_status;
/* Reads (and with reset != 0 clears) the status word; synchronises `stream`. */
int arreau_model_status(const arreau_model* model, arreau_status* out, int32_t reset, void* stream);
/* Round 5: selects the operand formats of the message path for this model (-1 keeps the current choice; 0 / 1): the fp8 (e4m3)
 * residual plane of the basis stash and the fp8 cross products of the layer projections (which need that plane and kernel
 * weights inside e4m3's range).  arreau_model_create chooses them from its calibration batch; the host clears both when an
 * evaluation came out non-finite with them on -- the hardware's fp8 conversion returns NaN for a basis value beyond 464 -- and
 * repeats it (HipEngine.checked, DiffusionLoss.sample).  No reference counterpart. */
int arreau_model_set_formats(arreau_model* model, int32_t basis_fp8, int32_t cross_fp8);
/* Selects the arithmetic of the dense kernels for this model (-1 keeps the current choice); the defaults come from
 * the environment (ARREAU_EDGE_VARIANT, ARREAU_MLP_VARIANT) at arreau_model_create.  Used by the parity report and
 * bench.py to time/compare the exact fp32-MFMA kernels against the default fp16x3 ones in one process.
 * mlp_variant 4 forces the small-launch form of the default ConvNext kernel (one node per workgroup, the layer's work dealt
 * to eight waves; bit-identical to variant 3, which picks it by itself for small launches) at every size (tests).
 * edge_variant 5 runs the whole score network on the shape-general fp32 GEMM kernels (what shapes without fused kernels
 * always use; such models accept no other value).  Those kernels read the plain weights
 * arreau_model_update_train_weights refreshes, so with variant 5 a model keeps sampling between optimiser steps. */
int arreau_model_set_variant(arreau_model* model, int32_t edge_variant, int32_t mlp_variant);

/* Scratch for one step over at most max_atoms atoms / max_crystals crystals. */
size_t arreau_workspace_bytes(const arreau_config* cfg, int64_t max_atoms, int64_t max_crystals);

/* ---- small geometric operators ------------------------------------------------------------ */

/* lattice_from_params, diffusion/lattice_helpers.py:55-105.  d_lengths[B,3], d_angles[B,3]
 * (consumed as radians) -> d_lattice[B,3,3]. */
int arreau_lattice_from_params(const float* d_lengths, const float* d_angles, int32_t B,
                               float* d_lattice, void* stream);

/* frac_to_cart_coords, diffusion/diffusion_helpers.py:223-230. */
int arreau_frac_to_cart(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets,
                        int32_t B, int32_t N, float* d_cart, void* stream);

/* radius_graph_pbc(cart, lattice, num_atoms, radius, max_num_neighbors_threshold,
 * remove_self_edges=True), diffusion/diffusion_helpers.py:328-564, in slot form.
 * Outputs: d_deg[N]; d_src[N,k] (global sender index, -1 when unused); d_cell[N,k] image code
 * 0..26 in the reference's SUPERCELLS order (diffusion_helpers.py:10), -1 when unused;
 * d_dir[N,k,3] = pos_sender + image_offset - pos_receiver; d_dist[N,k].
 * A candidate (sender, image) is in range when 1e-4f < d^2 <= (float)((double)radius * radius),
 * d^2 = (dx*dx + dy*dy) + dz*dz in float32 without contraction.  k may be 1 .. 64: per receiver
 * the k in-range candidates with the smallest keys are kept and written in ascending
 * enumeration index c = 27 * (sender - first atom of the crystal) + image; unused slots are
 * cleared.
 * Tie rule (the reference leaves it to an unstable sort): the key is (bits of d^2, c), so among
 * candidates whose float32 d^2 are EQUAL the smaller c wins -- the earlier sender, then the
 * earlier image.  The oracle's radius_graph_pbc(stable_ties=True) states the same rule.
 * Limit: the key holds c in 21 bits, c < 2^21, i.e. at most 77 672 atoms in one crystal
 * (27 * 77 672 = 2 097 144).  The limit is NOT checked: a larger crystal gives a wrong list
 * without a status flag. */
int arreau_radius_graph_pbc(const float* d_cart, const float* d_lattice,
                            const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                            float radius, int32_t k,
                            int32_t* d_deg, int32_t* d_src, int32_t* d_cell, float* d_dir,
                            float* d_dist, void* stream);

/* Slot form -> the reference's return tuple (edge_index[2,E] as (sender, receiver),
 * -unit_cell[E,3], dist[E], direction[E,3]; diffusion_helpers.py:548-555).
 * d_edge_offsets[N+1] is written (exclusive scan of deg); E = d_edge_offsets[N]. Outputs must
 * hold N*k entries. */
int arreau_compact_edges(const int32_t* d_deg, const int32_t* d_src, const int32_t* d_cell,
                         const float* d_dir, const float* d_dist, int32_t N, int32_t k,
                         int32_t* d_edge_offsets, int64_t* d_edge_index /*[2, N*k]*/,
                         float* d_cell_offsets /*[N*k,3]*/, float* d_out_dist, float* d_out_dir,
                         void* stream);

/* Receiver-sorted COO edges (edge_index[1] non-decreasing) -> slot form, for callers that bring
 * their own graph (PonitaFiberBundle.forward takes graph.edge_index, ponita.py:88-106).
 * d_status (int32, device) receives 1 when a receiver has more than k in-edges or the list is
 * not receiver-sorted. */
int arreau_edges_to_slots(const int64_t* d_edge_index /*[2,E]*/, const float* d_dist,
                          const float* d_dir, int64_t E, int32_t N, int32_t k,
                          int32_t* d_deg, int32_t* d_src, float* d_slot_dir, float* d_slot_dist,
                          int32_t* d_status, void* stream);

/* ---- structural screen of generated crystals ---------------------------------------------------------------------
 * Per crystal: the shortest interatomic contact over every periodic image within a search radius, the cell volume and the
 * mask state, against thresholds (the validity screen of CDVAE / DiffCSP / MatterGen; the reference has no counterpart, its
 * post-processing assumes filtered input).  An exact search of its own -- arreau_radius_graph_pbc looks at 27 images only,
 * stops at k and skips d^2 <= 1e-4.  One launch, one workgroup of four waves per crystal, no atomics, no second stream, no
 * arreau_model.  Every arithmetic step below is ONE float32 operation rounded to nearest, in the order written, never
 * contracted to a fused multiply-add, so a float32 host restatement (arreau_amd/diffusion/screening.py) matches bit for bit.
 *   1. cell (rows a_0, a_1, a_2 of d_lattice): c_0 = a_1 x a_2, c_1 = a_2 x a_0, c_2 = a_0 x a_1, each component
 *      u_p v_q - u_q v_p; det = (a_0x c_0x + a_0y c_0y) + a_0z c_0z; volume = |det|; |c_k| = sqrt((c_kx^2 + c_ky^2) + c_kz^2);
 *      plane spacing h_k = volume / |c_k|; number_density = n / volume (n atoms); q_k = search_radius / h_k.
 *   2. NONFINITE: a cell entry or a coordinate of the crystal is inf / NaN.  Nothing else is computed: the three reals are
 *      NaN, pair is -1, n_close 0, no other flag.
 *   3. CELL: not (volume >= min_volume), volume not finite, or not (q_k <= max_shells) for an axis.  The search is skipped:
 *      min_distance is NaN, pair -1, n_close 0; volume, number_density and MASKED are still reported.
 *   4. images per axis n_k = max(1, ceil(q_k)), shifts (n_1, n_2, n_3) with |n_k'| <= n_k in lexicographic order, index
 *      m = ((n_1 + N_1)(2 N_2 + 1) + (n_2 + N_2))(2 N_3 + 1) + (n_3 + N_3).  Two wrapped positions differ by less than one
 *      cell along every axis and a displacement of length <= R has a fractional component of at most R / h_k, so this
 *      range contains every pair within search_radius for any cell shape.
 *   5. positions: w = f - floor(f), a result >= 1 becomes 0; p_d = (w_0 L_0d + w_1 L_1d) + w_2 L_2d -- the expression of
 *      frac_to_cart_coords, on the wrapped coordinates.  Kept in LDS for crystals of up to 256 atoms; larger crystals form
 *      them from global memory where they are used (the same values).
 *   6. contacts: pairs i <= j (local atom indices); for i < j every shift, for i == j only the shifts after (0, 0, 0) in
 *      the order of 4 (an atom meets its own images, each once, never itself).  s_d = (n_1 L_0d + n_2 L_1d) + n_3 L_2d,
 *      disp = (p_j + s) - p_i, d2 = (dx dx + dy dy) + dz dz.
 *   7. the reported contact is the smallest by the key (bits of d2, i, j, m): among equal float32 d2 the smaller i, then the
 *      smaller j, then the earlier shift.  min_distance = sqrt(d2) (correctly rounded); pair = (i, j, n_1, n_2, n_3).
 *      n_close = the number of contacts with d2 < (float)((double)min_distance * min_distance) -- unordered contacts, each
 *      counted once.  The reduction is a wave minimum over the key, then the four waves through LDS: deterministic.
 *   8. flags: CLOSE n_close > 0;  MASKED d_types given, mask_type >= 0 and an atom of the crystal has it;  BEYOND not
 *      (d2_min <= (float)((double)search_radius * search_radius)) -- no contact within the search radius; min_distance is
 *      then the minimum over the enumerated images, an upper bound of the true one only (informational).  A crystal without
 *      atoms has no contact: min_distance +inf, pair -1, BEYOND.  A crystal is VALID when (flags & 15) == 0.
 * Limits: at most 2^24 atoms in one crystal (the key holds i and j in 24 bits each; not checked).  Offsets outside [0, N] or
 * descending are clamped, so a bad table reads no memory outside the arrays.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL criteria / result / arrays, negative sizes, a threshold that is
 * not finite or negative, search_radius <= 0 or below min_distance, max_shells outside 1..ARREAU_SCREEN_MAX_SHELLS,
 * mask_type < -1. */
#define ARREAU_SCREEN_NONFINITE 1
#define ARREAU_SCREEN_CELL 2
#define ARREAU_SCREEN_CLOSE 4
#define ARREAU_SCREEN_MASKED 8
#define ARREAU_SCREEN_BEYOND 16
#define ARREAU_SCREEN_INVALID_MASK 15
#define ARREAU_SCREEN_MAX_SHELLS 8
typedef struct arreau_screen_criteria {
    float min_distance;   /* A; default 0.5 */
    float min_volume;     /* A^3; default 0.1 */
    float search_radius;  /* A; default 3.0, at least min_distance */
    int32_t mask_type;    /* class index of the D3PM mask state, -1: none */
    int32_t max_shells;   /* cap on the images per axis, 1..ARREAU_SCREEN_MAX_SHELLS; default 8 */
} arreau_screen_criteria;
typedef struct arreau_screen_result { /* DEVICE arrays, one entry per crystal */
    float* min_distance;    /* [B]   */
    int32_t* pair;          /* [B,5] i, j (local to the crystal), n_1, n_2, n_3 */
    int32_t* n_close;       /* [B]   */
    float* volume;          /* [B]   */
    float* number_density;  /* [B]   */
    int32_t* flags;         /* [B]   ARREAU_SCREEN_* */
} arreau_screen_result;
/* d_frac[N,3] fractional coordinates (any real: wrapped by rule 5), d_types[N] class indices (may be NULL: no species check),
 * d_lattice[B,3,3] rows a, b, c.  `crit` and `out` are HOST pointers to the structs; the arrays `out` names are device arrays. */
int arreau_crystal_screen(const float* d_frac, const int32_t* d_types /* may be NULL */, const float* d_lattice /* [B,3,3] rows a,b,c */,
                          const int32_t* d_crystal_offsets, int32_t B, int32_t N, const arreau_screen_criteria* crit,
                          arreau_screen_result* out /* device arrays, each [B] (pair: [B,5]) */, void* stream);

/* ---- coordination environments of generated crystals -----------------------------------------------------------------
 * Per atom: its nearest distance over every periodic image, its neighbours -- every atom and image within (1 + tol) times that
 * distance and within a cutoff (the table-free rule pymatgen ships as MinimumDistanceNN; the reference's predict_bonds uses
 * CrystalNN, which weights Voronoi faces and needs radii: not this) --, their number, the first max_neighbors of them and how
 * many of them the other end agrees on; per crystal the sums and extremes.  The screen's exact image search, run per atom over
 * all j.  One launch, one workgroup of four waves per crystal, one wave per atom, no atomics (every reduction is an integer
 * sum or a minimum / maximum of the bits of a non-negative float: no order matters), no arreau_model.  Every arithmetic step is
 * ONE float32 operation rounded to nearest, in the order written, never contracted to a fused multiply-add, so a float32 host
 * restatement (arreau_amd/diffusion/coordination.py) matches bit for bit.
 *   1. cell, NONFINITE, images and positions: the screen's rules 1, 2, 4 and 5 with search_radius = cutoff.  CELL: volume not
 *      finite or not (q_k <= max_shells) for an axis (no volume threshold here).  For NONFINITE and CELL nothing else is
 *      computed: the reals are NaN, neighbors -1, the counts 0, min_cn and max_cn -1, no other flag.
 *   2. distance of receiver i, atom j, image m = (n_1, n_2, n_3): s_d = (n_1 L_0d + n_2 L_1d) + n_3 L_2d, disp = (p_j + s) - p_i,
 *      d2 = (dx dx + dy dy) + dz dz -- the screen's rule 6, for EVERY j (not j >= i) and every m; the pair (j = i, m = (0, 0, 0)) is
 *      the atom itself and is skipped, every other image of i counts.  The search range is e = j M + m, 0 <= e < n M.
 *   3. phase A: d2min(i) = the minimum of the bits of d2 over the range (+inf where it holds no finite d2); written to
 *      nearest_d2; a workgroup barrier follows.
 *   4. phase B: thr2(i) = f2 * d2min(i), f2 = (float)((1 + (double)tol)^2); r2 = (float)((double)cutoff * cutoff).  (j, m) is a
 *      NEIGHBOUR of i iff d2 <= thr2(i) and d2 <= r2.  cn(i) is their exact number.  One wave owns an atom and walks e in
 *      ascending chunks of 64; a ballot and a prefix population count give each hit its slot, so neighbors holds the first
 *      max_neighbors neighbours in ascending (j, m), (j, n_1, n_2, n_3) each with j local to the crystal, the rest -1.
 *   5. nearest = sqrt(d2min) (correctly rounded); farthest = sqrt of the largest neighbour d2, 0 at cn = 0; mutual(i) = the
 *      neighbours (j, m) of i with d2 <= thr2(j), d2 the one computed from i's side: the bonds both ends agree on.
 *   6. per crystal: n_bonds = sum cn, n_mutual = sum mutual, min_cn, max_cn (-1 without atoms), mean_cn = (float)n_bonds /
 *      (float)n (NaN without atoms).  flags: EMPTY n = 0; OVERLAP some d2min == 0; ISOLATED some cn = 0 (nothing within the
 *      cutoff; nearest is still the minimum over the range); OVERFLOW some cn > max_neighbors (the list is cut, cn is exact).
 * Limits: counts are int32 (a neighbour lies within the cutoff, so they stay far below 2^31 for any physical density); 32-bit
 * index arithmetic where n M fits, a 64-bit loop otherwise.  Offsets are clamped as in the screen.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, tol not finite or < 0, cutoff
 * not finite or <= 0, max_neighbors outside 1..ARREAU_COORD_MAX_NEIGHBORS, max_shells outside 1..ARREAU_SCREEN_MAX_SHELLS,
 * neighbors not 16-byte aligned.  B == 0 returns ARREAU_OK. */
#define ARREAU_COORD_NONFINITE 1
#define ARREAU_COORD_CELL 2
#define ARREAU_COORD_EMPTY 4
#define ARREAU_COORD_OVERLAP 8
#define ARREAU_COORD_ISOLATED 16
#define ARREAU_COORD_OVERFLOW 32
#define ARREAU_COORD_MAX_NEIGHBORS 64
typedef struct arreau_coordination_params {
    float tol;              /* a neighbour lies within (1 + tol) nearest; default 0.1 (a starting value, not a claim) */
    float cutoff;           /* A; default 6.0 */
    int32_t max_neighbors;  /* stored per atom, 1..ARREAU_COORD_MAX_NEIGHBORS; default 24 */
    int32_t max_shells;     /* cap on the images per axis, 1..ARREAU_SCREEN_MAX_SHELLS; default 8 */
} arreau_coordination_params;
typedef struct arreau_coordination_result { /* DEVICE arrays */
    int32_t* n_bonds;    /* [B] */
    int32_t* n_mutual;   /* [B] */
    int32_t* min_cn;     /* [B] */
    int32_t* max_cn;     /* [B] */
    float* mean_cn;      /* [B] */
    int32_t* flags;      /* [B] ARREAU_COORD_* */
    int32_t* cn;         /* [N] */
    int32_t* neighbors;  /* [N, max_neighbors, 4] j, n_1, n_2, n_3; 16-byte aligned */
    float* nearest;      /* [N] */
    float* farthest;     /* [N] */
    int32_t* mutual;     /* [N] */
    float* nearest_d2;   /* [N] d2min */
} arreau_coordination_result;
/* d_frac[N,3], d_lattice[B,3,3] rows a, b, c as for the screen (no species: the rule is table-free).  `params` and `out` are HOST
 * pointers to the structs; the arrays `out` names are device arrays. */
int arreau_crystal_coordination(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                                const arreau_coordination_params* params, arreau_coordination_result* out, void* stream);

/* ---- bond angles and Steinhardt order parameters of generated crystals -----------------------------------------------
 * What a coordination number cannot tell: per atom the distribution of the angles between its bonds and the bond-orientational
 * order parameters q_l, l = 2, 4, 6, 8 (Steinhardt, Nelson & Ronchetti, Phys. Rev. B 28, 784 (1983)) of the neighbour shell a
 * coordination result stores; per crystal the summed angle histogram and the mean q_l.  By the addition theorem of the
 * spherical harmonics, for a shell of m unit bond vectors u_e,
 *     q_l^2 = (4 pi / (2l+1)) sum_mm |mean_e Y_lmm(u_e)|^2 = (1 / m^2) sum_{e,f} P_l(u_e . u_f) = (m + 2 sum_{e<f} P_l(c_ef)) / m^2,
 * so one loop over the pairs of an atom's neighbours gives the histogram and every q_l from Legendre polynomials alone: no
 * spherical harmonics, no Wigner symbols, no tables.  No w_l, no neighbour-averaged parameters, no classification.
 * One launch after arreau_crystal_coordination, whose cn and neighbors arrays it reads: one workgroup of four waves per crystal,
 * one wave per atom (i = wave, wave + 4, ...), lane f owns bond f; no global atomics, no arreau_model.  Every float step is ONE
 * float32 operation rounded to nearest, in the order written, never contracted to a fused multiply-add, so a float32 host
 * restatement (arreau_amd/diffusion/bond_order.py) matches bit for bit.  "x < y ? x : y" below means that comparison: a NaN
 * never replaces a number, the first of two zeros stays.
 *   1. cell, positions and NONFINITE: the coordination rule 1 (wrapped positions p, cell rows L).  No image search is made, so
 *      there is no CELL flag.  For NONFINITE nothing else is computed: the reals are NaN, the counts 0, no other flag.
 *   2. the list: m(i) = min(cn(i), max_neighbors); entry e < m(i) of atom i is (j, n_1, n_2, n_3).  A crystal with some cn(i) < 0
 *      or with a j outside 0..n-1 among the first m(i) entries of an atom is BAD_LIST and blanked as for NONFINITE; this is
 *      decided for the whole crystal before anything is indexed with a j, and nothing is read out of range.
 *   3. bond e of atom i (lane e < m): s_d = (n_1 L_0d + n_2 L_1d) + n_3 L_2d, disp = (p_j + s) - p_i, d2 = (dx dx + dy dy) + dz dz
 *      (the coordination rule 2, the same operations); d = sqrt(d2) correctly rounded; u = disp / d componentwise.  An atom
 *      with a bond of d2 == 0 is DEGENERATE: its reals are NaN, its histogram 0, the crystal gets OVERLAP.
 *   4. pairs e < f: c_ef = (ux ux' + uy uy') + uz uz' (u of e first), then c = c < -1 ? -1 : c, c = c > 1 ? 1 : c.  Lane f
 *      (0 <= f < m) walks e = 0 .. f-1 in ascending order.
 *   5. Legendre polynomials: P_0 = 1, P_1 = c, P_{k+1} = a_k (c P_k) - b_k P_{k-1} for k = 1..7, a_k = (float)((2k+1)/(k+1)),
 *      b_k = (float)(k/(k+1)) formed in double; in the order t = c P_k; t = a_k t; s = b_k P_{k-1}; P_{k+1} = t - s.
 *   6. sums: lane f holds s_f = (((+0 + P_l(c_0f)) + P_l(c_1f)) + ...); lanes f >= m and lane 0 hold +0.  The LANE SUM folds the
 *      64 lane values by the butterfly v <- v + shuffle_xor(v, w), w = 32, 16, 8, 4, 2, 1: S_l(i).  It depends on the list alone.
 *   7. q2_l(i) = ((float)m + 2 S_l) / ((float)m (float)m), then q2 = q2 < 0 ? 0 : q2; q_l = sqrt(q2_l).  m = 0: NaN for both,
 *      the crystal gets ISOLATED.  m = 1: q2_l = 1 for every l.
 *   8. angle histogram, ARREAU_BOND_ANGLE_BINS = 37 bins centred on 0, 5, ..., 180 degrees: bin(c) = #{k in 0..35 : c <= E_k},
 *      E = cos_edges, which the caller computes as E_k = (float)cos((k + 1/2) 5 degrees) in double (centres on multiples of 5
 *      degrees keep 60, 90, 120 and 180 off the edges).  angles[i] counts the pairs of atom i per bin.  cos_min(i) and
 *      cos_max(i) are the extremes of c_ef (the largest and the smallest angle): lane f folds its pairs in walking order from
 *      +inf / -inf by lo = c < lo ? c : lo, hi = c > hi ? c : hi; the lanes are folded by the butterfly of rule 6 with
 *      lo = other < lo ? other : lo (hi alike), and lane 0's value is stored.  NaN for m < 2.
 *   9. per crystal: angle_hist = the sum of its atoms' histograms, n_angles their total; mean_q[l] = the lane sum of rule 6 of
 *      q_l over the atoms with m >= 1 and all four q finite, lane = i mod 64, ascending i within a lane, divided by (float) of
 *      their number; NaN without any.  n_used(i) = m(i).  flags: NONFINITE; EMPTY n = 0; BAD_LIST; OVERLAP; ISOLATED;
 *      TRUNCATED some cn > max_neighbors (the shell is cut, n_used says where).
 * A crystal alone gives the bits it gives inside any batch.  Offsets are clamped as in the screen.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, max_neighbors outside
 * 1..ARREAU_COORD_MAX_NEIGHBORS, d_neighbors not 16-byte aligned, cos_edges not strictly descending inside (-1, 1).  B == 0
 * returns ARREAU_OK. */
#define ARREAU_BOND_NONFINITE 1
#define ARREAU_BOND_EMPTY 2
#define ARREAU_BOND_BAD_LIST 4
#define ARREAU_BOND_OVERLAP 8
#define ARREAU_BOND_ISOLATED 16
#define ARREAU_BOND_TRUNCATED 32
#define ARREAU_BOND_ANGLE_BINS 37
#define ARREAU_BOND_ORDER_L 4 /* l = 2, 4, 6, 8 */
typedef struct arreau_bond_order_params {
    int32_t max_neighbors;                        /* the row width of d_neighbors, 1..ARREAU_COORD_MAX_NEIGHBORS */
    float cos_edges[ARREAU_BOND_ANGLE_BINS - 1];  /* E_k, strictly descending inside (-1, 1) */
} arreau_bond_order_params;
typedef struct arreau_bond_order_result { /* DEVICE arrays */
    float* mean_q;        /* [B, 4] */
    int32_t* n_angles;    /* [B] */
    int32_t* angle_hist;  /* [B, 37] */
    int32_t* flags;       /* [B] ARREAU_BOND_* */
    int32_t* n_used;      /* [N] m */
    float* q;             /* [N, 4] q_2, q_4, q_6, q_8 */
    float* q2;            /* [N, 4] their squares */
    float* cos_min;       /* [N] */
    float* cos_max;       /* [N] */
    int32_t* angles;      /* [N, 37] */
} arreau_bond_order_result;
/* d_frac, d_lattice, d_crystal_offsets as for the coordination search; d_cn [N] and d_neighbors [N, max_neighbors, 4] are a
 * coordination result's cn and neighbors arrays (or a list in their layout).  `params` and `out` are HOST pointers to the structs;
 * the arrays `out` names are device arrays. */
int arreau_crystal_bond_order(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                              const int32_t* d_cn, const int32_t* d_neighbors, const arreau_bond_order_params* params,
                              arreau_bond_order_result* out, void* stream);

/* ---- Voronoi cells of generated crystals: solid-angle-weighted neighbours, atom volumes -------------------------------
 * Per atom the faces of its Voronoi cell over every periodic image: the neighbours are the atoms whose bisecting planes bound
 * the cell, each with the solid angle its face subtends, the face's area and the distance; the WEIGHT of a face is its solid
 * angle over the atom's largest (pymatgen VoronoiNN's weight, where CrystalNN starts); the cell's volume comes with it.  Table
 * free: no radii, no electronegativities, no distance weighting, no probabilities -- not CrystalNN; plain (not radical, not
 * weighted) Voronoi cells; no polyhedron names.  One launch, one workgroup of four waves per crystal, one wave per atom
 * (i = wave, wave + 4, ...), no atomics, no arreau_model.  The distances of rule 1 are one float32 operation at a time; the
 * planes of rule 2 are solved and tested in float64 from those float32 displacements, taken as exact; the faces of rule 3 are
 * plain float32 (the compiler may fuse a multiply-add).  The order of every sum is fixed, so a result does not depend on the
 * launch or the batch, but no float32 host restatement matches it bit for bit: arreau_amd/diffusion/voronoi.py restates the rules
 * with the same split of precisions, and in float64 throughout.
 *   0. cell, NONFINITE, CELL, images, positions: the coordination rule 1 with search_radius = cutoff.  For NONFINITE and CELL
 *      nothing else is computed: the reals are NaN, neighbors -1, the counts 0, min_cn and max_cn -1, no other flag.
 *   1. CANDIDATES of atom i: every (j, m) but (i, (0, 0, 0)) with d2 <= r2 = (float)((double)cutoff * cutoff), d2 and disp formed
 *      exactly as in the coordination rule 2, gathered in ascending (j, m) by ballot.  d_e = disp as float64, h_e = |d_e|^2 / 2
 *      and |d_e| in float64 (the plane bisects the displacement the kernel holds); the stored distance is sqrt(d2) in float32.
 *      More than max_candidates of them: the atom is OVERFLOW, its reals NaN, its cn 0, its list -1.  No candidate is dropped
 *      early: the security-radius rule (farther than twice the largest vertex radius of a closed cell of nearer candidates) is
 *      not used, every candidate within the cutoff takes part.  An atom with a candidate at d2 == 0 shares its site and has no
 *      cell: it is OVERLAP, its reals NaN, its cn 0, its list -1 (an atom that merely sees such a pair meets each of their
 *      planes twice and fails the closure test of rule 5).
 *   2. VERTICES of face a (a = 0 .. K-1 in candidate order): for b = 0 .. K-1, b != a, lanes take c = b+1 .. K-1, c != a; v
 *      solves d_a.v = h_a, d_b.v = h_b, d_c.v = h_c by Cramer's rule, det = (d_a x d_b).d_c, v = (h_a d_b x d_c + h_b d_c x d_a +
 *      h_c d_a x d_b) / det.  The triple is SKIPPED when det == 0 or |det| < ARREAU_VORONOI_DET_TOL |d_a||d_b||d_c|.  v is
 *      ACCEPTED iff d_e.v - h_e <= ARREAU_VORONOI_PLANE_TOL * cutoff * |d_e| for every candidate e other than a, b, c
 *      (inclusive: v may lie up to PLANE_TOL * cutoff beyond a plane).  The planes are tested in ascending distance and the loop
 *      ends when no lane's vertex is left, which does not change the answer.  The hits are compacted by ballot in (b, c) order
 *      into the face's own list, at most ARREAU_VORONOI_FACE_VERTICES; more (only copies of degenerate vertices can make so many)
 *      make the atom OVERFLOW.  A vertex where q > 3 planes meet appears (q-1 choose 2) times in a face's list; the copies span
 *      fan triangles of zero area, so nothing is de-duplicated.
 *      Everything in this rule is float64.  Float32 does not suffice: with u = 2^-24 the bound below demands DET_TOL near
 *      1e-2, and so coarse a DET_TOL skips real, ill-conditioned vertices of irregular crystals whose loss moves omega_sum by
 *      less than CLOSURE_TOL (up to 6.5e-4 on random crystals in the float64 restatement), so the certificate would pass cells
 *      that are wrong in the fourth digit.  In float64, with u = 2^-53 and R = cutoff: Cramer's numerator has three terms of at most h |d||d| each, each with about 8 u relative
 *      rounding, and |det| >= DET_TOL |d_a||d_b||d_c|, so |dv| <= 8 u (|d_a| + |d_b| + |d_c|) / (2 DET_TOL) <= 12 u R / DET_TOL.
 *      DET_TOL = 1e-6 (three normals within a few 1e-5 degrees of one plane) makes that 1.4e-9 R; PLANE_TOL = 1e-6 is some 700
 *      times it, and small enough that what it lets in is harmless: a vertex accepted up to s beyond a plane adds a triangle
 *      of area about s^2 to a face (the true vertices next to it are accepted too), 4e-11 A^2 at R = 6 A.  Exactly degenerate
 *      vertices (sc, fcc) are degenerate in the float32 displacements too and fall inside the slack, and so do those the
 *      rounding of the inputs splits by less than it (ideal hcp given in float32: split by 1e-7 A, rejoined, closed to 4e-7
 *      sr); vertices split by more are the several true vertices of the cell the kernel was given.
 *   3. per FACE (a candidate with at least three accepted vertices): g = the mean of its vertices (lane sums, then the
 *      butterfly v <- v + shuffle_xor(v, w), w = 32 .. 1); n = d_a / |d_a|; t = the coordinate axis with the smallest |n_t| (x
 *      before y before z on ties); u1 = (n x t) / |n x t|, u2 = n x u1; angle(v) = atan2((v - g).u2, (v - g).u1); the vertices
 *      sorted by ascending angle, ties in list order: w_0 .. w_{k-1} (the vertices rounded to float32; all of rule 3 is float32).  area = sum_k n.((w_k - g) x (w_{k+1} - g)) / 2 (cyclic);
 *      solid_angle = sum_k 2 atan2(g.(w_k x w_{k+1}), |g||w_k||w_{k+1}| + (g.w_k)|w_{k+1}| + (g.w_{k+1})|w_k| + (w_k.w_{k+1})|g|)
 *      (Van Oosterom & Strackee 1983); both sums by lane (k, k + 64) and the butterfly.  distance = |d_a|.
 *   4. per ATOM: max_solid = the largest solid angle of its faces; weight_f = max(solid_angle_f, 0) / max_solid, and 0 for every
 *      face when max_solid is not > 0 (a face of zero area -- a second neighbour of sc or fcc that touches the cell in an edge
 *      or a corner -- has a solid angle that is rounding noise of either sign: it weighs 0); cn = the number of faces with
 *      weight >= tol (exact); at tol = 0 that is every face, the zero-area ones included, so count neighbours with a tol above
 *      0; cn_eff = the sum of all faces' weights; omega_sum = the sum of their solid angles;
 *      volume = sum area * distance / 6; max_radius = the largest |v| of an accepted vertex (sums: lane k holds faces k and
 *      k + 64, then the butterfly).  neighbors holds the first max_faces faces of weight >= tol in ascending (j, m), (j, n_1,
 *      n_2, n_3) each with j local to the crystal, -1 beyond: the coordination result's layout, so arreau_crystal_bond_order
 *      reads cn and neighbors as they are.  face_weight, face_solid_angle, face_area, face_distance [N, max_faces] in the same
 *      order, NaN beyond.  cn > max_faces sets TRUNCATED.
 *   5. the CERTIFICATE.  An atom is OPEN when 2 max_radius > cutoff (an atom beyond the cutoff could still cut the cell) or
 *      not (|omega_sum - 4 pi| <= ARREAU_VORONOI_CLOSURE_TOL) (a vertex was lost to DET_TOL, or the candidates close no cell; an
 *      atom without candidates is OPEN).  CLOSURE_TOL = 1e-3 sr: a lost vertex or a wrong face moves a solid angle by 1e-3 or
 *      more, the float32 sum of a closed cell stays within some 1e-5.  An OPEN atom keeps its numbers.  atom_flags [N] holds
 *      each atom's OVERLAP, OPEN, OVERFLOW and TRUNCATED bits.
 *   6. per crystal: n_faces = sum cn, min_cn, max_cn (-1 without atoms), mean_cn = (float)n_faces / (float)n, mean_cn_eff = (sum
 *      cn_eff) / (float)n, volume_sum = sum volume (each wave adds its atoms in order, the four waves are added in order; NaN
 *      when an atom is OVERFLOW or OVERLAP; NaN without atoms).  flags: the OR of the atoms' bits, EMPTY n = 0, and NONFINITE / CELL.
 * Offsets are clamped as in the screen.  The defaults (tol 0.05, cutoff 6 A) are starting values, not claims.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, tol not finite or outside
 * [0, 1], cutoff not finite or <= 0, max_faces outside 1..ARREAU_VORONOI_MAX_FACES, max_candidates outside
 * 1..ARREAU_VORONOI_MAX_CANDIDATES, max_shells outside 1..ARREAU_SCREEN_MAX_SHELLS, neighbors not 16-byte aligned.  B == 0
 * returns ARREAU_OK. */
#define ARREAU_VORONOI_NONFINITE 1
#define ARREAU_VORONOI_CELL 2
#define ARREAU_VORONOI_EMPTY 4
#define ARREAU_VORONOI_OVERLAP 8
#define ARREAU_VORONOI_OPEN 16
#define ARREAU_VORONOI_OVERFLOW 32
#define ARREAU_VORONOI_TRUNCATED 64
#define ARREAU_VORONOI_MAX_FACES 64
#define ARREAU_VORONOI_MAX_CANDIDATES 128
#define ARREAU_VORONOI_FACE_VERTICES 128
#define ARREAU_VORONOI_DET_TOL 1e-6   /* float64 */
#define ARREAU_VORONOI_PLANE_TOL 1e-6 /* float64 */
#define ARREAU_VORONOI_CLOSURE_TOL 1e-3f
typedef struct arreau_voronoi_params {
    float tol;               /* a face counts when its weight >= tol, in [0, 1]; default 0.05 (a starting value, not a claim) */
    float cutoff;            /* A; default 6.0 */
    int32_t max_faces;       /* stored per atom, 1..ARREAU_VORONOI_MAX_FACES; default 32 */
    int32_t max_candidates;  /* 1..ARREAU_VORONOI_MAX_CANDIDATES; default 128 */
    int32_t max_shells;      /* cap on the images per axis, 1..ARREAU_SCREEN_MAX_SHELLS; default 8 */
} arreau_voronoi_params;
typedef struct arreau_voronoi_result { /* DEVICE arrays */
    int32_t* n_faces;         /* [B] */
    int32_t* min_cn;          /* [B] */
    int32_t* max_cn;          /* [B] */
    float* mean_cn;           /* [B] */
    float* mean_cn_eff;       /* [B] */
    float* volume_sum;        /* [B] */
    int32_t* flags;           /* [B] ARREAU_VORONOI_* */
    int32_t* cn;              /* [N] */
    int32_t* neighbors;       /* [N, max_faces, 4] j, n_1, n_2, n_3; 16-byte aligned */
    float* face_weight;       /* [N, max_faces] */
    float* face_solid_angle;  /* [N, max_faces] */
    float* face_area;         /* [N, max_faces] */
    float* face_distance;     /* [N, max_faces] */
    float* volume;            /* [N] */
    float* omega_sum;         /* [N] */
    float* max_radius;        /* [N] */
    float* cn_eff;            /* [N] */
    int32_t* atom_flags;      /* [N] OVERLAP | OPEN | OVERFLOW | TRUNCATED */
} arreau_voronoi_result;
/* d_frac, d_lattice, d_crystal_offsets as for the coordination search.  `params` and `out` are HOST pointers to the structs; the
 * arrays `out` names are device arrays. */
int arreau_crystal_voronoi(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                           const arreau_voronoi_params* params, arreau_voronoi_result* out, void* stream);

/* ---- powder X-ray diffraction patterns of generated crystals ----------------------------------------------------------
 * Per crystal its powder pattern on a fixed 2 theta grid: the one observable a generated crystal is compared with in a
 * laboratory, and a signature that does not depend on the description -- a crystal gives the same pattern in any basis, in its
 * primitive cell, in its conventional cell and in any supercell.  Table free: the atoms are point scatterers of amplitude w_a
 * (the caller's [N] floats: the atomic numbers, the forward-scattering limit of the X-ray form factor, or 1, or anything else);
 * no Cromer-Mann form factors, no anomalous dispersion, no peak list, no merging of equivalent reflections, no preferred
 * orientation, no K alpha 2.  One launch, one workgroup of four waves per crystal, a thread per reflection of a round of 256
 * box entries, no atomics, no arreau_model.  The order of every sum is fixed, so a crystal's row is the same bits alone, in any
 * batch and at any place in it.  arreau_amd/diffusion/xrd.py restates the rules in float64 and with the same split of precisions.
 *   1. PARAMETERS (float64, on the host, once per launch): sigma = fwhm / (2 sqrt(2 ln 2)) degrees; the grid g_p = two_theta_min
 *      + p step, step = (two_theta_max - two_theta_min) / (n_points - 1), g_{n_points-1} = two_theta_max; the range lo =
 *      max(two_theta_min - 6 sigma, 0), hi = two_theta_max + 6 sigma as a cut on d*: d*_lo = 2 sin(lo / 2) / wavelength, d*_hi =
 *      2 sin(hi / 2) / wavelength.  6 sigma <= ARREAU_XRD_MAX_WINDOW = 10 degrees, so hi <= 170: asin and LP stay well conditioned.
 *   2. CELL (float64 from the float32 entries, taken as exact): rows a_1, a_2, a_3, det = a_1 . (a_2 x a_3), V = |det|, the
 *      reciprocal rows b_1 = (a_2 x a_3) / det, b_2 = (a_3 x a_1) / det, b_3 = (a_1 x a_2) / det: a_i . b_j = delta_ij, no 2 pi.
 *      NONFINITE: a cell entry, a coordinate or an amplitude of the crystal is not finite.  CELL: V or the float32 volume (the
 *      screen's expression, which `volume` reports) is zero or not finite.  EMPTY: no atoms.  In that order; one flag at most.
 *   3. BOX: |h_k| <= H_k = floor(d*_hi |a_k|) with |a_k| the DIRECT cell's row lengths.  The bound is exact, h_k = G . a_k <= |G|
 *      |a_k|; the reciprocal lengths would give a smaller box in a skewed cell and lose reflections.  RANGE: an H_k > max_index.
 *      A flagged crystal's pattern, volume and weight_sum are NaN and its n_reflections 0; nothing else is computed.
 *   4. REFLECTIONS: the box entries e = (h W_2 + (k + H_2)) W_3 + (l + H_3), W_k = 2 H_k + 1, h = 0 .. H_1, in ascending e; of them
 *      the half space h > 0, or h = 0 and k > 0, or h = k = 0 and l > 0 (Friedel: each counts twice).  G = (h b_1 + k b_2) + l b_3,
 *      d*^2 = |G|^2, float64; KEPT iff d*_lo^2 <= d*^2 <= d*_hi^2.  n_reflections = 2 * the kept: the lattice points of the full
 *      sphere's shell, which depends on the cell's description (a supercell has more, all but the parent's with F = 0).
 *   5. STRUCTURE FACTOR (float32, one rounding per operation, atoms in order): x_a the wrapped coordinates (f - floor(f), a result
 *      of 1 becomes 0); t = (h x + k y) + l z; r = t - rint(t) in revolutions; (s, c) = sincospi(2 r); re += w_a c, im += w_a s.
 *      The reduced phase carries at most 2 pi (|h| + |k| + |l| + 2) 2^-24 radians of error, which grows with max_index.
 *   6. INTENSITY (float64): sin theta = wavelength d* / 2, theta = asin, 2 theta in degrees; LP = (1 + cos^2 2 theta) / (sin^2
 *      theta cos theta) from sin theta alone; DW = exp(-b_iso d*^2 / 2) (exp(-B s^2) per amplitude, s = d* / 2, one B for every
 *      atom); I = 2 (re^2 + im^2) DW LP / V^2.  The 1 / V^2 makes the pattern a property of the crystal, not of the cell it is
 *      described in.  amp = (float)(I / (sigma sqrt(2 pi))).
 *   7. PATTERN: P(g_p) = sum over the kept reflections, in ascending e, of amp * expf(-0.5 z^2), z = (float)((g_p - 2 theta_hkl)
 *      / sigma), the difference float64, over the grid points with |g_p - 2 theta_hkl| <= 6 sigma; float32 adds, no atomics.  The
 *      cut at 6 sigma drops terms of relative size e^-18 = 1.5e-8.  The pattern is a smooth function of the inputs: no binning.
 *   8. weight_sum = sum w_a: thread t adds atoms t, t + 256, ..., then the wave butterfly, then the four waves in order.
 * Offsets are clamped as in the screen.  The defaults (Cu K alpha 1.54184 A, 5..90 degrees in 1701 points, fwhm 0.2, b_iso 0,
 * max_index 64) are starting values, not claims.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, wavelength not finite or
 * <= 0, not 0 <= two_theta_min < two_theta_max <= ARREAU_XRD_MAX_TWO_THETA, n_points outside 2..ARREAU_XRD_MAX_POINTS, fwhm not
 * finite or <= 0, 6 sigma > ARREAU_XRD_MAX_WINDOW, b_iso not finite or < 0, max_index outside 1..ARREAU_XRD_MAX_INDEX.  B == 0
 * returns ARREAU_OK. */
#define ARREAU_XRD_NONFINITE 1
#define ARREAU_XRD_CELL 2
#define ARREAU_XRD_EMPTY 4
#define ARREAU_XRD_RANGE 8
#define ARREAU_XRD_MAX_POINTS 4096
#define ARREAU_XRD_MAX_INDEX 127
#define ARREAU_XRD_MAX_TWO_THETA 160.0
#define ARREAU_XRD_MAX_WINDOW 10.0 /* degrees: the largest 6 sigma */
typedef struct arreau_xrd_params {
    double wavelength;     /* A; default 1.54184 (Cu K alpha) */
    double two_theta_min;  /* degrees; default 5 */
    double two_theta_max;  /* degrees; default 90 */
    double fwhm;           /* degrees; default 0.2 */
    double b_iso;          /* A^2; default 0 */
    int32_t n_points;      /* 2..ARREAU_XRD_MAX_POINTS; default 1701 */
    int32_t max_index;     /* 1..ARREAU_XRD_MAX_INDEX; default 64 */
} arreau_xrd_params;
typedef struct arreau_xrd_result { /* DEVICE arrays */
    float* pattern;          /* [B, n_points] */
    int32_t* n_reflections;  /* [B] */
    float* volume;           /* [B] */
    float* weight_sum;       /* [B] */
    int32_t* flags;          /* [B] ARREAU_XRD_* */
} arreau_xrd_result;
/* d_frac, d_lattice, d_crystal_offsets as for the coordination search; d_weights [N] float32, the atoms' amplitudes.  `params`
 * and `out` are HOST pointers to the structs; the arrays `out` names are device arrays. */
int arreau_crystal_xrd(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, const float* d_weights,
                       int32_t B, int32_t N, const arreau_xrd_params* params, arreau_xrd_result* out, void* stream);

/* ---- Ewald electrostatics of generated crystals ----------------------------------------------------------------------
 * Per crystal the electrostatic energy of point charges q_a (the caller's [N] floats, in units of e) on the sites of the periodic
 * crystal, its real-space, reciprocal-space, self and background parts, and per atom the site potential: the first physical
 * question asked of a generated ionic crystal.  Table free: the caller supplies the charges; no oxidation-state guessing, no
 * charge-balance check.  Tin-foil boundary conditions and, for a crystal that is not neutral, a neutralising background; no
 * dipole correction, no forces, no stress, no short-range repulsion (the energy alone favours collapse).  The screen's exact
 * real-space image walk and the powder pattern's reciprocal-space box walk in one launch, one workgroup of four waves per
 * crystal, no atomics, no arreau_model.  The order of every sum is fixed, so a crystal's numbers are the same bits alone, in any
 * batch and at any place in it.  arreau_amd/diffusion/ewald.py restates the rules in float64 and with the same split of precisions.
 * Units: charges in e, lengths in A, K = ARREAU_EWALD_K = 14.399645 eV A = V A / e, potentials in V (the sums of rules 3-5 are in
 * e / A; rule 6 multiplies them by K), energies in eV.
 *   1. PARAMETERS (float64, on the host, once per launch): s = sqrt(-ln accuracy).  Per crystal alpha = params.alpha where that
 *      is > 0, else sqrt(pi) cbrt(sqrt(n) / V) = sqrt(pi) (n / V^2)^(1/6) (n atoms); r_cut = s / alpha; G_cut = alpha s / pi.  Both
 *      sums then drop terms of relative size about `accuracy`.
 *   2. CELL: the powder pattern's rule 2 (float64 from the float32 entries: det, V = |det|, the reciprocal rows b_k, no 2 pi).
 *      NONFINITE: a cell entry or a coordinate of the crystal is not finite.  CELL: V or the float32 volume is zero or not
 *      finite.  EMPTY: no atoms.  CELL again: not (q_k <= max_shells) for an axis, q_k the screen's rule 1 with search_radius =
 *      (float)r_cut.  RANGE: an H_k = floor(G_cut |a_k|) > max_index (the powder pattern's rule 3 with d*_hi = G_cut).
 *      UNASSIGNED: a charge of the crystal is not finite (the host's marker for a species without a given charge).  In that
 *      order, one flag at most; nothing else is computed.
 *   3. REAL SPACE: images and positions by the screen's rules 4 and 5 with search_radius = (float)r_cut.  For receiver a, every
 *      atom b and image m, the entry e = b M + m without (b = a, m = (0, 0, 0)): displacement and d2 by the screen's rule 6,
 *      float32, one rounding per operation.  KEPT iff d2 <= (float)(r_cut^2).  A kept d2 = 0 sets OVERLAP and adds nothing.
 *      Otherwise r = sqrt((double)d2) and the term q_b erfc(alpha r) / r, float64.  One wave owns an atom (wave w: a = w, w + 4,
 *      ...); lane t adds its entries e = t, t + 64, ... in ascending order; the wave's sum is the butterfly v + shuffle_xor(v, 32
 *      .. 1).  n_pairs = the kept terms of the crystal with d2 > 0 (ordered pairs: each contact counts from both ends).
 *   4. RECIPROCAL SPACE: the powder pattern's rule 4 over the box of 2: the half space in ascending box index, G and |G|^2 in
 *      float64, KEPT iff 0 < |G|^2 <= G_cut^2; n_reciprocal = 2 * the kept.  S(G) = sum_b q_b (c_b + i s_b), (s_b, c_b) =
 *      sincospi(2 r_b) in float32 with r_b the reduced float32 phase of the powder pattern's rule 5; products and sums float64, in
 *      atom order.  w(G) = (2 / (pi V)) exp(-pi^2 |G|^2 / alpha^2) / |G|^2 (the 2 is Friedel's).  phi_a receives w Re S c_a + w Im
 *      S s_a for every kept G in ascending box index (thread t owns atoms t, t + 256, ...).
 *   5. SELF AND BACKGROUND: Q = sum q_a, A = sum |q_a|, float64 in atom order.  The self part of atom a is -2 alpha q_a / sqrt(pi),
 *      the background part -pi Q / (V alpha^2).  CHARGED (informational): |Q| > 1e-6 A; the neutralising background is in the number.
 *   6. POTENTIALS AND ENERGIES: each of the four parts of atom a is multiplied by K, and potential_a = ((K real + K reciprocal) +
 *      K self) + K background, in volts.  energy = (1 / 2) sum_a q_a potential_a -- the textbook (K / 2) sum q phi with K inside the
 *      potential --, every product and every sum one float64 operation rounded to nearest, in atom order; real, reciprocal, self,
 *      background the same sum over that part of the potential alone.  net_charge = Q; alpha and volume
 *      (V, float64) are reported.  A crystal with any flag but CHARGED has NaN reals, NaN potentials and zero counts.
 * Offsets are clamped as in the screen.  The defaults (accuracy 1e-8, alpha 0, max_shells 8, max_index 64) are starting values,
 * not claims.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, accuracy not in (0, 1),
 * alpha not finite or < 0, max_shells outside 1..ARREAU_SCREEN_MAX_SHELLS, max_index outside 1..ARREAU_XRD_MAX_INDEX.  B == 0
 * returns ARREAU_OK. */
#define ARREAU_EWALD_NONFINITE 1
#define ARREAU_EWALD_CELL 2
#define ARREAU_EWALD_EMPTY 4
#define ARREAU_EWALD_RANGE 8
#define ARREAU_EWALD_UNASSIGNED 16
#define ARREAU_EWALD_OVERLAP 32
#define ARREAU_EWALD_CHARGED 64 /* informational */
#define ARREAU_EWALD_K 14.399645 /* e^2 / (4 pi eps_0) in eV A */
typedef struct arreau_ewald_params {
    double accuracy;     /* in (0, 1); default 1e-8 */
    double alpha;        /* 1/A; 0: per crystal sqrt(pi) (n / V^2)^(1/6); default 0 */
    int32_t max_shells;  /* cap on the images per axis, 1..ARREAU_SCREEN_MAX_SHELLS; default 8 */
    int32_t max_index;   /* 1..ARREAU_XRD_MAX_INDEX; default 64 */
} arreau_ewald_params;
typedef struct arreau_ewald_result { /* DEVICE arrays */
    double* energy;         /* [B] eV */
    double* real;           /* [B] */
    double* reciprocal;     /* [B] */
    double* self;           /* [B] */
    double* background;     /* [B] */
    double* net_charge;     /* [B] e */
    double* alpha;          /* [B] 1/A */
    double* volume;         /* [B] A^3 */
    int64_t* n_pairs;       /* [B] */
    int32_t* n_reciprocal;  /* [B] */
    int32_t* flags;         /* [B] ARREAU_EWALD_* */
    double* potential;      /* [N] V */
    double* work;           /* [N] scratch: the reciprocal part of the potential while the launch runs */
} arreau_ewald_result;
/* d_frac, d_lattice, d_crystal_offsets as for the coordination search; d_charges [N] float32.  `params` and `out` are HOST
 * pointers to the structs; the arrays `out` names are device arrays. */
int arreau_crystal_ewald(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, const float* d_charges,
                         int32_t B, int32_t N, const arreau_ewald_params* params, arreau_ewald_result* out, void* stream);

/* ---- duplicate detection: structure fingerprints and their all-pairs match ------------------------------------------
 * The screen's sibling: per crystal a reduced formula and a fingerprint of its pair distribution (Oganov & Valle, J. Chem.
 * Phys. 130, 104504 (2009), with the normalisation taken at the bin centre so that it is finite for every input), and for
 * every crystal of a set the earliest crystal of that set -- or of another set -- it duplicates.  Two launches, no atomics,
 * no arreau_model, nothing copied to the host; no order of summation depends on the batch or the grid, so a crystal's row is
 * the same bits wherever it sits.
 *   1. reduced formula: the distinct species ids of the crystal (d_types: any int32, non-negative by convention -- class
 *      indices in the sampler, atomic numbers in a file) sorted ascending, at most ARREAU_FP_MAX_SPECIES; their counts N_A
 *      divided by the gcd of the counts.  species is padded with -1, counts with 0.  Two crystals are COMPARABLE when neither
 *      is flagged and both arrays are equal (the arrays are compared, not a hash).
 *   2. parameters r_max, n_bins (1..ARREAU_FP_BINS), sigma: delta = r_max / n_bins, R_k = (k + 1/2) delta, cut-off
 *      r_cut = (float)((double)r_max + 5 (double)sigma).
 *   3. contacts are enumerated exactly as arreau_crystal_screen enumerates them (its rules 1, 4, 5, 6 with search_radius =
 *      r_cut, the same float32 operations): wrapped positions, pairs i <= j, every image for i < j and the images after
 *      (0, 0, 0) for i == j, shells per axis from the plane spacings.  R = sqrt(d2) (correctly rounded); a contact counts
 *      when d2 < (float)((double)r_cut * r_cut).
 *   4. a contact between species ranks A <= B adds c g(R_k - R) to EVERY bin k of component (A, B), g(x) = exp(-x^2 /
 *      (2 sigma^2)) / (sigma sqrt(2 pi)), c = 1 for A != B and 2 for A == B (the ordered double sum meets such a contact
 *      twice).  Every (component, bin) cell adds its contacts in the enumeration order (i, j, m), one float32 accumulator.
 *   5. F_AB[k] = V S_AB[k] / (4 pi R_k^2 N_A N_B) - 1 (V the cell volume, N_A the unreduced counts); weights w_AB = N_A N_B /
 *      N^2; |F|_w^2 = sum_AB sum_k w_AB F_AB[k]^2 (a fixed-order sum); the stored vector is f_AB[k] = sqrt(w_AB) F_AB[k] /
 *      |F|_w, a unit vector.  Component (A, B) lies at index B (B + 1) / 2 + A of the row; the row has the fixed stride
 *      ARREAU_FP_ROW = 36 x 64 floats, unused components and bins >= n_bins are zero.
 *   6. flags (a flagged crystal has a zero row, species -1, counts 0, and neither matches nor is matched): NONFINITE a cell
 *      entry or a coordinate is inf / NaN (no other flag is then computed); EMPTY no atoms; MANY_SPECIES more than 8 distinct
 *      species; CELL volume not finite or not positive, or more than max_shells (1..8) images needed on an axis.
 *   7. distance d(x, y) = (1 - f_x . f_y) / 2, the dot product in float32 in ascending index order.  By construction it is
 *      invariant under atom permutation, a common translation, lattice translations of single atoms, rigid rotation, a change
 *      of cell basis and supercells (N_A N_B / V and the sum scale together).
 *   8. match of set X against set Y (NULL: X itself, and then only candidates a < x): duplicate_of = the smallest index a of
 *      Y comparable with x and d <= tolerance, else -1; distance = d to it (+inf when none); nearest / nearest_distance = the
 *      comparable candidate of smallest d, ties to the smaller index (-1 / +inf when none).  In self mode a crystal is UNIQUE
 *      when duplicate_of < 0 and flags == 0: the first member of each cluster is kept.
 * Offsets outside [0, N] or descending are clamped as in the screen.  Neither call synchronises.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, n_bins outside 1..64,
 * r_max or sigma not finite or not positive, max_shells outside 1..8, tolerance outside [0, 1]. */
#define ARREAU_FP_NONFINITE 1
#define ARREAU_FP_CELL 2
#define ARREAU_FP_MANY_SPECIES 4
#define ARREAU_FP_EMPTY 8
#define ARREAU_FP_MAX_SPECIES 8
#define ARREAU_FP_BINS 64
#define ARREAU_FP_COMPONENTS 36
#define ARREAU_FP_ROW (ARREAU_FP_COMPONENTS * ARREAU_FP_BINS)
typedef struct arreau_fingerprint_params {
    float r_max;         /* A; default 6 */
    float sigma;         /* A; default 0.1 */
    int32_t n_bins;      /* 1..ARREAU_FP_BINS; default 64 */
    int32_t max_shells;  /* cap on the images per axis, 1..ARREAU_SCREEN_MAX_SHELLS; default 8 */
} arreau_fingerprint_params;
typedef struct arreau_fingerprint_result { /* DEVICE arrays, one row per crystal: what the fingerprint writes, what the match reads */
    float* fingerprint;  /* [B, ARREAU_FP_ROW] */
    int32_t* species;    /* [B, 8] ascending, padded with -1 */
    int32_t* counts;     /* [B, 8] reduced counts, padded with 0 */
    int32_t* flags;      /* [B]    ARREAU_FP_* */
} arreau_fingerprint_result;
typedef struct arreau_match_result { /* DEVICE arrays, one entry per crystal of X */
    int32_t* duplicate_of;
    float* distance;
    int32_t* nearest;
    float* nearest_distance;
} arreau_match_result;
/* d_frac[N,3], d_types[N] species ids (required), d_lattice[B,3,3] rows a, b, c.  `params` and `out` are HOST pointers. */
int arreau_crystal_fingerprint(const float* d_frac, const int32_t* d_types, const float* d_lattice, const int32_t* d_crystal_offsets,
                               int32_t B, int32_t N, const arreau_fingerprint_params* params, arreau_fingerprint_result* out,
                               void* stream);
/* x, y: HOST pointers to the structs of two fingerprinted sets (y NULL: x against itself, By ignored); out: device arrays [Bx]. */
int arreau_fingerprint_match(const arreau_fingerprint_result* x, int32_t Bx, const arreau_fingerprint_result* y, int32_t By,
                             float tolerance, arreau_match_result* out, void* stream);

/* ---- symmetry search: the operations of a crystal in the cell it is given, its point group ----------------------------
 * The third instrument beside the screen and the fingerprint: which operations x' = W x + t (on fractional columns, modulo
 * lattice translations) map the crystal onto itself within a tolerance symprec (A), and which of the 32 point groups their
 * rotations form.  One launch, one workgroup of four waves per crystal, no atomics, no second stream, no arreau_model;
 * deterministic.  NOT computed: a space-group number, a primitive cell (arreau_crystal_reduce) or a conventional one
 * (arreau_crystal_conventional, which reads this search run on the reduced cell).
 * Conventions: the cell rows are a_0, a_1, a_2 (d_lattice); the Cartesian position of x is r_d = sum_k x_k L_kd.  Column j of W
 * holds the image of basis vector j, a'_j = sum_k W_kj a_k; with G_ij = a_i . a_j the image basis has the metric G' = W^T G W.
 * The rotation code of W is sum_{r,c} (W_rc + 1) 3^(3r + c) (W_00 the least significant base-3 digit; identity: 16484).
 *   1. cell checks.  NONFINITE: a cell entry or a coordinate of the crystal is inf / NaN (no other flag is then set).  CELL:
 *      the volume |a_0 . (a_1 x a_2)| (the screen's rule 1) is not positive or not finite.  EMPTY: no atoms.  Positions are
 *      wrapped as in the screen's rule 5: w = f - floor(f), a result >= 1 becomes 0.
 *   2. lattice candidates: every W with entries in {-1, 0, 1} (3^9 codes, in code order) and det = +-1 for which
 *      | sqrt(G'_ii) - sqrt(G_ii) | <= symprec for every i and | G'_ij - G_ij | <= symprec (|a_i| + |a_j|) / 2 for i < j.
 *      n_lattice counts them.  A lattice has at most 48 isometries: more than 48 means symprec is too loose for this cell --
 *      AMBIGUOUS, and beside n_lattice nothing is reported.  Limitation: an operation whose matrix in the given basis has an
 *      entry outside {-1, 0, 1} is not found; every conventional setting and the rhombohedral axes are covered, a badly skewed
 *      cell may not be.
 *   3. candidate translations: the species with the fewest atoms (the smallest id on ties), its first atom p0; for every atom q
 *      of that species, in ascending order, t = wrap(w_q - W w_p0), wrapped to [0, 1) as in 1.
 *   4. the test of (W, t): delta = (W w_i + t) - w_j, each component minus its nearest integer (rintf), c = delta's Cartesian
 *      image, d = |c|; the residual of the operation is the maximum over the atoms i of the minimum over the atoms j of the
 *      species of i; accepted when residual <= symprec.  The nearest image by components is the nearest image as long as the
 *      cell is not flatter than symprec, which is assumed.
 *   5. output: the accepted operations in the order (code of W ascending, q ascending): n_ops counts all of them, the first
 *      max_ops are stored (ops_rotation: the code; ops_translation; ops_residual), OVERFLOW when there are more; unused slots
 *      hold code -1 and zeros.  n_translations: the accepted operations with W = identity.  residual: the largest accepted one.
 *   6. point group: every distinct accepted W has a type from (det, trace): det +1 and trace 3, -1, 0, 1, 2 -> 1, 2, 3, 4, 6;
 *      det -1 and trace -3, 1, 0, -1, -2 -> -1, m, -3, -4, -6.  The ten counts are looked up among the 32 point groups
 *      (csrc/symfind_table.h, generated by closing each group's generators): point_group = 0..31 in the order 1, -1, 2, m, 2/m,
 *      222, mm2, mmm, 4, -4, 4/m, 422, 4mm, -42m, 4/mmm, 3, -3, 32, 3m, -3m, 6, -6, 6/m, 622, 6mm, -6m2, 6/mmm, 23, m-3, 432,
 *      -43m, m-3m.  point_group = -1 and NOT_A_GROUP when the counts match no row or n_ops != distinct rotations x
 *      n_translations (a tolerance can accept a set that is not closed).  The crystal system follows on the host.
 *   7. arithmetic: every step is one float32 operation rounded to nearest, in the order written, never contracted to a fused
 *      multiply-add: (W v)_r = (W_r0 v_0 + W_r1 v_1) + W_r2 v_2; a'_j likewise; dot products (x x' + y y') + z z'; c_d =
 *      (delta_0 L_0d + delta_1 L_1d) + delta_2 L_2d; square roots correctly rounded.  No float32 restatement is kept: the
 *      integer outputs are compared with the float64 restatement (arreau_amd/diffusion/symmetry_search.py) on guarded inputs,
 *      every decision quantity at most symprec / 2 or at least 2 symprec; the reals to 64 x 2^-24 x max_d sum_k |L_kd| (residuals)
 *      and 16 x 2^-24 (translations, modulo 1), derived there.
 * A crystal flagged NONFINITE, CELL, EMPTY or AMBIGUOUS has n_ops = n_translations = 0, residual NaN, point_group -1 and no stored
 * operation.  Crystals of up to 256 atoms keep their coordinates and species in LDS; larger ones read them from global memory
 * (the same values).  Cost: n_lattice x n_rarest x n^2 distance evaluations per crystal.  Offsets outside [0, N] or descending
 * are clamped as in the screen.  Does not synchronise.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, symprec not finite or not
 * positive, max_ops outside 1..ARREAU_SYM_MAX_OPS_CAP. */
#define ARREAU_SYM_NONFINITE 1
#define ARREAU_SYM_CELL 2
#define ARREAU_SYM_EMPTY 4
#define ARREAU_SYM_AMBIGUOUS 8
#define ARREAU_SYM_OVERFLOW 16
#define ARREAU_SYM_NOT_A_GROUP 32
#define ARREAU_SYM_MAX_OPS_CAP 4096
typedef struct arreau_symmetry_params {
    float symprec;   /* A; default 0.1 (what CDVAE and MatterGen evaluate with: a starting value, not a claim) */
    int32_t max_ops; /* operations stored per crystal, 1..ARREAU_SYM_MAX_OPS_CAP; default 192 */
} arreau_symmetry_params;
typedef struct arreau_symmetry_result { /* DEVICE arrays, one row per crystal */
    int32_t* n_lattice;      /* [B] */
    int32_t* n_ops;          /* [B] every accepted operation, also beyond max_ops */
    int32_t* n_translations; /* [B] */
    int32_t* ops_rotation;   /* [B, max_ops] rotation codes, -1 in unused slots */
    float* ops_translation;  /* [B, max_ops, 3] */
    float* ops_residual;     /* [B, max_ops] */
    float* residual;         /* [B] */
    int32_t* point_group;    /* [B] 0..31, -1: none */
    int32_t* flags;          /* [B] ARREAU_SYM_* */
} arreau_symmetry_result;
/* d_frac[N,3], d_types[N] species ids (required), d_lattice[B,3,3] rows a, b, c.  `params` and `out` are HOST pointers. */
int arreau_crystal_symmetry(const float* d_frac, const int32_t* d_types, const float* d_lattice, const int32_t* d_crystal_offsets,
                            int32_t B, int32_t N, const arreau_symmetry_params* params, arreau_symmetry_result* out, void* stream);

/* ---- cell reduction: the primitive, Delaunay-reduced cell of a crystal and its atoms in it ----------------------------------
 * The fourth instrument beside the screen, the fingerprint and the symmetry search: the pure translations a crystal has in the
 * cell it is given, the primitive cell they imply, a Delaunay-reduced (Selling) basis of that cell made of its shortest vectors,
 * and one atom per translation class expressed in it.  One launch, one workgroup of four waves per crystal, no atomics, no
 * arreau_model; deterministic.  NOT computed: a Niggli form, a space-group number; the conventional setting is a launch of its
 * own on this one's output (arreau_crystal_conventional).
 * Conventions as in the symmetry search: cell rows a_0, a_1, a_2, r_d = sum_k x_k L_kd, positions wrapped w = f - floor(f) (a
 * result >= 1 becomes 0).  dist(delta) of a fractional difference: each component minus its nearest integer (rintf) gives e; the
 * minimum over the 27 images s in {-1, 0, 1}^3, s_0 slowest, of |c|, c_d = ((e_0 + s_0) L_0d + (e_1 + s_1) L_1d) + (e_2 + s_2) L_2d.
 *   1. flags.  NONFINITE, CELL, EMPTY as in arreau_crystal_symmetry's rule 1.  A crystal flagged NONFINITE, CELL, EMPTY or
 *      AMBIGUOUS is copied through unchanged, bit for bit (positions not wrapped): lattice_out = lattice, transform = identity,
 *      multiplicity 1, n_out = n, keep = 0..n-1, selling_steps 0; n_translations is 0 for the first three and the number of
 *      accepted translations for AMBIGUOUS.
 *   2. pure translations.  The species with the fewest atoms (the smallest id on ties), its first atom p0; for every atom q of
 *      that species, ascending, t = wrap(w_q - w_p0).  t is a translation when max over the atoms i of min over the atoms j of
 *      the species of i of dist((w_i + t) - w_j) is <= symprec.  n_translations counts them (q = p0 gives the identity); m =
 *      n_translations.  AMBIGUOUS when m > ARREAU_RED_MAX_TRANSLATIONS, when m does not divide n, or when for some accepted t_a,
 *      t_b no accepted t_c has dist((t_a + t_b) - t_c) <= symprec (the set is not closed).
 *   3. primitive basis.  Every vector is held as integer numerators over m in the input basis; its Cartesian form is c_k =
 *      num_k / m (one division), v_d = (c_0 L_0d + c_1 L_1d) + c_2 L_2d.  The set: m e_0, m e_1, m e_2 (a, b, c), then per
 *      non-trivial translation, in q order, num = rint(m (t - rint(t))) + m s with the image s in {-1, 0, 1}^3 of the shortest
 *      |v|^2 (the first in lexicographic order on ties).  The set is sorted by |v|^2, ties to the lower index; the first triple
 *      i < j < k of the sorted list, in lexicographic order, with | |det| - V / m | <= V / (4 m) (det = v_i . (v_j x v_k), V the
 *      cell volume) is the primitive basis; all three vectors are negated when det < 0.  No such triple: AMBIGUOUS.
 *   4. Delaunay reduction.  Integer coefficients in the primitive basis: v_0, v_1, v_2 the basis, v_3 = -(v_0 + v_1 + v_2); each
 *      vector's Cartesian form is formed from its numerators as in 3 at every step (nothing accumulates).  tol = 1e-5 x the
 *      largest |v|^2 of the primitive basis.  While some v_i . v_j > tol: the first such pair in the order 01, 02, 03, 12, 13, 23
 *      takes the Selling step v_k += v_i, v_l += v_i (k, l the other two), v_i = -v_i.  At most ARREAU_RED_MAX_STEPS steps;
 *      selling_steps counts them, NOT_CONVERGED when the limit is reached.  Of the seven vectors v_0, v_1, v_2, v_3, v_0 + v_1,
 *      v_1 + v_2, v_2 + v_0, sorted by |v|^2 (ties to the lower index): the shortest, the next not parallel to it, the next
 *      independent of both (decided on the integers); all three negated when their integer determinant is negative.  Their
 *      numerators R give transform = R / m (rows: the reduced basis in the input basis, det = 1 / m) and lattice_out row r =
 *      (T_r0 L_0d + T_r1 L_1d) + T_r2 L_2d.  AMBIGUOUS when det R != m^2 or adj(R) / m is not an integer matrix.
 *   5. atoms.  Atom a is kept when for no non-trivial translation t_k the atom of its species nearest to w_a + t_k (dist; ties to
 *      the lower index) has an index below a: the lowest index of every translation class.  AMBIGUOUS when their number is not
 *      n / m.  The kept atoms, ascending, fill the crystal's first n_out = n / m output slots (the outputs use the input's
 *      offsets): keep = the atom's index local to the crystal, types_out its species, frac_out = wrap(w Q), Q = adj(R) / m the
 *      integer inverse of transform, (w_0 Q_0c + w_1 Q_1c) + w_2 Q_2c.  The slots n_out..n-1 hold keep -1, species -1, zeros.
 *   6. arithmetic: one float32 operation per step, rounded to nearest, in the order written, never contracted; square roots
 *      correctly rounded.  The float64 restatement (arreau_amd/diffusion/cell_reduction.py) reports the margin of every decision;
 *      on guarded inputs the discrete outputs agree and the reals are held to the bounds derived there.
 * Cost: n_rarest x n^2 x 27 distance evaluations for the translations, (m - 1) x n^2 x 27 for the atoms.  Offsets outside [0, N] or
 * descending are clamped as in the screen.  Does not synchronise.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, symprec not finite or not
 * positive. */
#define ARREAU_RED_NONFINITE 1
#define ARREAU_RED_CELL 2
#define ARREAU_RED_EMPTY 4
#define ARREAU_RED_AMBIGUOUS 8
#define ARREAU_RED_NOT_CONVERGED 16
#define ARREAU_RED_MAX_TRANSLATIONS 64
#define ARREAU_RED_MAX_STEPS 64
typedef struct arreau_reduce_params {
    float symprec; /* A; default 0.1, the symmetry search's */
} arreau_reduce_params;
typedef struct arreau_reduce_result { /* DEVICE arrays: one row per crystal, then one row per input atom */
    int32_t* multiplicity;   /* [B] m: input cell volume / reduced cell volume */
    int32_t* n_translations; /* [B] accepted pure translations, the identity included */
    float* lattice_out;      /* [B,3,3] rows of the reduced cell */
    float* transform;        /* [B,3,3] rows: the reduced basis in the input basis, multiples of 1 / m */
    int32_t* n_out;          /* [B] n / m */
    int32_t* flags;          /* [B] ARREAU_RED_* */
    int32_t* selling_steps;  /* [B] */
    float* frac_out;         /* [N,3] crystal b's atoms at offsets[b] .. offsets[b] + n_out[b] */
    int32_t* types_out;      /* [N] */
    int32_t* keep;           /* [N] the input atom (local to the crystal) of every output atom, -1 beyond n_out */
} arreau_reduce_result;
/* d_frac[N,3], d_types[N] species ids (required), d_lattice[B,3,3] rows a, b, c.  `params` and `out` are HOST pointers. */
int arreau_crystal_reduce(const float* d_frac, const int32_t* d_types, const float* d_lattice, const int32_t* d_crystal_offsets,
                          int32_t B, int32_t N, const arreau_reduce_params* params, arreau_reduce_result* out, void* stream);

/* ---- symmetrization: exact orbits, positions and cell under the operations the symmetry search found ---------------------
 * The fifth instrument: arreau_crystal_symmetry says which operations a crystal has within symprec; this entry point moves the
 * atoms onto sites those operations map onto each other exactly, gives the cell the metric they leave invariant and reports
 * the orbits (which atoms are equivalent, with which multiplicity and site-symmetry order).  One launch, one workgroup of four
 * waves per crystal, no atomics on floats, no second stream, no arreau_model; deterministic.  NOT computed: a space-group
 * number, an origin, a standard setting; the cell keeps the basis it came in.
 * `found` is the result of arreau_crystal_symmetry on the same arrays (a HOST struct of device pointers; n_ops, ops_rotation,
 * ops_translation and flags are read), max_ops its row width.  Conventions as in the symmetry search.  Per crystal, with the
 * stored operations (W_m, t_m), m < n_ops, n atoms, wrapped positions w_i (the screen's rule 5):
 *   1. flags.  NONFINITE, CELL and EMPTY as in arreau_crystal_symmetry's rule 1.  NO_GROUP: the search flagged the crystal
 *      AMBIGUOUS, OVERFLOW or NOT_A_GROUP (the stored operations are then not a whole group), or n_ops lies outside 1..max_ops, or a
 *      stored code is no matrix of determinant +-1.  NOT_A_PERMUTATION: a partner map of rule 2 is not one-to-one, or an orbit
 *      size of rule 6 does not divide n_ops.  A crystal with any flag is copied through unchanged: frac_out = w bit for bit, its
 *      lengths, angles and lattice come from its own metric G by rule 5, orbit[i] = i, orbit_size = site_order = 1, n_orbits =
 *      n, both displacements 0, ops_translation and ops_shift 0, partner -1.
 *   2. partners.  For every operation m and atom i: delta = (W_m w_i + t_m) - w_j, each component minus its nearest integer, and
 *      |c|^2 of its Cartesian image, exactly the float32 operations of the search's rule 4; p_m(i) is the atom j of i's species
 *      with the smallest |c|^2, the smallest j on ties, and delta_{m,i} the delta of that pair.  partner[m, a] = p_m(i) for the
 *      atom a = offsets[b] + i ([max_ops, N]; -1 for m >= n_ops).
 *   3. refined translations.  mean_m = (sum_i delta_{m,i}) / n, summed in atom order from 0; ops_shift_m = -mean_m and
 *      ops_translation_m = t'_m = t_m - mean_m (not wrapped): the least-squares translation for the permutation p_m.  The
 *      refined operations close under composition; unused slots hold zeros.
 *   4. positions.  frac_out_i = wrap(w_i + (sum_m V_m (mean_m - delta_{m,i})) / n_ops), V_m the integer inverse of W_m
 *      (adjugate x determinant), the sum in operation order from 0, each term (V_r0 g_0 + V_r1 g_1) + V_r2 g_2: the mean over the
 *      group of the partners carried back, V_m (w_{p_m(i)} - t'_m).  The result is invariant under every (W_m, t'_m) up to
 *      rounding.  A crystal whose only operation is the identity returns w bit for bit.
 *   5. metric.  G' = (sum of W^T G W over the distinct rotations) / their number, summed in code order (the stored operations
 *      are sorted by code: a rotation is distinct when its code differs from the one before); W^T G W is formed as the search's
 *      rule 2 forms it, a'_j = (W_0j a_0 + W_1j a_1) + W_2j a_2 and G'_ij = a'_i . a'_j.  lengths_i = sqrt(G'_ii); angles_i =
 *      acos(G'_jk / (lengths_j lengths_k)) in radians, j, k the other two axes, the quotient clamped to [-1, 1]; lattice is rebuilt
 *      from them as the sampler builds its cells (arreau_lattice_from_params' orientation), so (lengths, angles, lattice) is the
 *      representation the sampler uses.  frac_out is fractional and holds in either orientation.
 *   6. orbits.  orbit[i] = the smallest p_m(i) over m (local to the crystal), orbit_size[i] = the number of distinct p_m(i),
 *      site_order[i] = n_ops / orbit_size[i]; n_orbits = the number of atoms with orbit[i] = i.
 *   7. displacements.  u_i = frac_out_i before the wrap minus w_i, |u_i| in the INPUT cell; max_displacement = sqrt(max |u|^2),
 *      rms_displacement = sqrt((sum |u|^2) / n), in A.
 *   8. arithmetic: as the symmetry search's rule 7 -- one float32 operation at a time, rounded to nearest, in the order written,
 *      never contracted; divisions correctly rounded.  Only acos and the rebuilt lattice use the device's elementary functions.
 *      The float64 restatement (arreau_amd/diffusion/symmetrize.py) is compared on guarded inputs (every decision quantity of
 *      the search and the nearest against the second-nearest partner at most symprec / 2 or at least 2 symprec); the bounds on the
 *      reals are derived there.
 * The partner maps are held in global memory (out->partner), for crystals of any size.  Cost: n_ops x n^2 distance evaluations
 * per crystal and as many integer comparisons.  Offsets outside [0, N] or descending are clamped as in the screen.  Does not
 * synchronise.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL found / result / arrays, negative sizes, max_ops outside
 * 1..ARREAU_SYM_MAX_OPS_CAP. */
#define ARREAU_SYMZ_NONFINITE 1
#define ARREAU_SYMZ_CELL 2
#define ARREAU_SYMZ_EMPTY 4
#define ARREAU_SYMZ_NO_GROUP 8
#define ARREAU_SYMZ_NOT_A_PERMUTATION 16
typedef struct arreau_symmetrize_result { /* DEVICE arrays */
    float* frac_out;         /* [N,3] at the input's offsets */
    float* lattice;          /* [B,3,3] rows a, b, c rebuilt from lengths and angles */
    float* lengths;          /* [B,3] A */
    float* angles;           /* [B,3] radians */
    int32_t* orbit;          /* [N] the orbit's first atom, local to the crystal */
    int32_t* orbit_size;     /* [N] */
    int32_t* site_order;     /* [N] n_ops / orbit_size */
    int32_t* n_orbits;       /* [B] */
    float* max_displacement; /* [B] A */
    float* rms_displacement; /* [B] A */
    float* ops_translation;  /* [B, max_ops, 3] the refined t'_m, zeros in unused slots */
    float* ops_shift;        /* [B, max_ops, 3] t'_m - t_m: the mean difference of operation m */
    int32_t* partner;        /* [max_ops, N] p_m(i), local to the crystal; -1 in unused rows */
    int32_t* flags;          /* [B] ARREAU_SYMZ_* */
} arreau_symmetrize_result;
/* d_frac[N,3], d_types[N] species ids (required), d_lattice[B,3,3] rows a, b, c.  `found` and `out` are HOST pointers. */
int arreau_crystal_symmetrize(const float* d_frac, const int32_t* d_types, const float* d_lattice, const int32_t* d_crystal_offsets,
                              int32_t B, int32_t N, const arreau_symmetry_result* found, int32_t max_ops,
                              arreau_symmetrize_result* out, void* stream);

/* ---- conventional cell: the conventional basis, centring, Bravais lattice and atoms of a reduced crystal ----------------------
 * The seventh per-crystal instrument: arreau_crystal_reduce gives a crystal's primitive, Delaunay-reduced cell and
 * arreau_crystal_symmetry, run on THAT cell, its rotations; this entry point turns them into the cell a crystallographer reads:
 * the conventional basis of the crystal family, the centring (P, A, B, C, I, F, R), the Bravais lattice (aP, mP, mS, oP, oS, oI,
 * oF, tP, tI, hR, hP, cP, cI, cF) and the atoms of the conventional cell.  It neither reduces nor searches: the caller runs the
 * three launches in order (reduce, search on the reduced batch, this one).  One launch, one workgroup of four waves per crystal,
 * no atomics, no second stream, no arreau_model; deterministic.  NOT computed: a space-group number, an origin shift, the ITA
 * standard choice among the monoclinic centrings (A, C and I all count as mS), an idealised metric (the cell keeps its noise; to
 * idealise, symmetrize the conventional crystal afterwards).
 * The batch (d_frac, d_types, d_lattice, d_crystal_offsets) is primitive and Delaunay-reduced; `found` is the result of
 * arreau_crystal_symmetry on the same arrays (a HOST struct of device pointers; n_ops, ops_rotation, point_group and flags are
 * read), max_ops its row width.  Conventions as in the symmetry search: a lattice vector is an integer row v (v L in space), a
 * rotation W acts on columns, v' = W v; the rotations of a Delaunay-reduced cell have entries in {-1, 0, 1}, so every step below
 * but the comparison of lengths is exact integer arithmetic.  |v|^2 of an integer row: c_d = (v_0 L_0d + v_1 L_1d) + v_2 L_2d,
 * (c_x c_x + c_y c_y) + c_z c_z, as the cell reduction forms it.  Per crystal, with the distinct stored rotations in code order:
 *   1. flags.  NONFINITE, CELL and EMPTY as in arreau_crystal_symmetry's rule 1.  NO_GROUP: the search flagged the crystal
 *      AMBIGUOUS, OVERFLOW or NOT_A_GROUP, or n_ops lies outside 1..max_ops, or point_group outside 0..31, or a stored code is no
 *      matrix of determinant +-1, or there are more than 48 distinct rotations.  NO_BASIS: rules 2-5 give no basis or a check of
 *      rule 5 fails.  A crystal with any flag is copied through unchanged, bit for bit (positions not wrapped): lattice = the
 *      input's, transform = identity, centring 0, bravais = -1, n_points = 1, num_atoms = n, source = 0..n-1.
 *   2. proper parts and axes.  W' = det(W) W; its order from its trace: 3 -> 1, -1 -> 2, 0 -> 3, 1 -> 4, 2 -> 6 (anything else:
 *      NO_BASIS).  S = sum_{j < order} W'^j has rank 1: the axis is its first non-zero column and the normal of the perpendicular
 *      lattice plane {v : S v = 0} its first non-zero row, each divided by the gcd of its entries and given a positive first
 *      non-zero entry.  "The first part of order k" is the first in code order.
 *   3. shortest plane vectors.  The integer rows v != 0 with entries in -3..3 and normal . v = 0, enumerated in lexicographic
 *      order from (-3, -3, -3), v_0 slowest; the shortest is the first of the smallest |v|^2 (a strict float32 comparison).
 *   4. basis by family (point_group 0-1 triclinic, 2-4 monoclinic, 5-7 orthorhombic, 8-14 tetragonal, 15-26 trigonal and
 *      hexagonal, 27-31 cubic).  Every rule yields a set of integer candidates P (rows a, b, c); the right-handed ones (det P >
 *      0) are kept and the lexicographically smallest P, read row by row, wins: vectors the group maps onto each other are
 *      equally long, and integers, not floats, choose among them.
 *        triclinic     the cell as given, P = identity.
 *        monoclinic    b = +- the axis of the first part of order 2; a the shortest vector of its plane, c the shortest not
 *                      parallel to a, negated when a . c > 0 (float32, (x x' + y y') + z z'); candidates (s a, t b, s c), s, t = +-1.
 *        orthorhombic  the three distinct axes of the parts of order 2, sorted by |v|^2 (ties to the first found); when that
 *                      order makes the lattice A-centred the axes are taken as (second, third, first), when B-centred as (first,
 *                      third, second): the centred face becomes C with |a| <= |b|; candidates: every sign of the three.
 *        tetragonal    c = the axis of the first part R of order 4; a0 the shortest vector of its plane; candidates (a, R a, c) and
 *                      (a, R^-1 a, c) for a = +- R^j a0.
 *        trig., hex.   c = the axis of the first part of order 6, of order 3 when there is none; R the first part of order 3;
 *                      candidates as for tetragonal; with det P = 3 only those in the obverse setting (rule 5's R set) are kept.
 *        cubic         the three distinct axes of the parts of order 4, of order 2 when there is none; candidates: every order
 *                      and every sign of the three.
 *   5. transform, centring and checks, all exact.  n_points = det P must lie in 1..4.  The centring translations are the integer
 *      combinations of the rows of adj(P) modulo n_points (numerators over n_points), sorted lexicographically: exactly
 *      n_points of them, and one of the sets P {0}; A {0, (0,1,1)/2}; B {0, (1,0,1)/2}; C {0, (1,1,0)/2}; I {0, (1,1,1)/2}; F {0,
 *      (0,1,1)/2, (1,0,1)/2, (1,1,0)/2}; R {0, (1,2,2)/3, (2,1,1)/3} (obverse).  The family admits: triclinic P; monoclinic P, A,
 *      C, I; orthorhombic P, C, I, F; tetragonal P, I; trigonal and hexagonal P, R; cubic P, I, F.  Every distinct rotation in
 *      the conventional basis, adj(P)^T W P^T / n_points, must be an integer matrix.  Any failure: NO_BASIS.
 *   6. cell.  lattice row r = (P_r0 L_0d + P_r1 L_1d) + P_r2 L_2d; lengths_r = sqrt of its squared length; angles_i = acos of
 *      (row_j . row_k) / (lengths_j lengths_k), j, k the other two, clamped to [-1, 1], in radians: the sampler's representation,
 *      as the symmetrization reports it.  bravais = 0..13 in the order above; centring = 0..6 for P, A, B, C, I, F, R.
 *   7. atoms.  num_atoms = n x n_points.  Output atom k n + i is atom i under the k-th centring translation, in their sorted
 *      order: frac_out_c = wrap((((w_0 A_0c + w_1 A_1c) + w_2 A_2c) + num_kc) / n_points), A = adj(P), w the wrapped input
 *      position; types_out its species and source = i.  Crystal b's atoms start at 4 x offsets[b] (the per-atom arrays hold 4 N
 *      rows); the slots beyond num_atoms hold zeros, species -1 and source -1.
 *   8. arithmetic: one float32 operation per step, rounded to nearest, in the order written, never contracted; the division and
 *      the square roots correctly rounded; only acos is the device's.  The float64 restatement
 *      (arreau_amd/diffusion/conventional_cell.py) reports the relative gap of every float comparison that decided; on guarded
 *      inputs (every gap at least 1e-3) the integer outputs agree and the reals are held to the bounds derived there.
 * Cost: the basis is found by one thread per crystal (a few thousand integer operations and at most 2 x 342 squared lengths);
 * the atoms are written by the workgroup.  Offsets outside [0, N] or descending are clamped as in the screen.  Does not
 * synchronise.
 * Argument errors (ARREAU_EINVAL, nothing launched): NULL found / result / arrays, negative sizes, max_ops outside
 * 1..ARREAU_SYM_MAX_OPS_CAP. */
#define ARREAU_CONV_NONFINITE 1
#define ARREAU_CONV_CELL 2
#define ARREAU_CONV_EMPTY 4
#define ARREAU_CONV_NO_GROUP 8
#define ARREAU_CONV_NO_BASIS 16
typedef struct arreau_conventional_result { /* DEVICE arrays: one row per crystal, then 4 N rows of atoms */
    float* lattice;      /* [B,3,3] rows a, b, c of the conventional cell, P L */
    float* lengths;      /* [B,3] A */
    float* angles;       /* [B,3] radians */
    int32_t* transform;  /* [B,3,3] P: rows, the conventional vectors in the reduced basis */
    int32_t* centring;   /* [B] 0..6: P, A, B, C, I, F, R */
    int32_t* bravais;    /* [B] 0..13: aP, mP, mS, oP, oS, oI, oF, tP, tI, hR, hP, cP, cI, cF; -1: none */
    int32_t* n_points;   /* [B] det P: lattice points per conventional cell */
    int32_t* num_atoms;  /* [B] n x n_points */
    int32_t* flags;      /* [B] ARREAU_CONV_* */
    float* frac_out;     /* [4N,3] crystal b's atoms at 4 offsets[b] .. 4 offsets[b] + num_atoms[b] */
    int32_t* types_out;  /* [4N] */
    int32_t* source;     /* [4N] the reduced-cell atom (local to the crystal) of every output atom, -1 beyond num_atoms */
} arreau_conventional_result;
/* d_frac[N,3], d_types[N] species ids (required), d_lattice[B,3,3] rows a, b, c.  `found` and `out` are HOST pointers. */
int arreau_crystal_conventional(const float* d_frac, const int32_t* d_types, const float* d_lattice, const int32_t* d_crystal_offsets,
                                int32_t B, int32_t N, const arreau_symmetry_result* found, int32_t max_ops,
                                arreau_conventional_result* out, void* stream);

/* ---- structure match: is crystal x that crystal y, under which map, and how far off in A ------------------------------------
 * The sixth instrument: for every pair (x, y) of a pair list, x a crystal of batch X and y one of batch Y (Y may be X), the
 * change of basis W and the translation under which y's atoms fall next to x's, the atom-to-atom map and the root-mean-square
 * displacement, in A and normalised as pymatgen's StructureMatcher normalises it.  One launch, one workgroup of four waves per
 * pair, no atomics, no arreau_model, no synchronisation; deterministic.  Where the nearest-partner map of a candidate is no
 * permutation the candidate is skipped (rule 6) unless the assignment mode OPTIMAL is asked for (arreau_structure_match_assigned):
 * then the optimal (Hungarian-type) assignment is solved for it, rule 6b.  NOT computed: supercells, formula reduction
 * or anonymous species (the species multisets are compared exactly: run arreau_crystal_reduce first); a rescaling of the cells
 * to one volume; a mapping W with an entry outside {-1, 0, 1} (complete for two Delaunay-reduced cells, rule 2).
 * Conventions as in the symmetry search: cell rows a_0, a_1, a_2, fractional columns, the metric G = L L^T, column j of W the
 * image of basis vector j, the code of W sum (W_rc + 1) 3^(3r + c).  w_i: x's wrapped positions, v_j: y's (the screen's rule 5).
 *   1. flags per pair.  BAD_PAIR (alone, nothing is read through the indices): an index outside its batch, or x has more atoms
 *      than partner_stride.  NONFINITE (alone): a non-finite cell entry or coordinate in either crystal.  Else any of CELL
 *      (either volume not positive or not finite), EMPTY (either crystal has no atoms), DIFFERENT (the atom counts differ, or
 *      some species has another number of atoms in y than in x).  A pair with one of these five reports rms = rms_norm =
 *      max_dist = +inf, mapping = -1, translation 0, matched = 0, partner -1 and the three counts 0.
 *   2. lattice mappings.  Every W with entries in {-1, 0, 1} and det +-1 (det -1 included: the match is blind to handedness, as
 *      StructureMatcher is), in code order; G' = W^T G_y W is formed as the search's rule 2 forms it, a'_j = (W_0j a_0 + W_1j a_1)
 *      + W_2j a_2 of y's rows and G'_ij = a'_i . a'_j.  W is accepted when |sqrt(G'_ii) - sqrt(Gx_ii)| <= ltol sqrt(Gx_ii) for every
 *      i and |angle'_i - angle^x_i| <= angle_tol for every i, angle_i = acos(G_jk / (len_j len_k)), j, k the other two axes, the
 *      quotient clamped to [-1, 1] (the symmetrization's rule 5).  n_mappings counts every accepted W; the first max_mappings are
 *      used, OVERFLOW when there are more; NO_MAPPING when there are none (the outputs of rule 1, n_mappings 0).
 *   3. y in the mapped basis: v'_j = wrap(V v_j), V = W^-1 = det x adj(W), an exact integer matrix (entries up to +-2), each row
 *      (V_r0 v_0 + V_r1 v_1) + V_r2 v_2.
 *   4. metric of the comparison.  G_m = (G_x + G') / 2, entry by entry.  dist^2 of a fractional difference: each component minus
 *      its nearest integer (rintf), then the smallest e G_m e^T over the 27 images e + s, s in {-1, 0, 1}^3, s_0 slowest, the first
 *      on ties; g_r = (G_r0 e_0 + G_r1 e_1) + G_r2 e_2, e G e^T = (e_0 g_0 + e_1 g_1) + e_2 g_2, a rounded result below 0 becomes 0.
 *      The normalisation length is l = cbrt(sqrt(det G_m) / n), det G_m expanded along its first row.
 *   5. candidate translations.  The species of x with the fewest atoms (the smallest id on ties), its first atom p0; for every
 *      atom q of y of that species, ascending: t = wrap(w_p0 - v'_q).  n_candidates = used mappings x atoms of that species.
 *   6. test of (W, q).  For every atom i of x, p(i) is the atom j of y of i's species with the smallest dist^2 of (v'_j + t) - w_i,
 *      the smallest j on ties, and e_i the difference of the image that attains it.  A candidate whose p is not one-to-one is
 *      dropped; n_permutations counts the others.  For those t' = t - (sum_i e_i) / n, summed in atom order from 0: the
 *      least-squares translation of that map (not wrapped); d_i^2 = dist^2 of (v'_p(i) + t') - w_i, rms = sqrt((sum_i d_i^2) / n),
 *      max_dist = sqrt(max_i d_i^2).  Where the nearest-partner map is a permutation it is the optimal assignment.
 *  6b. assignment OPTIMAL (arreau_structure_match_assigned; NEAREST is rule 6 as it stands).  A candidate whose p is not one-to-one
 *      is not dropped: its map becomes the one-to-one, species-preserving map that minimises sum_i c(i, p(i)), c(i, j) = dist^2 of
 *      (v'_j + t) - w_i exactly as rule 4 forms it in float32, at the UNREFINED t of rule 5, each c rounded to the nearest multiple
 *      of 2^-24 A^2 and the sums formed exactly (64-bit integers), so the minimum does not depend on an order of operations; pairs
 *      of different species are excluded.  Rule 1 makes such a map exist, so every candidate survives and NO_PERMUTATION is not
 *      set.  e_i is the difference of the image that attains dist^2 for the chosen partner; from there rule 6 goes on unchanged:
 *      t' = t - (sum_i e_i) / n in atom order, the distances once more under t', rms and max_dist -- one pass, as
 *      StructureMatcher._cart_dists does it.  The solver is a shortest-augmenting-path one (Jonker-Volgenant): column duals start
 *      at 0, a row keeps its nearest partner when it is the smallest row that claims that column, the remaining (free) rows are
 *      augmented in ascending i, and the unscanned column of the smallest reduced distance is taken next, ties to the smallest j.
 *      Where several maps attain the minimum, this order decides; it depends on the inputs alone, not on the launch.
 *      n_permutations keeps its meaning (the candidates whose nearest-partner map was one-to-one; n_candidates - n_permutations
 *      were solved), and the flag ASSIGNED (informational: it does not make a pair unmatched) says that the winning candidate's
 *      map came from this step.
 *   7. result.  The candidate of the smallest rms, ties to the smaller code, then the smaller q: rms and max_dist in A, rms_norm =
 *      rms / l, mapping = the code of W, translation = t', partner[p, i] = p(i) (local to y; -1 from x's atom count to
 *      partner_stride), matched = (rms_norm <= stol).  NO_PERMUTATION when mappings exist and no candidate survived (the outputs
 *      of rule 1 with n_mappings and n_candidates as counted).
 *   8. arithmetic: as the symmetry search's rule 7 -- one float32 operation at a time, rounded to nearest, in the order written,
 *      never contracted; divisions and square roots correctly rounded.  Only acos and cbrt come from the device library.  The
 *      float64 restatement (arreau_amd/diffusion/structure_match.py) is compared on guarded inputs; the bounds on the reals are
 *      derived there.
 *   9. argument errors (ARREAU_EINVAL, nothing launched): NULL params / result / arrays, negative sizes, ltol, angle_tol or stol
 *      not finite or not positive, max_mappings outside 1..ARREAU_SM_MAX_MAPPINGS_CAP, a partner_stride above 256 without scratch.
 *      P = 0 is a no-op.  arreau_structure_match_assigned also: an assignment outside {0, 1}; OPTIMAL with a partner_stride above
 *      ARREAU_SM_ASSIGN_LDS_ATOMS and d_cost NULL.
 * Crystals of up to 256 atoms keep their coordinates, species and the four partner maps under test in LDS; larger ones read global
 * memory and keep the maps in out->scratch (the same values).  Cost: n_mappings x n_rarest x n^2 x 27 metric evaluations per pair.
 * Offsets outside [0, N] or descending are clamped as in the screen. */
#define ARREAU_SM_NONFINITE 1
#define ARREAU_SM_CELL 2
#define ARREAU_SM_EMPTY 4
#define ARREAU_SM_DIFFERENT 8
#define ARREAU_SM_BAD_PAIR 16
#define ARREAU_SM_NO_MAPPING 32
#define ARREAU_SM_OVERFLOW 64
#define ARREAU_SM_NO_PERMUTATION 128
#define ARREAU_SM_ASSIGNED 256 /* informational: the winning candidate's map came from the assignment step (rule 6b) */
#define ARREAU_SM_MAX_MAPPINGS_CAP 4096
#define ARREAU_SM_ASSIGN_NEAREST 0
#define ARREAU_SM_ASSIGN_OPTIMAL 1
#define ARREAU_SM_ASSIGN_LDS_ATOMS 24  /* crystals of up to this many atoms keep the four cost matrices under test in LDS */
#define ARREAU_SM_ASSIGN_STATE_ROWS 6  /* rows of solver state behind every cost matrix of d_cost */
typedef struct arreau_structure_match_params {
    float ltol;           /* relative tolerance on the cell lengths; default 0.2 (StructureMatcher's) */
    float angle_tol;      /* radians; default 5 degrees */
    float stol;           /* on rms_norm; default 0.3 */
    int32_t max_mappings; /* lattice mappings tried per pair, 1..ARREAU_SM_MAX_MAPPINGS_CAP; default 192 */
} arreau_structure_match_params;
typedef struct arreau_structure_match_result { /* DEVICE arrays, one row per pair */
    float* rms;              /* [P] A */
    float* rms_norm;         /* [P] rms / l */
    float* max_dist;         /* [P] A */
    int32_t* mapping;        /* [P] the code of W, -1: none */
    float* translation;      /* [P,3] t' */
    int32_t* partner;        /* [P, partner_stride] p(i), local to y */
    int32_t* n_mappings;     /* [P] every accepted W, also beyond max_mappings */
    int32_t* n_candidates;   /* [P] */
    int32_t* n_permutations; /* [P] */
    int32_t* matched;        /* [P] 0 / 1 */
    int32_t* flags;          /* [P] ARREAU_SM_* */
    int32_t* scratch;        /* [P, 4, partner_stride] the maps under test of crystals above 256 atoms; may be NULL when
                                partner_stride <= 256 */
    int32_t partner_stride;  /* the row width of partner: at least the atom count of every x in the pair list */
} arreau_structure_match_result;
/* x_* / y_*: a batch each, frac[N,3], types[N] species ids, lattice[B,3,3] rows a, b, c, offsets[B+1]; d_pairs[P,2] (x, y) indices
 * (device).  `params` and `out` are HOST pointers. */
int arreau_structure_match(const float* x_frac, const int32_t* x_types, const float* x_lattice, const int32_t* x_offsets, int32_t Bx,
                           int32_t Nx, const float* y_frac, const int32_t* y_types, const float* y_lattice, const int32_t* y_offsets,
                           int32_t By, int32_t Ny, const int32_t* d_pairs, int32_t P, const arreau_structure_match_params* params,
                           arreau_structure_match_result* out, void* stream);
/* The same with the assignment mode of rule 6b: ARREAU_SM_ASSIGN_NEAREST is arreau_structure_match bit for bit, ARREAU_SM_ASSIGN_OPTIMAL
 * solves the assignment of every candidate whose nearest-partner map is not one-to-one.  d_cost: device scratch of
 * P x 4 x (partner_stride + ARREAU_SM_ASSIGN_STATE_ROWS) x partner_stride floats -- per pair and wave a cost matrix
 * [partner_stride, partner_stride] and the rows of solver state (used by crystals above 256 atoms; smaller ones keep it in LDS);
 * may be NULL when partner_stride <= ARREAU_SM_ASSIGN_LDS_ATOMS or assignment is NEAREST.  Its contents are not an output. */
int arreau_structure_match_assigned(const float* x_frac, const int32_t* x_types, const float* x_lattice, const int32_t* x_offsets, int32_t Bx,
                                    int32_t Nx, const float* y_frac, const int32_t* y_types, const float* y_lattice,
                                    const int32_t* y_offsets, int32_t By, int32_t Ny, const int32_t* d_pairs, int32_t P,
                                    const arreau_structure_match_params* params, arreau_structure_match_result* out, int32_t assignment,
                                    float* d_cost, void* stream);

/* ---- the score network ---------------------------------------------------------------------- */

/* One evaluation of DiffusionLoss.predict_scores (diffusion/diffusion_loss.py:112-197):
 * feature assembly (:124-158), PBC neighbour list (:164-180) unless `use_given_edges`, and
 * PonitaFiberBundle.forward (ponita/models/ponita.py:88-123) with the read-outs of :126-155.
 *   d_frac[N,3], d_types[N] (class index), d_lengths[B,3], d_angles[B,3],
 *   d_t[B] timestep per crystal (the time feature is betas[t], diffusion_loss.py:126).
 * Outputs: d_eps[N,3] (pred_frac_eps_x), d_logits[N,S], d_len0[B,3] (pred_lengths_0).
 * When use_given_edges != 0 the slot arrays d_deg/d_src/d_dir/d_dist are inputs (teacher-forced
 * graph); otherwise they are outputs of the internal neighbour search and may be NULL to use
 * workspace storage.  Of a given graph only slots [0, min(d_deg[i], k)) of receiver i are read as
 * data: the rest may hold anything (NaN included) without changing an output bit. */
int arreau_predict_scores(const arreau_model* model,
                          const float* d_frac, const int32_t* d_types, const float* d_lengths,
                          const float* d_angles, const int32_t* d_t,
                          const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                          int32_t use_given_edges,
                          int32_t* d_deg, int32_t* d_src, float* d_dir, float* d_dist,
                          float* d_eps, float* d_logits, float* d_len0,
                          void* d_workspace, size_t workspace_bytes, void* stream);

/* The inner operator seam: `model(batch)` at diffusion/diffusion_loss.py:183-189, i.e. PonitaFiberBundle.forward
 * (ponita/models/ponita.py:88-123) on the batch attributes the reference assembles at diffusion_loss.py:156-180:
 *   d_x[N, S+74]   batch.x   scalar node features (any values: the embedding is the general x . W^T, :98)
 *   d_vec[N,4,3]   batch.vec (fractional coordinate, then the three lattice rows; diffusion_loss.py:158)
 *   d_lattice[B,3,3] batch.lattice (only the edge cosine features read it, transforms/invariants.py:82-85)
 *   d_crystal_offsets[B+1]  CSR form of batch.batch / batch.num_atoms (atoms of a crystal contiguous)
 *   slot-form edges (arreau_edges_to_slots converts batch.edge_index / dists / inter_atom_direction).
 * Outputs: the reference's return tuple (ponita.py:123) without its None entries:
 *   d_logits[N,S] (output_scalar), d_vec_out[N,1,3] (output_vec), d_global_scalar[B,3] (global_add_pool, :152). */
int arreau_ponita_forward(const arreau_model* model, const float* d_x, const float* d_vec, const float* d_lattice,
                          const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                          const int32_t* d_deg, const int32_t* d_src, const float* d_dir, const float* d_dist,
                          float* d_logits, float* d_vec_out, float* d_global_scalar,
                          void* d_workspace, size_t workspace_bytes, void* stream);

/* The four state updates of one loop iteration (diffusion/diffusion_loss.py:338-347):
 * VP_lattice.reverse_given_x0 on lengths with pred_lengths_0 * num_atoms
 * (diffusion_helpers.py:185-199), lattice_from_params, VE_pbc.reverse on the fractional
 * coordinates (diffusion_helpers.py:65-81) and D3PM.reverse on the atom types (d3pm.py:198-215).
 * Noise is supplied by the caller in the reference's draw order: d_z_lattice[B,3] ~ N(0,1),
 * d_z_frac[N,3] ~ N(0,1), d_u_types[N,S] ~ U[0,1).  State is updated in place; d_lattice[B,3,3]
 * receives the new cell. */
int arreau_reverse_step(const arreau_model* model,
                        float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                        const int32_t* d_t, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                        const float* d_eps, const float* d_logits, const float* d_len0,
                        const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                        float* d_lattice, void* stream);

/* The hot loop of DiffusionLoss.sample (diffusion/diffusion_loss.py:318-347) enqueued in ONE call: for timestep
 * t_start, t_start-1, ..., t_start-n_steps+1 (the reference runs T-1 .. 1): arreau_predict_scores, then the reverse
 * updates with the three draws of the step (diffusion_helpers.py:193-197, :79; d3pm.py:206) generated INSIDE the update
 * kernels from Philox4x32-10 keyed by (seed, timestep, draw, element) -- no RNG launches, no noise arrays, no host work
 * between steps; the timestep lives on the device.  State (d_frac, d_types, d_lengths) is updated in place, d_lattice
 * [B,3,3] receives the final cell.  d_const_types (may be NULL): species re-imposed after every step
 * (use_constant_atomic_symbols, lightning_wrappers/diffusion.py:231-236).  d_fixed_lengths[B,3] (may be NULL): the
 * same idea for the cell -- fixed-cell sampling, the given lengths re-imposed after every step (an extension; the
 * reference has no counterpart; bench.py uses it to keep the synthetic checkpoint's cells at the sampler's density).
 * use_graph != 0 captures one step into a
 * hipGraph and replays it (same trajectory; pays for itself only on small, launch-bound batches).
 * Does not synchronise. */
int arreau_sample_loop(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                       const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                       uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                       void* d_workspace, size_t workspace_bytes, int32_t use_graph, void* stream);

/* ---- conditioned sampling (structure completion) ---------------------------------------------------------------
 * Known atoms, species and cells held to a template while the rest is generated: RePaint-style replacement (Lugmayr et
 * al., CVPR 2022) without resampling jumps.  Every pointer is a DEVICE pointer and may be NULL; masks hold one byte per
 * atom / crystal, nonzero = known; a mask needs its values, values without a mask are ignored.
 *   x0[N,3], pos_mask[N]: known fractional coordinates;  a0[N], type_mask[N]: known class indices (z-table indices);
 *   l0[B,3], len_mask[B]: known cell lengths.
 * The state at time tau is (frac, types, lengths); the update of the step that leaves timestep t produces tau = t - 1 (in a
 * respaced loop, tau = s, the scheduled successor of t: see the section below).
 *   1. positions: after the VE reverse update, frac = remainder(x0 + ve_sigmas[tau] * z, 1),
 *      z = Philox normal (seed, t, kind 3, element 3 i + d); at tau = 0 exactly remainder(x0, 1).  This is VE_pbc.forward
 *      at tau (diffusion/diffusion_helpers.py:43-47).
 *   2. lengths: after VP_lattice.reverse_given_x0, l = sqrt(abar[tau]) l0 + sqrt(1 - abar[tau]) z,
 *      z = Philox normal (seed, t, kind 4, element 3 b + d); at tau = 0 exactly l0.  This is VP_lattice.forward
 *      (diffusion_helpers.py:156-163).  The replacement comes before the cell (and the next step's set-up) is formed.
 *   3. angles: the caller writes the template's angles (radians, matrix_to_params of the template cell,
 *      lattice_helpers.py:16-35) into d_angles for the known cells; the others keep the host-drawn monoclinic angles.
 *   4. species: the known class is re-imposed after every D3PM update (per atom, like d_const_types, which it overrides).
 *   5. initial state: arreau_condition_initial_state overwrites the known components of a drawn initial state at
 *      tau = t_start by rules 1, 2 and 4 with Philox timestep key t_start + 1.
 * Kinds 3 and 4 are draws of their own: every unknown atom or crystal draws exactly what it draws without a condition.
 * The reference's constant_atoms (diffusion/diffusion_loss.py:289, 311-312, 345-346) is the case "every species known". */
typedef struct arreau_sample_condition {
    const float* x0;
    const uint8_t* pos_mask;
    const int32_t* a0;
    const uint8_t* type_mask;
    const float* l0;
    const uint8_t* len_mask;
} arreau_sample_condition;

/* arreau_sample_loop with a condition (rules above; `cond` is a host pointer to the struct, NULL = unconditioned).  The
 * condition's device pointers are part of what a cached hipGraph was captured for: another condition is captured anew. */
int arreau_sample_loop_conditioned(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                   const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                                   uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                   void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                   const arreau_sample_condition* cond, void* stream);

/* Rule 5: the known components of an initial state drawn for timestep t_start (in place, d_frac[N,3], d_types[N],
 * d_lengths[B,3]), before the first arreau_sample_loop_conditioned call of the run. */
int arreau_condition_initial_state(const arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, int32_t B,
                                   int32_t N, int32_t t_start, uint64_t seed, const arreau_sample_condition* cond,
                                   void* stream);

/* ---- respaced sampling (fewer denoising steps) -----------------------------------------------------------------
 * The loop runs on a strictly descending schedule t_1 > t_2 > ... > t_K of trained timesteps with t_1 <= T-1 and t_K = 1
 * ("respacing", Nichol & Dhariwal 2021, section 4).  The step that leaves t_i produces the state at s = t_{i+1}; the step at
 * t_K = 1 produces s = 0.  The network is evaluated at t as before; every process jumps from t to s in closed form, float32,
 * the reference's own formulas with t - 1 replaced by s:
 *   1. VE positions (diffusion_helpers.py:65-81): mean = x_t - eps (sig_t^2 - sig_s^2),
 *      std = sqrt(sig_s^2 (sig_t^2 - sig_s^2) / sig_t^2), x_s = remainder(mean + std z, 1), sig = ve_sigmas.
 *   2. VP lengths (reverse_given_x0, :185-199): beta = min(1 - abar_t / abar_s, lattice_clipmax), alpha = 1 - beta,
 *      mean = (sqrt(abar_s) beta x0 + sqrt(alpha) (1 - abar_s) x_t) / (1 - abar_t), var = (1 - abar_s) beta / (1 - abar_t),
 *      l_s = mean + var z (the reference's variance, not its square root), z = 0 for t <= 1.
 *   3. D3PM species (d3pm.py:74-110, 198-215): for t > 1 the posterior logits are
 *      log(Qbar_{t-s}[:, x_t] + eps) + log(softmax(x0_logits) . Qbar_s + eps), Qbar_k = q_mats[k-1] (the mask chain is
 *      time-homogeneous, so the (t-s)-step transition is Qbar_{t-s}); at t = 1 the raw x0 logits.  Gumbel scale and tie rule
 *      as in arreau_reverse_step.
 *   4. a stride-1 step (s = t - 1) uses the model's tables as arreau_reverse_step does (betas[t], q_one_step_transposed,
 *      q_mats[t-2]): the full schedule T-1, ..., 1 is the schedule-less loop bit for bit.
 *   5. the network input of the next step is evaluated at s (its per-crystal embedding is prepared for s).
 *   6. conditioned sampling: a known component is the template noised to tau = s (rules 1, 2 of the section above, with the
 *      draw (seed, t, kind 3/4)), exactly the template at s = 0; rule 5 (the initial state) uses t_start = t_1.
 *   7. noise keys do not change: the step at t draws (seed, t, kind, element), so a respaced run uses, at every timestep it
 *      visits, the draws a full run uses there.
 * Valid targets are s = 0 at t = 1 and 1 <= s <= t - 1 for t > 1; any other s is clamped into that range and sets
 * ARREAU_STATUS_BAD_TIMESTEP.  No claim on sample quality at a given K is made here (there is no trained checkpoint to judge it).
 *
 * d_next[T+1] (device, int32): the schedule as a next-timestep table, d_next[t_i] = t_{i+1}, d_next[1] = 0, and for every
 * t_i also d_next[t_i + 1] = t_i (a loop starts "one above" its first timestep: its first launch advances the device
 * timestep; when t_i + 1 is itself scheduled this holds already).  A loop call may then start at any scheduled timestep,
 * which is how a run is cut into segments (frames).  lattice_clipmax: VP_lattice's clipmax (0.999 by default). */
typedef struct arreau_sample_schedule {
    const int32_t* d_next;
    float lattice_clipmax;
} arreau_sample_schedule;

/* arreau_sample_loop_conditioned on a schedule: n_steps steps from t_start (a scheduled timestep, 1 <= t_start <= T-1) along
 * d_next.  `schedule` is a host pointer, NULL = every timestep (arreau_sample_loop_conditioned).  The table pointer and the
 * clip are part of what a cached hipGraph was captured for. */
int arreau_sample_loop_scheduled(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                 const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                                 uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                 void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                 const arreau_sample_condition* cond, const arreau_sample_schedule* schedule, void* stream);

/* arreau_reverse_step from timestep d_t[b] to d_s[B] (per crystal, rules above): the respaced step with the caller's noise,
 * for the loops with host-side noise and for parity tests.  At d_s[b] = d_t[b] - 1 it is arreau_reverse_step bit for bit. */
int arreau_reverse_step_to(const arreau_model* model,
                           float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                           const int32_t* d_t, const int32_t* d_s, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                           const float* d_eps, const float* d_logits, const float* d_len0,
                           const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                           float* d_lattice, float lattice_clipmax, void* stream);

/* ---- predictor-corrector sampling (Langevin corrector steps on positions) ----------------------------------------
 * Song et al. 2021 ("Score-Based Generative Modeling through SDEs", Algorithms 2 and 5): at every visited timestep t, M
 * Langevin "corrector" moves on the fractional coordinates come before the predictor step that leaves t.  The reference has
 * no corrector; this rule is the library's own.  Lengths, angles and species are never moved by a corrector.
 *   1. score: the network's eps for positions is trained on the wrapped displacement VE_pbc.forward returns (std sig_t;
 *      diffusion/diffusion_helpers.py:43-63, the loss at diffusion_loss.py:94-110) and the predictor moves against it, so the
 *      score estimate is g = -eps / sig_t^2, sig = ve_sigmas.
 *   2. step size (SNR rule, Algorithm 5), per crystal b: gamma_b = 2 (r |z_b| / |g_b|)^2, the norms over the 3 n components
 *      of the atoms the corrector moves in b; then x <- remainder(x + gamma_b g + sqrt(2 gamma_b) z, 1).  Evaluated as
 *      x <- remainder(x - a eps + c z, 1) with q = |z| / |eps|, a = 2 r^2 sig_t^2 q^2, c = 2 r sig_t^2 q (no quantity of size
 *      1 / sig^2 is formed).  A crystal whose |eps|^2 is 0 or not finite (or whose a, c are not finite) is left unmoved.
 *      r = snr (0.16 is Song et al.'s VE setting).
 *   3. order: "the step at t" = M corrections at t (each after a full network evaluation on the current state at t), then the
 *      predictor step that leaves t, on the network evaluated after the last correction.  Segment, frame and graph-replay
 *      boundaries stay between steps.  No corrector runs on the final state.
 *   4. noise: z = Philox normal (seed, t, kind 5, element 3 i + d) with the iteration index j = 0..M-1 in the counter's fourth
 *      word (0 for every other draw), so the predictor draws exactly what an uncorrected run draws.
 *   5. respacing: corrections run at every scheduled t.  Conditioning: known positions are not moved and are left out of the
 *      norms (a crystal with every position known is untouched); they keep the values the conditioning rules give them.
 *   6. limits: 0 <= M <= ARREAU_MAX_CORRECTOR_STEPS, and snr finite and > 0 when M > 0 (ARREAU_EINVAL otherwise). */
#define ARREAU_MAX_CORRECTOR_STEPS 16
typedef struct {
    int32_t steps; /* M */
    float snr;     /* r */
} arreau_corrector;

/* arreau_sample_loop_scheduled with M corrector steps per visited timestep (rules above; `corrector` is a host pointer, NULL or
 * steps == 0 = arreau_sample_loop_scheduled).  M and the snr are part of what a cached hipGraph was captured for. */
int arreau_sample_loop_corrected(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                 const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                                 uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                 void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                 const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                                 const arreau_corrector* corrector, void* stream);

/* One corrector move (rule 2) with the caller's noise d_z_frac[N,3], at timestep d_t[b] (1..T; another value is clamped and
 * sets ARREAU_STATUS_BAD_TIMESTEP) per crystal, in place on d_frac[N,3], from the network's d_eps[N,3]: for the loops with
 * host-side noise and for parity tests.  `condition` (host pointer, may be NULL): its position mask keeps those atoms unmoved
 * and out of the norms.  Fed arreau_philox_fill_word(seed, t, 5, j, ...), it is the loop's j-th correction bit for bit. */
int arreau_corrector_step(const arreau_model* model, float* d_frac, const int32_t* d_t, const int32_t* d_crystal_offsets,
                          int32_t B, int32_t N, const float* d_eps, const float* d_z_frac, float snr,
                          const arreau_sample_condition* condition, void* stream);

/* ---- RePaint resampling (jump back and re-denoise blocks of steps) ------------------------------------------------
 * Lugmayr et al., CVPR 2022, section 4.2 ("resampling"): the visited steps are cut into blocks of J; every block is run R
 * times, and every pass after the first starts with a jump of the whole state from the block's bottom back up to its top by
 * the forward process.  Replacement alone (conditioned sampling above) never pulls the unknown atoms into agreement with the
 * known ones; the jumps do.
 *   R = passes per block (RePaint's jump_n_sample; R = 1: no resampling), J = jump length in schedule steps (J >= 1).
 *   1. blocks: the steps a call visits are t_1 > ... > t_n (t_1 = t_start, n = n_steps); t_{n+1} is the successor of t_n (the
 *      schedule's next timestep, t - 1 without a schedule, 0 after 1).  Block k covers steps kJ+1 .. min(kJ+J, n); its top is
 *      t_{kJ+1}, its bottom t_{min(kJ+J,n)+1}.  Every block runs R passes; passes r = 1..R-1 each start with a jump from the
 *      bottom s up to the top t.  The last block may be shorter; the final block, whose bottom is 0, is resampled too.
 *   2. jump s -> t (0 <= s < t <= T, float32, per crystal), the forward process in closed form:
 *      positions  x <- remainder(x + sqrt(sig_t^2 - sig_s^2) z, 1), sig = ve_sigmas (sig_0 = ve_sigmas[0] = sigma_min), the
 *                 difference of squares formed as (sig_t - sig_s)(sig_t + sig_s) (VE_pbc.forward composed,
 *                 diffusion_helpers.py:43-47);
 *      lengths    l <- sqrt(abar_t / abar_s) l + sqrt(1 - abar_t / abar_s) z, abar_0 = 1 (VP_lattice.forward composed,
 *                 :156-163), then the cell by lattice_from_params into d_lattice;
 *      species    x <- argmax_c [log(Qbar_{t-s}[x, c] + eps) - log(-log(clip(u_c, eps, 1)))], Qbar_k = q_mats[k-1]
 *                 (D3PM.q_sample, d3pm.py:119-127: the rule and tie rule of the training forward), S uniforms per atom; the
 *                 absorbing fast path and the dense path give the same bits.
 *   3. held, not jumped: the lengths of a fixed cell (d_fixed_lengths), species given by d_const_types, known species of a
 *      condition (type_mask).  Known positions and known lengths ARE jumped (RePaint noises the whole state); the block's next
 *      update re-imposes them under conditioning rules 1-2.
 *   4. noise: the jump in front of pass r draws Philox (seed, t = block top, kind, element) with counter word3 = r: kind 6
 *      positions (normal, element 3 i + d), kind 7 lengths (normal, 3 b + d), kind 8 species (uniform, i S + c).  Inside pass r
 *      the predictor kinds 0-2 and the conditioning kinds 3-4 draw with word3 = 256 r, the corrector (kind 5) with 256 r + j.
 *      Pass 0 therefore draws exactly what a run without resampling draws, and R = 1 is arreau_sample_loop_corrected bit for
 *      bit, for any J.
 *   5. after a jump the device timestep is the block's top (in a respaced loop through the table's "one above" entry), in
 *      both loop forms and on the shape-general path; the next step's cell and per-crystal embedding are prepared for it.
 *   6. resampling combines with respacing, conditioning, corrector steps, fixed cells, constant species, ragged batches and graph
 *      replay (one captured step serves every pass and block; jumps are launched between replays).  No sample-quality claim is
 *      made: there is no trained checkpoint here.
 * The loop cuts blocks from the steps of ONE call: a run cut into calls at block boundaries is the run in one call. */
#define ARREAU_MAX_RESAMPLE_PASSES 64
typedef struct {
    int32_t passes;            /* R, 1..ARREAU_MAX_RESAMPLE_PASSES */
    int32_t jump_length;       /* J >= 1 */
    const int32_t* timesteps;  /* HOST copy of the schedule t_1..t_K behind `schedule` (NULL without one): block tops/bottoms */
    int32_t n_timesteps;
} arreau_resampling;

/* arreau_sample_loop_corrected with RePaint resampling (rules above; `resampling` is a host pointer, NULL or passes == 1 =
 * arreau_sample_loop_corrected).  Bad R or J, or (with a schedule and R > 1) a host copy that does not hold t_start followed by
 * at least n_steps - 1 further timesteps, return ARREAU_EINVAL before any work.  That the host copy matches the device table d_next
 * is not checked: the blocks follow the host copy, the device timestep the table.  R and J are part of what a cached hipGraph
 * was captured for. */
int arreau_sample_loop_resampled(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                 const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                                 uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                 void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                 const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                                 const arreau_corrector* corrector, const arreau_resampling* resampling, void* stream);

/* One jump (rule 2) from d_s[b] up to d_t[b] per crystal with the caller's noise d_z_frac[N,3], d_z_lengths[B,3] and
 * d_u_types[N,S], in place on (d_frac, d_types, d_lengths); d_lattice[B,3,3] receives the cells.  Held components (rule 3):
 * d_const_types, d_fixed_lengths (may be NULL) and the type mask of `cond` (host pointer, may be NULL).  A pair outside
 * 0 <= s < t <= T is clamped into it and sets ARREAU_STATUS_BAD_TIMESTEP.  For the loops with host-side noise and for parity
 * tests: fed arreau_philox_fill_word(seed, t, 6 / 7 / 8, r, ...), it is the loop's jump in front of pass r bit for bit. */
int arreau_resample_jump(const arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                         const int32_t* d_s, const int32_t* d_t, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                         const float* d_z_frac, const float* d_z_lengths, const float* d_u_types,
                         const int32_t* d_const_types, const float* d_fixed_lengths,
                         const arreau_sample_condition* cond, float* d_lattice, void* stream);

/* ---- lattice systems (tied cell lengths) --------------------------------------------------------------------------
 * A crystal of a chosen lattice system gets that system's angles from the host (d_angles, radians) and a tie code for its lengths:
 * 0 none (orthorhombic, monoclinic, triclinic), 1 a = b (tetragonal, hexagonal), 2 a = b = c (cubic, rhombohedral).  gamma is the
 * angle between a and b in lattice_from_params, so the tied pair is axes 0 and 1.  Angles are never diffused; lengths are, per
 * axis, so the tie is kept on the device at every step.  Per crystal b with code g, G = the tied set (empty, {0, 1} or {0, 1, 2});
 * axis 0 is the group's leader.
 *   1. update: the length update of a step (rule 2 of the respaced section; the stride-1 step as in arreau_reverse_step) is computed
 *      once for the axes in G with x_t = the leader's current length, x0 = the mean of the group's x0 (x0_i = pred_lengths_0_i *
 *      num_atoms, summed in axis order and divided by |G|) and z = the leader's draw (Philox kind 0, element 3 b + 0, or
 *      d_z_lattice[3 b + 0]), and written to every axis of G: tied axes are bitwise equal after every step, whatever the input.
 *      Axes outside G are updated as without a tie; d_len0 (the pooled network output in the loop) stays per axis.
 *   2. jump (RePaint resampling): the axes of G jump from the leader's length with the leader's draw (kind 7, element 3 b + 0, or
 *      d_z_lengths[3 b + 0]).
 *   3. fixed cell: the fixed lengths are re-imposed as without a tie (the caller ties them).
 *   4. a crystal whose lengths a condition knows (len_mask[b]) is not tied: the conditioning rule wins.
 *   5. a code outside 0..2 counts as 0 and sets ARREAU_STATUS_BAD_TIE.
 *   6. noise keys do not change: a crystal with code 0 draws, and computes, exactly what it does without a tie.
 * The initial lengths of a run are the caller's; tie them (lengths[b, G] = lengths[b, 0]) before the first call. */

/* arreau_sample_loop_resampled with the tie rules above.  d_length_tie[B] (device, int32) holds the code per crystal; NULL is
 * arreau_sample_loop_resampled bit for bit.  Both loop forms and the shape-general path apply it; the pointer is part of what a
 * cached hipGraph was captured for. */
int arreau_sample_loop_tied(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                            const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                            uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                            void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                            const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                            const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                            void* stream);

/* arreau_reverse_step_to with the tie rules above (the caller's noise; d_length_tie may be NULL = arreau_reverse_step_to). */
int arreau_reverse_step_tied(const arreau_model* model,
                             float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                             const int32_t* d_t, const int32_t* d_s, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                             const float* d_eps, const float* d_logits, const float* d_len0,
                             const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                             float* d_lattice, float lattice_clipmax, const int32_t* d_length_tie, void* stream);

/* arreau_resample_jump with the tie rules above (the caller's noise; d_length_tie may be NULL = arreau_resample_jump). */
int arreau_resample_jump_tied(const arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                              const int32_t* d_s, const int32_t* d_t, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                              const float* d_z_frac, const float* d_z_lengths, const float* d_u_types,
                              const int32_t* d_const_types, const float* d_fixed_lengths,
                              const arreau_sample_condition* cond, float* d_lattice, const int32_t* d_length_tie, void* stream);

/* ---- space-group symmetry (atoms tied in Wyckoff orbits) -------------------------------------------------------------
 * A space-group operation g acts on fractional coordinates as x -> R x + t (R integer, det +-1).  A constrained crystal's atoms
 * form orbits: each orbit O has a leader l (in the host's layout its lowest atom index), every atom j of O an operation k(j) with
 * g_k(j)(x_l) = x_j (mod 1), and l a stabilizer H_l (the operations that fix x_l mod 1).  At every step, per orbit:
 *   1. eps_bar = (1/|O|) sum_{j in O} R_k(j)^-1 eps_j, summed in the order of the orbit's member list (a displacement: no wrap).
 *   2. y = the VE reverse update of x_l (arreau_reverse_step's arithmetic, or the respaced step's) with eps_bar and the LEADER's
 *      draw (Philox kind 1, elements 3 l + d, or d_z_frac row l), without the wrap.  The members' draws are not used.
 *   3. x_l' = remainder_1( (1/|H_l|) sum_{h in H_l} (R_h y + t_h + n_h) ), n_h = rint(x_l - R_h x_l - t_h) (x_l the current,
 *      on-site position: the n_h are exact integers and the average is the affine projection onto the site, whatever the step);
 *      for |H_l| = 1 (a general position) x_l' = remainder_1(y).
 *   4. every other member: x_j' = remainder_1(R_k(j) x_l' + t_k(j)).
 *   5. species: the leader draws from the D3PM reverse with the orbit's MEAN logits (summed in member order, times 1/|O|) and
 *      its own uniforms (kind 2, elements l S + s, or d_u_types row l); every member takes the leader's new class.  Constant
 *      species (d_const_types) are re-imposed at the leader; the caller keeps them constant per orbit.
 *   6. lengths and angles: the lattice-system tie (d_length_tie, rules above), as without symmetry.
 *   7. an atom with leader -1 (an unconstrained crystal) computes exactly what it computes without the tables, bit for bit.
 * Tables (device pointers, all int32 unless stated): leader[N] (global atom index, -1 unconstrained), op[N] (k(j), a row of the
 * operation tables), orbit[N] (the orbit of a leader); orbit_ptr[n_orbits + 1] / orbit_atoms[n_orbit_atoms] (CSR: the members of
 * every orbit, leader included), stab_ptr[n_orbits + 1] / stab_ops[n_stab_ops] (CSR: H_l as operation rows); rot[n_ops, 9],
 * rot_inv[n_ops, 9], trans[n_ops, 3] (float32, row-major R, R^-1 and t).  Every index is checked before it is followed: a leader
 * outside -1..N-1, an orbit whose ranges, member atoms (all in the leader's crystal, all naming it as leader) or operation rows
 * are out of range, or a member whose leader does not lead itself, sets ARREAU_STATUS_BAD_SYMMETRY, and the atoms concerned are
 * updated without symmetry (the members of a rejected orbit are left as they were).  The initial state is the caller's: leaders
 * on their sites, members their images. */
typedef struct arreau_symmetry {
    const int32_t* leader;
    const int32_t* op;
    const int32_t* orbit;
    const int32_t* orbit_ptr;
    const int32_t* orbit_atoms;
    const int32_t* stab_ptr;
    const int32_t* stab_ops;
    const float* rot;
    const float* rot_inv;
    const float* trans;
    int32_t n_orbits, n_orbit_atoms, n_stab_ops, n_ops;
} arreau_symmetry;

/* arreau_sample_loop_tied with the symmetry rules above: the Philox loop (eager or graph replay, respaced schedules, fixed cells).
 * `symmetry` NULL is arreau_sample_loop_tied bit for bit.  With tables, `cond`, a corrector with steps > 0 and resampling with
 * passes > 1 are rejected (ARREAU_EINVAL).  The table pointers are part of what a cached hipGraph was captured for. */
int arreau_sample_loop_sym(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                           const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                           uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                           void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                           const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                           const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                           const arreau_symmetry* symmetry, void* stream);

/* arreau_reverse_step_tied with the symmetry rules above (the caller's noise; `symmetry` NULL = arreau_reverse_step_tied). */
int arreau_reverse_step_sym(const arreau_model* model,
                            float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                            const int32_t* d_t, const int32_t* d_s, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                            const float* d_eps, const float* d_logits, const float* d_len0,
                            const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                            float* d_lattice, float lattice_clipmax, const int32_t* d_length_tie, const arreau_symmetry* symmetry,
                            void* stream);

/* ---- DDIM-style sampling (an eta that scales the reverse step's noise) -----------------------------------------------
 * Song, Meng & Ermon 2021 ("Denoising Diffusion Implicit Models"): the same trained network and the same schedule, with a
 * parameter eta in [0, 1] that scales the noise a step injects -- eta = 1 the ancestral step of the sections above, eta = 0 a
 * deterministic map.  On a respaced schedule the ancestral step injects the full posterior noise of every jump; this is the
 * usual remedy.  The reference has no such option; the rules are the library's own.  The step that leaves t produces s (t - 1,
 * or the scheduled successor).  Float32 on the model's tables, evaluated in the order written:
 *   1. VE positions.  The predictor moves against eps with weight sig_t^2 - sig_s^2, so its x0 estimate is x_t - sig_t^2 eps.
 *      With r = sig_s / sig_t:  dir = sig_s sqrt((1 - eta^2) + eta^2 r^2),
 *      x_s = remainder(x_t - eps sig_t (sig_t - dir) + eta sig_s sqrt(1 - r^2) z, 1).
 *      eta = 1: rule 1 of the respaced section (sig_t (sig_t - dir) = sig_t^2 - sig_s^2, the same std).  eta = 0:
 *      x_s = remainder(x_t - eps sig_t (sig_t - sig_s), 1).
 *   2. VP lengths (x0 prediction).  beta as in rule 2 of the respaced section (betas[t] at stride 1, otherwise
 *      min(1 - abar_t / abar_s, lattice_clipmax)); den = 1 - abar_t, var = (1 - abar_s) beta / den,
 *      k = sqrt(max((1 - abar_s) (1 - eta^2 beta / den), 0) / den),
 *      l_s = (sqrt(abar_s) - k sqrt(abar_t)) x0 + k x_t + eta var z,  z = 0 for t <= 1.
 *      The direction term uses the true posterior variance; the noise keeps the ancestral step's amplitude (var, not its
 *      root).  eta = 1 is that step wherever beta is not clipped, up to the rounding of the float32 betas table against
 *      1 - abar_t / abar_s.  At (t, s) = (1, 0): l_s = x0.
 *   3. species: unchanged -- the D3PM step with its Gumbel draw.  eta = 0 makes positions and lengths a function of the
 *      state alone; species are deterministic only where they are held (d_const_types, a condition's known species) or at a
 *      species temperature of 0 (the section "Species control" below), which removes the draw.
 *   4. fixed cells, the known components of a condition (their rules and draws, kinds 3 and 4), corrector steps, resampling
 *      jumps and the lattice-system tie apply as without an eta.  Tied axes take the leader's x_t and draw and the group's
 *      mean x0, and stay bitwise equal.
 *   5. noise keys do not change: kinds 0 and 1 draw what they draw in the ancestral step.  The noise terms are added only
 *      when eta > 0: at eta = 0 the draws are not read (not generated, and a caller's d_z_lattice / d_z_frac may be NULL).
 *   6. eta not finite or outside [0, 1]: ARREAU_EINVAL before any work.  Not combined with space-group symmetry.
 * No claim on sample quality is made: there is no trained checkpoint here. */

/* arreau_sample_loop_tied with the eta step above in every step (d_length_tie and the other options may be NULL as there): both
 * loop forms, the shape-general path, graph replay, schedules, segments, conditions, correctors, resampling, fixed cells and
 * constant species.  eta is part of what a cached hipGraph was captured for: another eta is captured anew. */
int arreau_sample_loop_eta(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                           const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                           uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                           void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                           const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                           const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                           float eta, void* stream);

/* arreau_reverse_step_tied as the eta step (the caller's noise; d_length_tie may be NULL; at eta = 0 d_z_lattice and d_z_frac
 * may be NULL).  Fed arreau_philox_fill's draws it is the step of arreau_sample_loop_eta bit for bit. */
int arreau_reverse_step_eta(const arreau_model* model,
                            float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                            const int32_t* d_t, const int32_t* d_s, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                            const float* d_eps, const float* d_logits, const float* d_len0,
                            const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                            float* d_lattice, float lattice_clipmax, const int32_t* d_length_tie, float eta, void* stream);

/* ---- Second-order multistep sampling (the previous step's prediction extrapolates the move) ------------------------------
 * Lu et al. 2022 ("DPM-Solver++", the 2M rule): the eta = 0 step of the section above is a first-order solver of the
 * probability-flow ODE, so its error falls as 1/K on K steps.  Keeping the previous step's prediction and extrapolating with it
 * makes the move second order at the same one network evaluation per step.  The reference has no such option; the rules are the
 * library's own.  The step leaves level t for level s (t - 1, or the scheduled successor).  Float32 on the model's tables,
 * evaluated in the order written.
 *   History: the caller provides hist_eps[N,3] and hist_x0[B,3] (float32), hist_t_atom[N] and hist_t_len[B] (int32): per element
 *   the previous prediction, per atom / crystal the level p it was made at; a level of 0 means empty.  Every element's history and
 *   level are read and then overwritten by the thread that owns them: no cross-thread ordering and no second buffer, so one captured
 *   graph step serves every replay.  A history level p is usable when t < p <= T (only a usable p indexes a table).
 *   1. VE positions (noise prediction, log-sigma time).  e = sig_t eps;  r = logf(sig_p / sig_t) / logf(sig_t / sig_s).  The move is
 *      second order when p is usable, s >= 1 and 1/3 <= r <= 3 (float32 compares with 1.0f / 3.0f and 3.0f: a NaN or an infinite r
 *      fails).  Then d = e + (e - e_p) / (2 r) and x_s = remainder(x_t - (sig_t - sig_s) d, 1).  Otherwise the move is the eta = 0
 *      move of the DDIM section, bit for bit.  Then hist_eps <- e and the atom's level <- t.
 *   2. VP lengths (x0 prediction, log-SNR time).  x0 as in the step (pooled read-out times the atom count, or the tied group's
 *      mean);  lam_u = 0.5 (logf(abar_u) - logf(1 - abar_u));  r = (lam_t - lam_p) / (lam_s - lam_t);  k as in rule 2 of the DDIM
 *      section at eta = 0, k = sqrt(max(1 - abar_s, 0) / (1 - abar_t)).  Second order under the same three conditions:
 *      D = x0 + (x0 - x0_p) / (2 r) and l_s = (sqrt(abar_s) - k sqrt(abar_t)) D + k x_t.  Otherwise the eta = 0 length move, bit for
 *      bit (at s = 0: l = x0).  Then hist_x0 <- x0 (per axis, the value used) and the crystal's level <- t.  Tied axes take the
 *      leader's x_t and history value and the group's mean x0, and stay bitwise equal.  A fixed cell holds its lengths as without
 *      (its history is still kept).
 *   3. species: unchanged -- the D3PM step with its draw, kind 2, the same keys (a species temperature of 0, the section "Species
 *      control" below, removes it).  No position or length draw is read (a caller's
 *      d_z_lattice / d_z_frac may be NULL).
 *   4. the caller empties the levels (zero-fills hist_t_atom and hist_t_len) whenever the state changes outside a step.  A loop call
 *      never empties them, so a run cut into calls (frames, segments) is the run in one call.  The four pointers are part of what a
 *      cached hipGraph was captured for.
 *   5. combines with schedules, the lattice-system tie, fixed cells, constant species, any t_start, graph replay, both loop forms,
 *      the shape-general path and, on the step export, per-crystal timesteps.
 *   6. rejected with ARREAU_EINVAL before any work: a condition, corrector steps > 0, resampling passes > 1, a NULL struct or
 *      history pointer.  The exports take no symmetry tables and no eta.
 * The step-size guard: a second-order move across very unequal steps (the cosine schedule's first respaced step has r above 4 in
 * log-SNR units at T = 1000: 5.4 at K = 24) extrapolates further than the history supports; such a move is first order.
 * No claim on sample quality is made: there is no trained checkpoint here. */
typedef struct arreau_multistep {
    float* hist_eps;       /* [N,3] sig_p eps of the previous step */
    float* hist_x0;        /* [B,3] its predicted clean lengths */
    int32_t* hist_t_atom;  /* [N]   the level the atom's hist_eps was made at (0: empty) */
    int32_t* hist_t_len;   /* [B]   the level the crystal's hist_x0 was made at (0: empty) */
} arreau_multistep;

/* arreau_sample_loop_tied with the multistep step above in every step (`multistep` is a host pointer to the struct of device
 * pointers; d_length_tie, schedule and the fixed / constant arrays may be NULL as there; condition, corrector and resampling must be
 * NULL or empty, rule 6): both loop forms, the shape-general path and graph replay. */
int arreau_sample_loop_multistep(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                 const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                                 uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                 void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                 const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                                 const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                                 const arreau_multistep* multistep, void* stream);

/* arreau_reverse_step_eta at eta = 0 as the multistep step (the caller's uniforms for the species; d_z_lattice and d_z_frac are not
 * read and may be NULL; d_length_tie may be NULL).  With empty levels it is arreau_reverse_step_eta at eta = 0 bit for bit; fed
 * arreau_philox_fill's draws it is the step of arreau_sample_loop_multistep bit for bit. */
int arreau_reverse_step_multistep(const arreau_model* model,
                                  float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                  const int32_t* d_t, const int32_t* d_s, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                                  const float* d_eps, const float* d_logits, const float* d_len0,
                                  const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                                  float* d_lattice, float lattice_clipmax, const int32_t* d_length_tie,
                                  const arreau_multistep* multistep, void* stream);

/* ---- Species control (per-crystal element sets, a species temperature) -------------------------------------------------
 * The D3PM species step restricted to a set of classes per crystal ("generate in a chemical system") and its Gumbel term scaled
 * by a temperature that can be turned down to 0, which makes the eta = 0 and multistep samplers functions of the initial state in
 * all three components.  The reference has no such option; the rules are the library's own.  They touch the species half of the
 * step alone: positions, lengths and the cell are those of the step without the option, bit for bit.
 *   Inputs: per crystal b an admission row allow[b] of four uint32 words -- class c is bit c & 31 of word c >> 5 (S <= 124; bits at
 *   or above S are ignored) -- and one scalar temperature tau >= 0.
 *   The admitted set: the step leaves level t for level s.  E(b, t) is every ordinary class c < S - 1 whose bit is set, plus the
 *   mask class S - 1: when t > 1 always (the chain passes through it), when t == 1 only if its own bit is set.
 *   Float32, in this order:
 *   1. x0 logits: l_c stays for c in E and becomes -inf otherwise, so the softmax gives an excluded class an exact 0 and its
 *      maximum and sum run over what is left.
 *   2. posterior: computed as without the option (unit stride, respaced, absorbing shortcut, dense chain) from that softmax.
 *   3. posterior logits: post_c stays for c in E and becomes -inf otherwise (at t == 1 post is the masked logits of 1).  This makes
 *      the exclusion exact: without it an excluded class keeps 2 log(1e-6) and can win a Gumbel draw.
 *   4. value_c = post_c + (tau scale_t) g_c, scale_t = 1 for t != 1 and 0.2 at t == 1, g_c = -log(-log(clip(u_c, 1e-6, 1))) from the
 *      keys of the step without the option (kind 2, element i S + c).  At tau == 0 nothing is added: the uniforms are neither read
 *      nor generated and d_u_types may be NULL.
 *   5. arg-max over the admitted classes only, lowest index first on ties.  Only a value above -inf competes (a NaN does not); if
 *      no admitted class has one (non-finite logits) the result is the lowest admitted class.  So after a step a sampled atom of
 *      crystal b holds a class of E(b, t), unconditionally.  (A row that admits nothing at t == 1 -- the callers reject a row
 *      without an ordinary class -- gives the mask class.)
 *   6. held species (d_const_types, a condition's known species) are imposed after the draw, as without the option; they are not
 *      checked on the device.
 *   7. an atom that enters the step outside its set (a given initial state, a RePaint jump on a non-absorbing chain) leaves it inside.
 *   8. a symmetric orbit draws one class by the same steps: the orbit's mean logits, the leader's draw, its crystal's row.
 *   9. a row of all ones (or a NULL table) with tau == 1 is the step without the option bit for bit: no value is masked, and
 *      1.0f * scale is scale.
 * A temperature that is negative or not finite is rejected with ARREAU_EINVAL before any work.  The table pointer and the
 * temperature are part of what a cached hipGraph was captured for.  No claim on sample quality is made. */
typedef struct arreau_species_control {
    const uint32_t* d_allow; /* [B,4] admission rows (device); NULL: every class for every crystal */
    float temperature;       /* tau >= 0: the scale of the Gumbel term (1: the step's own; 0: no draw) */
} arreau_species_control;

/* Whichever loop of arreau_sample_loop_sym / _eta / _multistep the options name, under species control: `symmetry` and `multistep`
 * as there (NULL: without), `eta` a host pointer to the eta of arreau_sample_loop_eta (NULL: the ancestral step, whose kernels
 * differ from the eta = 1 kernels in rounding), `species` a host pointer to the struct above (required).  Every other argument as
 * in arreau_sample_loop_tied: schedule, condition, corrector, resampling, tie, fixed cell, constant species, t_start, segments, graph
 * replay, both loop forms and the shape-general path.  What those loops do not combine stays rejected with ARREAU_EINVAL: symmetry
 * with an eta, a condition, corrector steps or resampling; multistep with a condition, corrector steps, resampling, symmetry or an
 * eta other than 0. */
int arreau_sample_loop_species(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                               const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                               uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                               void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                               const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                               const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                               const arreau_symmetry* symmetry, const float* eta, const arreau_multistep* multistep,
                               const arreau_species_control* species, void* stream);

/* The step of arreau_reverse_step_sym / _eta / _multistep (whichever `symmetry`, `eta`, `multistep` name; all NULL:
 * arreau_reverse_step_tied) under species control, on the caller's noise and per-crystal d_t / d_s.  d_u_types may be NULL at a
 * temperature of 0; d_z_lattice and d_z_frac at eta = 0 or with multistep.  Fed arreau_philox_fill's draws it is the step of
 * arreau_sample_loop_species bit for bit. */
int arreau_reverse_step_species(const arreau_model* model,
                                float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                const int32_t* d_t, const int32_t* d_s, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                                const float* d_eps, const float* d_logits, const float* d_len0,
                                const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                                float* d_lattice, float lattice_clipmax, const int32_t* d_length_tie,
                                const arreau_symmetry* symmetry, const float* eta, const arreau_multistep* multistep,
                                const arreau_species_control* species, void* stream);

/* ---- Starting the sampler from given crystals (forward noising, DDIM inversion) ---------------------------------------
 * Every loop export takes t_start, so a run may enter the schedule anywhere; what follows produces the states to enter with.
 * Level convention: "a state at level t" is one whose first network evaluation is at timestep t.  The prior draw of a full
 * run is a state at level T-1.  The reference has neither operation; the rules are the library's own.
 *   1. forward noising to level t (arreau_noise_state, 1 <= t <= T): the jump (s, t) = (0, t) of the RePaint section, rule 2,
 *      computed by the same kernel:
 *      positions  x <- remainder(x + sqrt((sig_t - sig_0)(sig_t + sig_0)) z, 1);
 *      lengths    l <- sqrt(abar_t) l + sqrt(1 - abar_t) z, then the cell into d_lattice;
 *      species    q_sample with q_mats[t-1] and that kernel's Gumbel arg-max.
 *      Held as there (rule 3): species given by d_const_types, the lengths of d_fixed_lengths; d_length_tie ties the lengths
 *      as in the lattice-systems section (rule 2 there).  The draws are Philox (seed, t, kind 6 / 7 / 8, element, word3 = 0).
 *      A resampled loop draws these kinds only with pass words r >= 1 (its pass 0 starts without a jump), so the keys with
 *      word3 = 0 are free and no loop draw is ever repeated.  Fed arreau_philox_fill_word(seed, t, 6 / 7 / 8, 0, ...),
 *      arreau_resample_jump with d_s = 0, d_t = t reproduces it bit for bit.
 *   2. inversion step from level s up to level t (1 <= s < t <= T): the inverse of the eta = 0 step of the DDIM section
 *      (Song, Meng & Ermon 2021, section 4.3), with the network evaluated on the state at s with timestep s.  Float32 on the
 *      model's tables, evaluated in the order written:
 *      positions  x_t = remainder(x_s + eps sig_s (sig_t - sig_s), 1).  The predictor's x0 estimate is x_s - sig_s^2 eps; the
 *                 unit-variance direction sig_s eps is kept and rescaled to sig_t.
 *      lengths    x0 = the predicted clean lengths exactly as the eta move takes them (pooled read-out times the atom count);
 *                 rho = sqrt((1 - abar_t) / (1 - abar_s)),  l_t = sqrt(abar_t) x0 + rho (l_s - sqrt(abar_s) x0).
 *                 No beta, no clip and no draw enters.  With d_fixed_lengths the lengths are held.
 *      species    never written: the species the network sees at every level are the caller's (the situation of
 *                 d_const_types in a sampling loop).  D3PM has no inverse.
 *   3. a pair outside 1 <= s < t <= T is clamped into it (s into 1..T-1, then t into s+1..T) and sets
 *      ARREAU_STATUS_BAD_TIMESTEP, as the descending step does for its target; crystals with valid pairs in the same batch are
 *      not affected.
 *   4. no noise is read and no seed enters.  Lattice-system ties, symmetry tables and conditions are not part of these rules:
 *      the exports below do not take them.
 *   5. identity: let x_t, l_t be the step's output for (eps, x0).  The eta = 0 step t -> s fed eps sig_s / sig_t and the same x0
 *      returns x_s, l_s up to rounding: x_t - (eps sig_s / sig_t) sig_t (sig_t - sig_s) = x_s, and with k = 1 / rho,
 *      (sqrt(abar_s) - k sqrt(abar_t)) x0 + k l_t = l_s.  rho reaches 63 at T = 100 and 579 at T = 1000 from level 1: the
 *      rounding of the length move scales with rho (|l_s| + |x0|), not with |l_t|.
 * The final step 1 -> 0 of a sampling run has no inverse here: a crystal is taken as the state at the lowest level visited.
 * No claim on reconstruction quality is made: there is no trained checkpoint here. */

/* Rule 1 in place on (d_frac, d_types, d_lengths); d_lattice[B,3,3] receives the cells.  d_const_types, d_fixed_lengths and
 * d_length_tie may be NULL.  t outside 1..T: ARREAU_EINVAL before any work. */
int arreau_noise_state(const arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                       const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t, uint64_t seed,
                       const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                       const int32_t* d_length_tie, void* stream);

/* One inversion step (rules 2-3) per crystal from level d_s[b] up to d_t[b] on the caller's network outputs d_eps[N,3] and
 * d_len0[B,3], in place on (d_frac, d_lengths); d_lattice receives the cells.  d_types is not read or written;
 * d_fixed_lengths may be NULL.  For tests and host-driven loops: fed arreau_predict_scores' outputs at d_s it is the step of
 * arreau_invert_loop bit for bit. */
int arreau_invert_step(const arreau_model* model, float* d_frac, const int32_t* d_types, float* d_lengths,
                       const float* d_angles, const int32_t* d_s, const int32_t* d_t, const int32_t* d_crystal_offsets,
                       int32_t B, int32_t N, const float* d_eps, const float* d_len0, const float* d_fixed_lengths,
                       float* d_lattice, void* stream);

/* n_steps inversion steps in one call: the state (a state at level t_first) climbs t_first = u_0 < u_1 < ... < u_n along the
 * device table d_up (int32 [T+1]): d_up[u_i] = u_{i+1}, and d_up[t_first - 1] = t_first -- the "one below" entry the loop's
 * first launch advances from, mirroring the "one above" entry of a descending schedule; also at stride 1 the table is the
 * caller's.  A climb cut into calls needs that entry for the first level of every call.  One network evaluation per step, at the level left.  Both loop forms, the shape-general path and graph replay
 * (use_graph, from 3 steps) as in arreau_sample_loop; that the loop climbs is part of what a cached hipGraph was captured for,
 * so a sampling graph of the same buffers is never replayed for it, or the other way round.  t_first < 1 or
 * t_first + n_steps > T: ARREAU_EINVAL before any work; a table entry that does not climb is clamped and flagged (rule 3). */
int arreau_invert_loop(arreau_model* model, float* d_frac, const int32_t* d_types, float* d_lengths, const float* d_angles,
                       const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_first, int32_t n_steps,
                       const int32_t* d_up, const float* d_fixed_lengths, float* d_lattice, void* d_workspace,
                       size_t workspace_bytes, int32_t use_graph, void* stream);

/* The sampler's in-kernel noise written out: d_out[i] = draw (seed, timestep, kind, element i) -- standard normal for
 * kind 0 (z_lattice), 1 (z_frac), 3 (known positions) and 4 (known lengths), uniform [0,1) for kind 2 (u_types); d_raw[4 i .. 4 i + 3] (may be NULL) = the raw
 * Philox4x32-10 words of counter (i, timestep, kind, 0), key = seed.  Feeding these arrays to arreau_reverse_step
 * reproduces arreau_sample_loop's update bit for bit.  Kinds above 4 are rejected (arreau_philox_fill_word). */
int arreau_philox_fill(uint64_t seed, int32_t timestep, int32_t kind, int64_t n, float* d_out, uint32_t* d_raw,
                       void* stream);
/* arreau_philox_fill with the counter's fourth word given: counter (i, timestep, kind, word3).  Kinds 0..8; kind 5 (the
 * corrector's Langevin noise, standard normal) with word3 = j is what the loop's j-th correction at `timestep` draws; kinds 6, 7
 * (standard normal) and 8 (uniform [0,1)) with word3 = r are the draws of a resampled loop's jump in front of pass r. */
int arreau_philox_fill_word(uint64_t seed, int32_t timestep, int32_t kind, uint32_t word3, int64_t n, float* d_out,
                            uint32_t* d_raw, void* stream);

/* ---- keyed sampling (a crystal is a function of (seed, key), not of its batch) -------------------------------------------
 * The loops above key a draw by (seed, timestep, kind, GLOBAL element, word3): element 3 i + d with i the atom's index in the
 * batch, so a crystal's draws depend on where it sits in the batch.  The keyed loop gives every crystal b a stream of its own,
 * derived from (seed, key_b), and counts elements inside the crystal.  The reference has no such mode; the rules are the
 * library's own (restated in arreau_amd/diffusion/keyed.py).
 *   1. stream seed: for a key 0 <= key < 2^63,
 *          s_b = stream_seed(seed, key_b) = w0 | w1 << 32,
 *      w0, w1 words 0 and 1 of philox4x32_10(counter = (key lo, key hi, 0x4B455953, 0), key = (seed lo, seed hi)).  The caller
 *      computes it on the host in exact integer arithmetic and hands the library the table d_crystal_seeds [B] (uint64, device).
 *      (seed 5, key 1) and (seed 6, key 0) are different streams, unlike seed + key.
 *   2. draws of the loop: wherever the Philox loop draws (seed, t, kind, element, word3), the keyed loop draws
 *      (s_b, t, kind, element', word3), b the crystal of the element and element' counted within it:
 *          3 a + d   positions (kinds 1, 3, 5, 6),   d   lengths (kinds 0, 4, 7; a tied axis the leader's d = 0),
 *          a S + c   species (kinds 2, 8),           a the atom's index in its crystal.
 *      Kinds and word3 keep their meaning (corrector iteration, 256 r in pass r, r for the jump).  Every draw site: the position and
 *      species halves of the step (plain, eta, multistep, species control), the length components (plain and tied), the symmetric
 *      step's leaders, the known components of a condition in the step and in the initial state, the corrector, the jump, the
 *      forward noising of arreau_noise_state.
 *   3. initial state: kinds 13 (normal [3], the lengths), 14 (normal [n,3], the positions) and 15 (uniform, the j-th uniform the
 *      crystal's angle draw consumes), at counter timestep 0, word3 0, under s_b.  The host applies its formulas to them exactly
 *      as to its generators' values.  arreau_philox_fill_crystals writes them out.
 *   4. hence the state of crystal b after any number of steps is a function of (model, options, seed, key_b, its atom count, its
 *      own inputs).  Within one score arithmetic it is bitwise independent of the other crystals of the batch, of its index in it
 *      and of how the run is cut into calls.
 *   5. limits.  (a) The score network picks its kernels by the size of the launch: batches on different sides of the basis-form
 *      threshold, or run with and without ARREAU_CROSS_FP8, agree to the bound of the network's batch-independence test, not
 *      bitwise.  (b) The re-run of a batch after an fp16x3 overflow is a decision about the whole batch: a crystal that shares a
 *      batch with an overflowing one is re-run with it on other kernels.
 * Without the table every kernel draws exactly what it drew before the table existed.
 *
 * arreau_sample_loop_keyed: arreau_sample_loop_species plus d_crystal_seeds; NULL is arreau_sample_loop_species bit for bit.  Every
 * combination that loop accepts, both loop forms, the shape-general path, eager and graph replay (the table pointer is part of
 * what a cached graph was captured for); what it rejects stays rejected. */
int arreau_sample_loop_keyed(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                             const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                             uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                             void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                             const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                             const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                             const arreau_symmetry* symmetry, const float* eta, const arreau_multistep* multistep,
                             const arreau_species_control* species, const uint64_t* d_crystal_seeds, void* stream);
/* arreau_noise_state / arreau_condition_initial_state with the table (the latter also takes the crystal offsets, which it needs
 * to count within a crystal); a NULL table is the export without it. */
int arreau_noise_state_keyed(const arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                             const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t, uint64_t seed,
                             const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                             const int32_t* d_length_tie, const uint64_t* d_crystal_seeds, void* stream);
int arreau_condition_initial_state_keyed(const arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths,
                                         const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, uint64_t seed,
                                         const arreau_sample_condition* cond, const uint64_t* d_crystal_seeds, void* stream);
/* The keyed draws written out in batch layout: exactly one of per_atom_width / per_crystal_width is positive.  per_atom_width = w:
 * d_out [N,w], row of atom a of crystal b = the draws (d_seeds[b], timestep, kind, a w + c, word3), c < w (w = 3 for positions,
 * S for species).  per_crystal_width = w: d_out [B,w], row b = the draws of elements 0..w-1.  Normal for kinds 0, 1, 3..7, 13, 14,
 * uniform [0,1) for kinds 2, 8, 15; kinds 9..12 are rejected.  d_raw (may be NULL; d_out may be NULL with it): the four raw words
 * per element.  Fed to arreau_reverse_step*, arreau_corrector_step and arreau_resample_jump*, these arrays reproduce the keyed
 * loop bit for bit (a tied axis reads the leader's entry of the [B,3] array, as in the loop). */
int arreau_philox_fill_crystals(const uint64_t* d_seeds, const int32_t* d_crystal_offsets, int32_t B, int32_t timestep,
                                int32_t kind, uint32_t word3, int32_t per_atom_width, int32_t per_crystal_width, float* d_out,
                                uint32_t* d_raw, void* stream);

/* ---- contact guidance (steer the sampler away from short contacts) -------------------------------------------------------
 * Training-free, energy-based guidance of the positions: every network evaluation of a step is followed by one launch that adds
 * the gradient of a contact penalty to the predicted eps, so that what the step predicts as the clean structure has its short
 * contacts pushed apart.  The reference has no such option; the rules are the library's own (restated in float64 in
 * arreau_amd/diffusion/contact_guidance.py).  Parameters: min_distance d0 in A (finite, > 0), weight w (finite, >= 0), max_shells
 * in 1..ARREAU_SCREEN_MAX_SHELLS (the screen's cap, with the screen's meaning).  For crystal b: the wrapped fractional positions
 * (w = f - floor(f), a result of 1 becomes 0), the Cartesian positions r = (w_0 L_0 + w_1 L_1) + w_2 L_2 and the cell rows a, b, c
 * = L_0, L_1, L_2 that the step's network evaluation saw (the screen's rules 4 and 5).  Float32, one rounding per operation, in the
 * order written, never contracted.
 *   1. contacts: every (i, j, n) with j != i and n = (n_1, n_2, n_3) in the screen's image range for the radius d0
 *      (q_k = d0 / spacing of the planes across axis k, N_k = max(1, ceil(q_k)), |n_k| <= N_k), s = (n_1 L_0 + n_2 L_1) + n_3 L_2,
 *      disp = (r_j + s) - r_i, d2 = (dx dx + dy dy) + dz dz, d = sqrt(d2), for which 0 < d2 < (float)((double)d0 * d0) -- the
 *      comparison of squares the screen's CLOSE count makes, that is 0 < d < d0.  Self images (j = i) are left out: they exert no
 *      force on positions.  A pair with d2 == 0 is skipped and sets OVERLAP.
 *   2. penalty: U_b = 1/2 sum_i sum_(j,n) 1/2 (d0 - d)^2, in A^2 (every unordered contact once).
 *   3. Cartesian gradient on atom i: D_i = sum_(j,n) ((d0 - d) / d) disp.  It points towards the neighbours (dU/dr_i = D_i).
 *   4. metric-preconditioned fractional gradient: g_i = D_i L^-1, g_i,k = (D_i . c_k) / V with c_0 = b x c, c_1 = c x a,
 *      c_2 = a x b and V = a . (b x c), signed.  A fractional move -w g_i is then the Cartesian move -w D_i, whatever the cell.
 *   5. guided prediction: eps'_i = eps_i + (w / sigma_t^2) g_i, sigma = ve_sigmas, t the crystal's timestep (clamped into 1..T and
 *      flagged in the model's status word like every step).  Every consumer of the step's eps reads eps' in place of eps: the
 *      predictor in all its instances (ancestral, respaced, eta, multistep and its history, tied, symmetric, species control,
 *      keyed) and the corrector.  Reading: the predictor's clean-position estimate x - sigma_t^2 eps becomes
 *      x - sigma_t^2 eps - w g: the predicted clean structure is moved one descent step of size w down U.  For an isolated
 *      contact each atom moves w (d0 - d) away from the other, so w = 0.5 resolves it exactly.  Under the predictor's reading of
 *      eps as -score this is guidance by p_t(y | x) ~ exp(-w U / sigma_t^2).  The corrector reads -eps' / sigma_t^2 as its score (its rule
 *      1) and normalises its step by |eps'| (its rule 2): guidance turns a corrector move, it does not lengthen it.
 *   6. order within a step: after every network evaluation of the step, a corrector's re-evaluations included, and before
 *      whatever reads that evaluation's eps (evaluate, guide, correct, evaluate, guide, predict).
 *   7. atoms with known positions under a condition get a guided eps like any other atom, which the conditioning rule then
 *      overwrites; they still push their neighbours.
 *   8. flags (per crystal, int32): NONFINITE a cell entry or coordinate is not finite; CELL the volume is not finite or an axis
 *      needs more than max_shells images (not (q_k <= max_shells)); EMPTY n = 0; OVERLAP a pair with d2 == 0 was skipped.
 *      NONFINITE stands alone (nothing else is computed); CELL and EMPTY may be set together.  A crystal flagged NONFINITE, CELL or EMPTY keeps its eps bit for bit, with U = 0 and contacts = 0.
 *   9. weight == 0 or a NULL struct is the loop without the option: no launch is added, bit identical.  An inversion loop
 *      rejects the option, bad parameters are rejected, with ARREAU_EINVAL before any work.
 *  10. the three parameters and the three diagnostic pointers are part of what a cached hipGraph was captured for.
 * Summation order (fixed, so eager runs, graph replay and a crystal's place in the batch give the same bits): one workgroup of four
 * waves per crystal, wave v owns atoms v, v + 4, ...; for atom i lane l adds the contacts it meets at e = l, l + 64, ... of the
 * range e = j M + m (j ascending, images m in lexicographic order), the 64 partial sums are folded by the butterfly
 * xor 32, 16, ..., 1, a wave adds the energies of its atoms in ascending i, and the four waves are added in wave order.  No
 * float atomics.  energy = 0.25 * that sum; contacts = the ordered contacts / 2.
 * What this is not: the penalty acts on positions only -- no cell-strain term (lengths and angles are not guided), no radii or
 * species dependence (one d0 for every pair), no weight schedule other than 1 / sigma_t^2, no claim on sample quality. */
#define ARREAU_GUIDE_NONFINITE 1
#define ARREAU_GUIDE_CELL 2
#define ARREAU_GUIDE_EMPTY 4
#define ARREAU_GUIDE_OVERLAP 8
typedef struct arreau_contact_guidance {
    float min_distance;  /* d0 in A: finite, > 0 */
    float weight;        /* w: finite, >= 0; 0 is the loop without the option */
    int32_t max_shells;  /* 1..ARREAU_SCREEN_MAX_SHELLS */
    float* d_energy;     /* [B] U_b of the last evaluation (device), or NULL */
    int32_t* d_contacts; /* [B] its unordered contacts (device), or NULL */
    int32_t* d_flags;    /* [B] ARREAU_GUIDE_* (device), or NULL */
} arreau_contact_guidance;

/* arreau_sample_loop_keyed plus `guidance`, a HOST pointer to the struct above; NULL (or weight == 0) is that loop bit for bit.
 * Every combination that loop accepts, both loop forms, the shape-general path, eager and graph replay. */
int arreau_sample_loop_guided(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                              const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                              uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                              void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                              const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                              const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                              const arreau_symmetry* symmetry, const float* eta, const arreau_multistep* multistep,
                              const arreau_species_control* species, const uint64_t* d_crystal_seeds,
                              const arreau_contact_guidance* guidance, void* stream);
/* Rules 1-5 and 8 on the caller's arrays: d_eps [N,3] in place, at the per-crystal timesteps d_t [B], with the cells d_lattice
 * [B,3,3] (rows a, b, c).  `guidance` is required; weight == 0 launches too (eps + 0 g, and the diagnostics).  For tests and
 * host-driven loops: between arreau_predict_scores and a step export it is the guided loop's step bit for bit. */
int arreau_contact_guidance_step(const arreau_model* model, const float* d_frac, const float* d_lattice, const int32_t* d_t,
                                 const int32_t* d_crystal_offsets, int32_t B, int32_t N, float* d_eps /* in place */,
                                 const arreau_contact_guidance* guidance, void* stream);

/* ---- XRD guidance (steer the sampler towards a target powder pattern) -----------------------------------------------------
 * Training-free guidance of the positions by an observable: every network evaluation of a step is followed by one launch that
 * adds the gradient of the distance between the crystal's powder pattern and a target pattern to the predicted eps, so that the
 * pattern of what the step predicts as the clean structure approaches the target.  The use is structure solution from a powder
 * pattern: the cell (fixed, conditioned or of a lattice system) and the composition are given, where the atoms sit is left to
 * the sampler.  The reference has no such option; the rules are the library's own (restated in float64 in
 * arreau_amd/diffusion/xrd_guidance.py).  Parameters: `params`, an arreau_xrd_params with the xrd launch's meaning and
 * validation; weight w in A^2 (finite, >= 0); d_target [B, n_points] float32, the target pattern of every crystal on that grid;
 * the amplitudes as d_class_weights [S] float32, one per species class -- the amplitude of an atom is that of its current class
 * (d_types as the evaluation saw them; a class outside 0..S-1 weighs 0), so a class of weight 0, such as the mask class, does not
 * scatter and gets no push -- or, for the step export only, as d_atom_weights [N]; exactly one of the two.  Per crystal, on the
 * wrapped positions and the cell that the step's network evaluation saw:
 *   1. PATTERN: P is the pattern of arreau_crystal_xrd for these atoms and amplitudes, its rules 2-7, bit for bit (the two
 *      kernels run one reflection walk, csrc/xrd_dev.h).
 *   2. DISTANCE: dist = (1 - P.Q / (|P| |Q|)) / 2, Q the target row.  The three sums P.Q, P.P, Q.Q are float64 of the float32
 *      values in a fixed order: thread t adds the points p = t (mod 256) in ascending order, then the butterfly xor 32, 16, ..., 1
 *      within a wave, then the four waves in wave order.
 *   3. DERIVATIVE WITH RESPECT TO THE PATTERN: u(p) = -(1/2) (Q(p) / (|P||Q|) - (P.Q) P(p) / (|P|^3 |Q|)), float64, rounded to
 *      float32 (it replaces P in LDS).
 *   4. PER KEPT REFLECTION (the forward walk's half space, cuts and box order; Re F, Im F, 2 theta and the window are formed
 *      again by the same code, the same bits): c = sum over the window's grid points, in ascending p, of u(p) G(p), with G(p) =
 *      expf(-0.5 z^2) and the 6 sigma test of rule 7 of the xrd section, the products and the sum float64; kappa = 2 DW LP /
 *      V^2 / (sigma sqrt(2 pi)), the factor that multiplies |F|^2 in rule 6 there (Friedel's 2 inside), float64.
 *   5. CARTESIAN GRADIENT on atom a: D_a = -4 pi w_a sum over the kept reflections of kappa c (Re F sin phi_a - Im F cos phi_a)
 *      G_hkl, with (sin, cos) = sincospi(2 r_a) of the reflection's reduced float32 phase r_a at atom a (rule 5 of the xrd
 *      section) and G_hkl = (h b_1 + k b_2) + l b_3 the float64 reciprocal vector of the walk.  Everything after the sincospi is
 *      float64.  D_a = d dist / d r_a: the peak positions depend on the cell alone.
 *   6. FRACTIONAL GRADIENT AND GUIDED EPS: g_a = D_a L^-1, g_a,k = (D_a . b_k) (contact guidance's rule 4; the b_k of rule 2 of
 *      the xrd section), rounded to float32; eps'_a = eps_a + (w / sigma_t^2) g_a in float32, coefficient and timestep clamp as
 *      in contact guidance's rule 5, and every consumer of the step's eps reads eps'.  The predictor's clean-position estimate
 *      moves -w g: one descent step of size w on the distance.
 *   7. ORDER WITHIN A STEP: evaluate, contact guidance if given, XRD guidance, then the corrector or the predictor; after a
 *      corrector's re-evaluations too.
 *   8. FLAGS (int32 per crystal, one at most, in this order): NONFINITE (an amplitude counts), CELL, EMPTY, RANGE with the xrd
 *      launch's meaning and values; LARGE more than 256 atoms (the per-atom accumulators are LDS-resident: a stated limit);
 *      NO_TARGET the target row has an entry that is not finite or is negative, or is all zero; DARK |P|^2 is zero or not
 *      finite: nothing scatters in range.  A flagged crystal keeps its eps bit for bit; its distance is NaN, its reflections 0,
 *      its g (d_gradient) 0.
 *   9. weight == 0 or a NULL struct is the loop without the option: no launch is added, bit identical.  An inversion loop
 *      rejects the option; bad parameters, a NULL target, none or both of the amplitude arrays, and atom weights in a loop are
 *      ARREAU_EINVAL before any work.  The parameters and the pointers are part of what a cached hipGraph was captured for.
 * Summation order (fixed, so eager runs, graph replay and a crystal's place in the batch give the same bits): one workgroup of four
 * waves per crystal.  The second walk runs in rounds of 256 box entries; a round's kept reflections are compacted in thread order
 * into a list, as the forward walk compacts them.  Wave v owns atoms v, v + 4, ...; for atom a lane l adds the list entries l,
 * l + 64, ... in ascending order, the 64 partial sums are folded by the butterfly xor 32, 16, ..., 1, and the round's sum is added
 * to the atom's accumulator, rounds in ascending order.  No float atomics.
 * Diagnostics (device, each may be NULL, of the last evaluation): d_distance [B] float32 of rule 2's value, d_reflections [B]
 * (2 * the kept, the xrd launch's n_reflections), d_flags [B].
 * What this is not: positions only -- a wrong cell cannot be repaired (fix the cell); no guidance of species; no intensity
 * scale or background fit (the cosine distance is scale free); no weight schedule other than 1 / sigma_t^2; no claim on sample
 * quality. */
#define ARREAU_XGUIDE_NO_TARGET 16
#define ARREAU_XGUIDE_DARK 32
#define ARREAU_XGUIDE_LARGE 64
typedef struct arreau_xrd_guidance {
    arreau_xrd_params params;     /* the grid, wavelength, fwhm, b_iso, max_index */
    float weight;                 /* w in A^2: finite, >= 0; 0 is the loop without the option */
    const float* d_target;        /* [B, n_points] (device) */
    const float* d_class_weights; /* [S] (device), or NULL with d_atom_weights */
    const float* d_atom_weights;  /* [N] (device), arreau_xrd_guidance_step only, or NULL */
    float* d_distance;            /* [B] (device), or NULL */
    int32_t* d_reflections;       /* [B] (device), or NULL */
    int32_t* d_flags;             /* [B] ARREAU_XRD_* | ARREAU_XGUIDE_* (device), or NULL */
} arreau_xrd_guidance;

/* arreau_sample_loop_guided plus `xrd_guidance`, a HOST pointer to the struct above; NULL (or weight == 0) is that loop bit for
 * bit.  Every combination that loop accepts, both loop forms, the shape-general path, eager and graph replay. */
int arreau_sample_loop_xrd_guided(arreau_model* model, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                  const int32_t* d_crystal_offsets, int32_t B, int32_t N, int32_t t_start, int32_t n_steps,
                                  uint64_t seed, const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                  void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                  const arreau_sample_condition* cond, const arreau_sample_schedule* schedule,
                                  const arreau_corrector* corrector, const arreau_resampling* resampling, const int32_t* d_length_tie,
                                  const arreau_symmetry* symmetry, const float* eta, const arreau_multistep* multistep,
                                  const arreau_species_control* species, const uint64_t* d_crystal_seeds,
                                  const arreau_contact_guidance* guidance, const arreau_xrd_guidance* xrd_guidance, void* stream);
/* Rules 1-6 and 8 on the caller's arrays: d_eps [N,3] in place, at the per-crystal timesteps d_t [B], with the cells d_lattice
 * [B,3,3] (rows a, b, c) and the classes d_types [N] (may be NULL with d_atom_weights).  d_gradient [N,3] (may be NULL) receives
 * g itself.  `guidance` is required; weight == 0 launches too (eps + 0 g, g and the diagnostics).  For tests and host-driven
 * loops: between arreau_predict_scores (and arreau_contact_guidance_step) and a step export it is the guided loop's step bit
 * for bit. */
int arreau_xrd_guidance_step(const arreau_model* model, const float* d_frac, const int32_t* d_types, const float* d_lattice,
                             const int32_t* d_t, const int32_t* d_crystal_offsets, int32_t B, int32_t N, float* d_eps /* in place */,
                             const arreau_xrd_guidance* guidance, float* d_gradient, void* stream);

/* ---- score-matching training loss, forward part (BASELINE config 5) ------------------------------------------ */

/* The forward-noising half of DiffusionLoss.__call__ (diffusion/diffusion_loss.py:222-234), random draws supplied by
 * the caller in the reference's order (z_frac: randn_like(frac_x0), diffusion_helpers.py:45; u_types: rand(N,S),
 * d3pm.py:141; z_lengths: randn_like(lengths), diffusion_helpers.py:158); d_t[B] in 1..T (diffusion_loss.py:213-216):
 *   VE_pbc.forward (diffusion_helpers.py:43-63, with min_distance_sqr_pbc :254-325 and cart_to_frac_coords :233-251)
 *     -> d_noisy_frac[N,3], d_target_eps[N,3] (the wrapped fractional noise, in [0,1));
 *   D3PM.get_xt / q_sample (d3pm.py:119-143) -> d_noisy_types[N];
 *   matrix_to_params (lattice_helpers.py:16-35) -> d_lengths[B,3], d_angles[B,3];
 *   VP_lattice.forward (diffusion_helpers.py:156-163) -> d_noisy_lengths[B,3].
 * d_inv_lattice[B,3,3] receives the inverse cells (scratch the caller owns). */
int arreau_diffusion_noise(const arreau_model* model, const float* d_frac0, const int32_t* d_types0,
                           const float* d_lattice0, const int32_t* d_t, const int32_t* d_crystal_offsets,
                           int32_t B, int32_t N, const float* d_z_frac, const float* d_u_types,
                           const float* d_z_lengths, float* d_noisy_frac, float* d_target_eps,
                           int32_t* d_noisy_types, float* d_noisy_lengths, float* d_lengths, float* d_angles,
                           float* d_inv_lattice, void* stream);

/* The three errors of DiffusionLoss.__call__ (diffusion_loss.py:250-274) from the network outputs on the noised state:
 * compute_frac_x_error (:95-110), D3PM.calculate_loss (d3pm.py:146-163: vb * 0.001 + cross entropy) and
 * mse(pred_lengths, lengths / num_atoms) (:264-267); loss weights 1, 1, 1 (:91-93).
 *   d_losses[6] = {loss, error_frac_x, error_atomic_type, error_lattice, vb, ce};  d_terms[N,3] = per-atom scratch.
 * Optional (may be NULL): the gradients of `loss` with respect to the network outputs -- d_grad_eps[N,3],
 * d_grad_logits[N,S], d_grad_lengths[B,3] -- the seeds of the backward pass (what autograd hands to the model in
 * lightning_wrappers/diffusion.py:108-118). */
int arreau_diffusion_losses(const arreau_model* model, const float* d_pred_eps, const float* d_target_eps,
                            const float* d_logits, const int32_t* d_types0, const int32_t* d_noisy_types,
                            const int32_t* d_t, const float* d_pred_lengths, const float* d_lengths,
                            const int32_t* d_crystal_offsets, int32_t B, int32_t N, float* d_terms,
                            float* d_losses, float* d_grad_eps, float* d_grad_logits, float* d_grad_lengths,
                            void* stream);

/* ---- training runs: keyed forward noising, per-crystal loss rows, their binned reduction ------------------------ */

/* arreau_diffusion_noise with its draws made inside the kernels, keyed by the CRYSTAL and not by its place in the batch:
 * Philox4x32-10, counter = (element, t, kind, crystal id), key = the 64-bit seed.  Draw kinds (after the sampler's 0..8):
 *    9  the timestep uniform   element 0, counter timestep 0
 *   10  z_frac    (normal)     element 3 a + d, a the atom's index WITHIN its crystal
 *   11  u_types   (uniform)    element a S + s
 *   12  z_lengths (normal)     element d
 * normals and uniforms formed from the words as the sampler forms them (Box-Muller of words 0 and 1; 24 bits of word 0).
 *   1. d_crystal_ids[B]: int64, each below 2^32 (the low 32 bits are the counter word; a caller that holds the ids on the host
 *      rejects larger ones).  copies = R >= 1 copies of every crystal may be noised; d_copy[B] (NULL: all 0) says which copy a
 *      row is.  R > T: ARREAU_EINVAL before any work.  A copy outside 0..R-1 is clamped and sets ARREAU_STATUS_BAD_TIMESTEP.
 *   2. the timestep of a row, in integers so that it can be restated exactly: with u24 the top 24 bits of word 0 of the kind-9
 *      draw,   t = 1 + ((copy * 2^24 + u24) * T) / (R * 2^24)   (64-bit integer division).
 *      R = 1 is a uniform draw over 1..T; R > 1 gives each copy of a crystal its own stratum of 1..T, so its copies never
 *      share a timestep.  The kernel writes d_t[B].  given_timesteps != 0: d_t is the caller's and kind 9 is not drawn.
 *      arreau_keyed_timestep is the rule on the host (u24 < 2^24, 0 <= copy < R <= T, else ARREAU_EINVAL).
 *   3. everything after the draws is arreau_diffusion_noise's arithmetic, order and status flags (the same kernels, the draw
 *      source a template argument).  Hence: fed the same numbers as arrays -- arreau_philox_fill_keyed(seed, t_b, kind, id_b)
 *      per crystal -- arreau_diffusion_noise gives the same bits; and a crystal's noised state is a function of
 *      (seed, id, copy, R) alone, whatever the batch around it, its place in it, or the launch geometry.
 * arreau_philox_fill_keyed: d_out[i] = the draw (i, timestep, kind, crystal id) of kinds 9..12 (other kinds: ARREAU_EINVAL;
 * arreau_philox_fill_word keeps its kinds 0..8); d_raw as in arreau_philox_fill. */
int arreau_diffusion_noise_keyed(const arreau_model* model, const float* d_frac0, const int32_t* d_types0,
                                 const float* d_lattice0, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                                 uint64_t seed, const int64_t* d_crystal_ids, int32_t copies, const int32_t* d_copy,
                                 int32_t given_timesteps, int32_t* d_t, float* d_noisy_frac, float* d_target_eps,
                                 int32_t* d_noisy_types, float* d_noisy_lengths, float* d_lengths, float* d_angles,
                                 float* d_inv_lattice, void* stream);
int arreau_philox_fill_keyed(uint64_t seed, int32_t timestep, int32_t kind, uint32_t crystal_id, int64_t n, float* d_out,
                             uint32_t* d_raw, void* stream);
int arreau_keyed_timestep(uint32_t u24, int32_t copy, int32_t copies, int32_t T, int32_t* t_out);

/* One crystal's share of the loss, as SUMS (not means), so that any aggregate can be formed from rows: the reference's batch
 * loss is (sum coord + 0.001 sum vb + sum ce) / N + sum lattice / (3 B) over the rows of a batch. */
typedef struct {
    float coord;        /* sum over the crystal's atoms of d_terms[.][0] (wrapped coordinate error) */
    float vb;           /* ... of d_terms[.][1] */
    float ce;           /* ... of d_terms[.][2] */
    float lattice;      /* sum over the three axes of (pred_length - length / num_atoms)^2 */
    int32_t num_atoms;  /* > 0 in a written row: 0 marks a row no crystal was written to */
    int32_t timestep;
} arreau_loss_row;

/* arreau_diffusion_losses on the same inputs, writing everything it writes (the same two launches: the same bits in d_losses,
 * d_terms and the gradients), plus, in a third launch, for every crystal b the row d_rows[d_row_index[b]] of a caller-owned table
 * of n_rows rows (int64 indices; one outside 0..n_rows-1 writes nothing and sets ARREAU_STATUS_BAD_TIMESTEP).
 * The in-crystal sums have ONE order, which depends on the crystal's atom count alone, not on the batch or the launch geometry:
 * one wave of 64 lanes per crystal; lane l adds the terms of atoms l, l + 64, l + 128, ... of the crystal in ascending order
 * (starting from 0.0f), then the 64 lane sums are combined by the xor butterfly with partner distances 32, 16, 8, 4, 2, 1.  The
 * lattice sum is (e_0 + e_1) + e_2 with e_d = d * d rounded to fp32 on its own.  No float atomics. */
int arreau_diffusion_loss_rows(const arreau_model* model, const float* d_pred_eps, const float* d_target_eps,
                               const float* d_logits, const int32_t* d_types0, const int32_t* d_noisy_types,
                               const int32_t* d_t, const float* d_pred_lengths, const float* d_lengths,
                               const int32_t* d_crystal_offsets, int32_t B, int32_t N, float* d_terms, float* d_losses,
                               float* d_grad_eps, float* d_grad_logits, float* d_grad_lengths, const int64_t* d_row_index,
                               arreau_loss_row* d_rows, int64_t n_rows, void* stream);

/* One launch sums the n_rows rows of a table into n_bins + 1 records: record q < n_bins takes the rows of timestep bin
 * q = (t - 1) * n_bins / T (integer division; t clamped to 1..T), record n_bins every written row.
 *   d_sums[n_bins + 1][4]     float64 sums of coord, vb, ce, lattice;
 *   d_counts[n_bins + 1][2]   int64 atom count and crystal count, followed by ONE more int64, d_counts[2 (n_bins + 1)]: the number
 *                             of unwritten rows (num_atoms <= 0), which are skipped -- how a rank's partial table is recognised.
 * Fixed order, float64: one workgroup of 256 threads per record; thread k adds its rows k, k + 256, ... in row order, then the 256
 * partials meet in the tree with strides 128, 64, ..., 1.  Two launches on one table give the same bits.  1 <= n_bins <= 1024. */
int arreau_loss_rows_reduce(const arreau_loss_row* d_rows, int64_t n_rows, int32_t n_bins, int32_t T, double* d_sums,
                            int64_t* d_counts, void* stream);

/* Training-mode evaluation of the score network on a (noised) batch -- same inputs and outputs as
 * arreau_predict_scores, fp32 throughout, every layer's activations kept for the backward pass (the sampling kernels
 * keep none).  PonitaFiberBundle.forward in train mode (ponita/models/ponita.py:88-123). */
int arreau_train_forward(arreau_model* model, const float* d_frac, const int32_t* d_types, const float* d_lengths,
                         const float* d_angles, const int32_t* d_t, const int32_t* d_crystal_offsets, int32_t B,
                         int32_t N, float* d_eps, float* d_logits, float* d_len0, void* stream);

/* Backward pass of the last arreau_train_forward: given d(loss)/d(eps, logits, len0) (arreau_diffusion_losses), the
 * gradient of every trainable tensor, written to the DEVICE arrays `d_grads` points to, in the state_dict layout
 * of arreau_state_dict (entries for buffers -- ori_grid, t_emb_w, schedules, D3PM matrices -- are ignored).  What
 * loss.backward() leaves in .grad in the reference's training_step (lightning_wrappers/diffusion.py:108-118). */
int arreau_train_backward(arreau_model* model, const float* d_grad_eps, const float* d_grad_logits,
                          const float* d_grad_len0, const arreau_state_dict* d_grads, void* stream);

/* After an optimizer step: refresh the fp32 weights the TRAINING entry points read (arreau_train_forward / backward)
 * from the caller's updated tensors -- `d_sd` holds DEVICE pointers in the state_dict layout (buffers ignored).  Only
 * device-to-device copies: no host repacking between steps.  The sampling kernels' packed operand planes are NOT
 * rebuilt; until the model is re-created from the new state_dict, arreau_predict_scores / arreau_ponita_forward /
 * arreau_sample_loop return ARREAU_EINVAL. */
int arreau_model_update_train_weights(arreau_model* model, const arreau_state_dict* d_sd, void* stream);

/* FiberBundleConv.callibrate's inputs (ponita/nn/conv.py:121-123,140-146) from the last arreau_train_forward:
 * d_stats[L][3] = unbiased std of x (layer input), x_1 (after the spatial conv), x_2 (after the spherical conv). */
int arreau_train_conv_stats(arreau_model* model, float* d_stats, void* stream);

/* Gradient clipping + Adam of the training step as two launches on the step's flat gradient buffer (no counterpart as a
 * function in the reference: `gradient_clip_val=0.5` of pl.Trainer, main_diffusion.py:297 = torch.nn.utils.clip_grad_norm_,
 * then torch.optim.Adam over the two parameter groups of configure_optimizers, lightning_wrappers/diffusion.py:152-218).
 * create: a table of `n_tensors` parameter tensors -- d_params[i] (device pointer, contiguous fp32, numel[i] elements), its
 * position flat_offset[i] in the flat gradient buffer of arreau_train_backward's caller (all the d_grads arrays are views of
 * one allocation of flat_len floats) and its parameter group; host arrays, copied.
 * step (t = args->step, counted from 1): norm = |flat gradient|_2 -> *d_norm_out (may be NULL); coefficient
 * min(max_norm / (norm + 1e-6), 1) (max_norm <= 0: none); per element torch's single-tensor Adam: g = grad * coef
 * (+ weight_decay * p), m += (1 - beta1)(g - m), v = beta2 v + (1 - beta2) g g,
 * p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).  A non-finite norm makes g = 0 for the whole step.
 * d_exp_avg / d_exp_avg_sq: the moments, flat_len floats each, laid out like the gradient buffer (caller-owned: they are the
 * optimizer's state).  Reproducible bit for bit: the norm is a two-stage sum in a fixed order, no atomics.
 * d_mirrors (may be NULL, entries may be NULL): a second destination per tensor for the updated values -- the model's own fp32
 * copy of that tensor (arreau_model_train_weight_pointers), which makes arreau_model_update_train_weights' copies unnecessary;
 * arreau_model_refresh_derived_train_weights then rebuilds the two weights the training entry points read in a derived form
 * (the folded polynomial weight of basis_fn.1, the transposed embedder) from the caller's updated tensors.
 * step_ema: the same step (the same bits in parameters, moments, mirrors and norm), and in the same pass an exponential moving
 * average of the weights (NeMo's EMAOptimizer, lightning_wrappers/callbacks.py:173-180), per element after p is updated:
 *   e = e * d + w * p_new,   d = decay, w = 1 - decay (both formed in double, each rounded to fp32 once; e * d is rounded, then
 *   one fused multiply-add).
 * d_ema: flat_len floats laid out like the gradient buffer (caller-owned, like the moments); 0 <= decay <= 1.  A step whose
 * norm is not finite updates the average too, from the values the step leaves. */
#define ARREAU_OPT_MAX_GROUPS 4
typedef struct arreau_optimizer arreau_optimizer;
typedef struct {   /* doubles: torch forms 1 - beta, 1 - beta^t and lr / (1 - beta1^t) from Python floats before anything is rounded to fp32 */
    int64_t step;
    double lr[ARREAU_OPT_MAX_GROUPS];
    double weight_decay[ARREAU_OPT_MAX_GROUPS];
    double beta1, beta2, eps;
    double max_norm;
} arreau_adam_args;
int arreau_optimizer_create(int32_t n_tensors, void* const* d_params, void* const* d_mirrors, const int64_t* numel,
                            const int64_t* flat_offset, const int32_t* group, int32_t n_groups, int64_t flat_len,
                            arreau_optimizer** out);
int arreau_optimizer_step(arreau_optimizer* opt, const float* d_flat_grad, float* d_exp_avg, float* d_exp_avg_sq,
                          const arreau_adam_args* args, float* d_norm_out, void* stream);
int arreau_optimizer_step_ema(arreau_optimizer* opt, const float* d_flat_grad, float* d_exp_avg, float* d_exp_avg_sq,
                              const arreau_adam_args* args, float* d_ema, double decay, float* d_norm_out, void* stream);
void arreau_optimizer_destroy(arreau_optimizer* opt);
/* DEVICE pointers of the model's own fp32 training weights, stacked [L, ...] in the state_dict layout (NULL: basis_w1,
 * x_embedder_w and every buffer entry). */
int arreau_model_train_weight_pointers(arreau_model* model, arreau_state_dict* out);
int arreau_model_refresh_derived_train_weights(arreau_model* model, const float* d_basis_w1, const float* d_x_embedder_w,
                                               void* stream);

/* The dense product every Linear of the training step runs through (no counterpart in the reference: torch.nn.functional.linear and
 * autograd's matmuls, ponita.py:65-66, conv.py:110-116, convnext.py:24-30), exposed so that the parity tests can call it directly:
 *   C[m][n] = alpha * sum_k A(m, k) B(k, n) + beta * C[m][n],   A(m, k) = d_A[m * as0 + k * as1],  B(k, n) = d_B[k * bs0 + n * bs1]
 * (strides in elements; one of each operand's strides must be 1).  `mode`: 0 = exact fp32 products (v_mfma_f32_32x32x2_f32),
 * 1 = fp16x3, 2 = bf16x6 (three / six 16-bit MFMA products per fp32 product; shapes the split kernel does not take run exact).
 * Device pointers; the split-K scratch is allocated and freed inside (a test hook, not a production entry point). */
int arreau_debug_sgemm(int32_t mode, int32_t M, int32_t N, int32_t K, const float* d_A, int64_t as0, int64_t as1, const float* d_B,
                       int64_t bs0, int64_t bs1, float* d_C, int32_t ldc, float alpha, float beta, void* stream);

/* Timing hook used by bench.py: records hipEvents around the dominant kernel of
 * arreau_predict_scores (the edge kernel) on the stream it is launched on.
 * enable=1 starts collecting; arreau_edge_kernel_time_ms returns the mean over the launches
 * recorded since then (synchronises the events) and the count. */
int arreau_profile_edge_kernel(int32_t enable);
int arreau_edge_kernel_time_ms(double* mean_ms, int64_t* launches);
/* The same for the per-layer message kernel of the default path since round 3 (conv_proj_kernel: kernel projection +
 * message passing + spherical convolution, ponita/nn/conv.py:110-127): L launches per evaluation. */
int arreau_conv_kernel_time_ms(double* mean_ms, int64_t* launches);

/* Debug aid, no reference counterpart: the "uninitialised-state probe".  pattern != 0: every kernel launch of the
 * sampling path is preceded (same stream) by a kernel that fills every CU's LDS and vector registers with `pattern`;
 * 0 switches it off.  A correct kernel's outputs do not depend on what the previous wave left on its CU, so results
 * must be bit-identical for every pattern (eager launches only; process-wide).  tests/test_gpu_parity.py uses it. */
int arreau_debug_set_pollution(uint32_t pattern);
/* The probe's positive control: one kernel per CU READS the whole LDS and 16 vector registers per lane without writing
 * them first and reports the fraction of words equal to `pattern` (close to 1 right after a pollution with it). */
int arreau_debug_leftover_fraction(uint32_t pattern, double* lds_fraction, double* reg_fraction, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARREAU_HIP_H */
