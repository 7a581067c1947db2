// Internal declarations shared by the translation units of libarreau_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <tuple>

#include "../../include/arreau_hip.h"
#include "score_plan.h"

#define ARREAU_NUM_ATTR 6      // inv1, inv2, dist, cos a, cos b, cos c   (transforms/invariants.py:85-88)
#define ARREAU_NUM_MONO 83     // distinct monomials of degree 1..3 in 6 variables (6 + 21 + 56)
#define ARREAU_MONO_PAD 96     // padded to 3 MFMA input tiles of 32
#define ARREAU_POLY_COLS 258   // 6 + 36 + 216 columns of PolynomialFeatures(3)  (nn/embedding.py:10-14)
#define ARREAU_ORI 16

struct arreau_train_ctx;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

void arreau_set_error(const std::string& msg);

#define ARREAU_CHECK_HIP(expr)                                                              \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            arreau_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));           \
            return ARREAU_EHIP;                                                             \
        }                                                                                   \
    } while (0)

#define ARREAU_REQUIRE(cond, msg)                                                           \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            arreau_set_error(std::string(msg));                                            \
            return ARREAU_EINVAL;                                                           \
        }                                                                                   \
    } while (0)

// Conditioned sampling (arreau_sample_condition, include/arreau_hip.h): the known components of the state, device pointers, each
// may be null.  Masks are one byte per atom / crystal, nonzero = known.  Kernels take it by value and hand their helpers a pointer
// to it, or null when the launch has no condition (then the helpers compile to the unconditioned code).
struct SampleConditionDev {
    const float* x0;          // [N,3] known fractional coordinates
    const uint8_t* pos_mask;  // [N]
    const int32_t* a0;        // [N]   known class indices
    const uint8_t* type_mask; // [N]
    const float* l0;          // [B,3] known cell lengths
    const uint8_t* len_mask;  // [B]
    bool operator==(const SampleConditionDev&) const = default;
};

// The sampler state a loop call or a single update works on: device pointers and sizes, the caller's.  Host side only: launchers
// take it by const reference and hand the kernels its members.
struct SampleState {
    float* frac;                 // [N,3]
    int32_t* types;              // [N]
    float* lengths;              // [B,3]
    const float* angles;         // [B,3]
    const int32_t* offsets;      // [B+1]
    int B, N;
    const int32_t* const_types;  // [N] or null: species held
    const float* fixed_lengths;  // [B,3] or null: cell held
    float* lattice;              // [B,3,3] the caller's output cell
    bool operator==(const SampleState&) const = default;
};

// Member-wise equality of the public header's structs that SampleOptions holds (not ours to extend).  The structured binding stops
// compiling when a member is added, so none can be left out of the comparison.
#define ARREAU_MEMBERWISE_EQ(T, ...)                     \
    inline bool operator==(const T& a, const T& b) {     \
        auto members = [](const T& v) {                  \
            const auto& [__VA_ARGS__] = v;               \
            return std::tie(__VA_ARGS__);                \
        };                                               \
        return members(a) == members(b);                 \
    }
ARREAU_MEMBERWISE_EQ(arreau_symmetry, leader, op, orbit, orbit_ptr, orbit_atoms, stab_ptr, stab_ops, rot, rot_inv, trans, n_orbits, n_orbit_atoms,
                     n_stab_ops, n_ops)
ARREAU_MEMBERWISE_EQ(arreau_multistep, hist_eps, hist_x0, hist_t_atom, hist_t_len)
ARREAU_MEMBERWISE_EQ(arreau_species_control, d_allow, temperature)
ARREAU_MEMBERWISE_EQ(arreau_contact_guidance, min_distance, weight, max_shells, d_energy, d_contacts, d_flags)
ARREAU_MEMBERWISE_EQ(arreau_xrd_params, wavelength, two_theta_min, two_theta_max, fwhm, b_iso, n_points, max_index)
ARREAU_MEMBERWISE_EQ(arreau_xrd_guidance, params, weight, d_target, d_class_weights, d_atom_weights, d_distance, d_reflections, d_flags)
#undef ARREAU_MEMBERWISE_EQ

// Respaced sampling (arreau_sample_loop_scheduled, arreau_reverse_step_to; the rules are stated in include/arreau_hip.h): the step
// that leaves timestep t of crystal b produces the state at s = s_of[b] when s_of is given, else s = next[t] (the device-side
// next-timestep table [T+1] of the loop).  Kernels take it by value and hand their helpers a pointer to it, or null when the
// launch has no schedule (then s = t - 1 and the helpers compile to the schedule-less code).
struct StepScheduleDev {
    const int32_t* next;  // [T+1] or null
    const int32_t* s_of;  // [B]   or null
    float clipmax;        // the VP schedule's beta clip (VP_lattice clipmax)
    bool operator==(const StepScheduleDev&) const = default;
};

// Predictor-corrector sampling (arreau_sample_loop_corrected, arreau_corrector_step; the rule is stated in include/arreau_hip.h):
// M corrector moves at the step's timestep come before the predictor, each after a full network evaluation on the current state.
struct CorrectorDev {
    int steps;  // M (0: the plain step)
    float snr;
    bool operator==(const CorrectorDev&) const = default;
};

// What modifies a step of the sampler, on the host side, as the launchers read it: pointers, null / zero for the plain step.  A loop
// call's is a view of its SampleOptions (below); a step export fills its own.  The launchers pick the kernel instance from it.
struct StepOptions {
    const SampleConditionDev* cond = nullptr;  // conditioned sampling (the COND instances); needs Philox noise
    const StepScheduleDev* sched = nullptr;    // respaced step: s from a table or per crystal; null: s = t - 1
    CorrectorDev corr{};                       // corrector moves before the predictor
    const int32_t* pass = nullptr;        // resampled loop: the device word of the pass index, word3 = 256 pass[0] (RESAMPLE)
    const int32_t* length_tie = nullptr;  // lattice systems: the tie code per crystal (TIE)
    const arreau_symmetry* sym = nullptr; // space-group symmetry: the orbit tables (SYM); not with a condition or a resampled loop
    float eta = -1.0f;                    // DDIM-style step (ETA): the noise scale in [0, 1]; negative: the ancestral step.  Not with sym
    const arreau_multistep* ms = nullptr; // second-order multistep (MS): the history buffers; eta is then 0; a schedule and a tie only
    bool invert = false;                  // DDIM inversion (INVERT): `sched` names the HIGHER level every crystal climbs to; no other option
    const arreau_species_control* species = nullptr;  // species control (SPEC): the admission rows and the temperature; not with invert
    const uint64_t* crystal_seeds = nullptr;  // keyed sampling: the stream seed of every crystal (StepNoiseSrc::seeds of every draw)
    const arreau_contact_guidance* guide = nullptr;  // contact guidance: one launch on the eps of every evaluation; null (also for weight 0): none; not with invert
    const arreau_xrd_guidance* xrd_guide = nullptr;  // XRD guidance: one launch on that eps, after contact guidance's; null (also for weight 0): none; not with invert
};

// The options of one loop call, checked, normalised and held by value (api.hip: resolve_loop_request is the one place that fills
// it): what every step of the call reads, and -- being all of it -- the options' part of the key of a captured step.  An absent
// option is its value-initialised member whatever the caller's struct held (a NULL corrector and steps == 0, a NULL guidance and
// weight == 0 are the same options); eta is -1 without one.  The floats compare with ==, which for these values is equality of
// their bits: every accepted one is finite and never -0 (the checks reject the rest, x + 0.0f turns -0 into +0).  No member
// initialisers: it lives in the zero-filled model.
struct SampleOptions {
    SampleConditionDev cond;       // conditioned sampling: the six pointers (all null: none)
    StepScheduleDev sched;         // respaced sampling: the table and the clip (next null: every timestep)
    CorrectorDev corr;             // corrector moves (steps 0, snr 0: none)
    int32_t resample_passes, resample_jump;  // RePaint resampling: R and J (0, 0: none)
    const int32_t* pass;           // ... and the workspace word of the pass index its steps read
    const int32_t* length_tie;     // lattice systems: the tie codes (null: untied)
    arreau_symmetry sym;           // space-group symmetry: the tables (leader null: none)
    float eta;                     // DDIM-style steps: their eta (negative: ancestral steps)
    arreau_multistep ms;           // second-order multistep: the history buffers (hist_eps null: none)
    bool invert;                   // DDIM inversion (arreau_invert_loop): other kernels on the same buffers and table
    bool species_on;               // species control: whether the steps are the SPEC instances ...
    arreau_species_control species;  // ... and their admission rows and temperature
    const uint64_t* crystal_seeds; // keyed sampling: the table of stream seeds (null: not keyed)
    arreau_contact_guidance guide; // contact guidance: parameters and diagnostic arrays (weight 0: none)
    arreau_xrd_guidance xrd_guide; // XRD guidance: parameters, target, amplitudes and diagnostic arrays (weight 0: none)
    bool operator==(const SampleOptions&) const = default;
    StepOptions view() const {     // valid while *this is
        return StepOptions{.cond = cond.pos_mask || cond.type_mask || cond.len_mask ? &cond : nullptr, .sched = sched.next ? &sched : nullptr,
                           .corr = corr, .pass = pass, .length_tie = length_tie, .sym = sym.leader ? &sym : nullptr, .eta = eta,
                           .ms = ms.hist_eps ? &ms : nullptr, .invert = invert, .species = species_on ? &species : nullptr,
                           .crystal_seeds = crystal_seeds, .guide = guide.weight > 0.0f ? &guide : nullptr,
                           .xrd_guide = xrd_guide.weight > 0.0f ? &xrd_guide : nullptr};
    }
};

// What the cached executable graph of arreau_sample_loop was captured for: the buffers, the seed, every kernel choice of the
// evaluation and all the options, which are kernel arguments or launch choices of the capture.  A new option is a member of
// SampleOptions and so part of the key.  SampleGraphKey{} (the zero-filled model's) is the key no call has.
struct SampleGraphKey {
    SampleState state;      // buffers and sizes
    const void* workspace;
    uint64_t seed;          // the Philox seed
    ScorePlan plan;
    SampleOptions opt;
    bool operator==(const SampleGraphKey&) const = default;
};

// Packed weights resident in HBM.  All pointers are device pointers into `blob`.
struct arreau_model {
    arreau_config cfg;
    int S, C, D, L, O, W, H, k, T;
    float* blob;
    size_t blob_floats;
    const float* ori;        // [O][3]
    const float* w1p;        // basis layer 1, folded onto 83 monomials, MFMA-packed  out C, in 96
    const float* b1;         // [C]
    const float* w2p;        // basis layer 2, MFMA-packed                            out D, in C
    const float* b2;         // [D]
    const float* wkp;        // [L] conv.kernel.weight, MFMA-packed                   out C, in D
    const float* edge_bf16;  // w1 | w2 | wk_l as bf16x3 chunks (uint16 data), one chunk per output tile
    const float* edge_f16;   // w1 | w2 | wk_l as fp16x3 chunks (uint16 data, two planes), one chunk per output tile
    int f16_ok;              // 1 when every packed weight fits fp16 (|w| < 6e4): the fp16x3 kernels may be used
    const float* conv_x8;    // [L] fp8 e4m3 cross-product operands of conv.kernel.weight (conv_proj.hip, round 4; uint8 data)
    int x8_ok;               // 1 when 64 |w| <= 448 for every kernel weight AND the calibration allows it: the fp8 cross products may be used
    int x8_weights_ok;       // 64 |w| <= 448 for every kernel weight (what x8_ok may be switched back to)
    int fp8_ok;              // 1 when the fp8 (e4m3) residual plane of the basis stash passed the end-to-end calibration (model.hip: calibrate_message_formats)
    float calib_fp8, calib_x8;  // share of the parity bounds the formats used up on the calibration batch (fp8 residual plane; that + fp8 cross products); -1: not measured
    int train_full_range;    // 1: the training forward runs bf16x6 products even where the weights fit fp16 (arreau_model_set_variant(.., 1))
    int calibrating;         // 1 while that calibration runs: basis form at any launch size, formats from fp8_ok / x8_ok alone
    float edge_act_bound, node_act_bound;  // weight-derived bounds of the fp16 operands of the edge / ConvNext chains (model.hip)
    // Arithmetic / geometry variants requested for this model (defaults from ARREAU_*_VARIANT at create,
    // arreau_model_set_variant overrides) and the plan the last evaluation of the score network executed (all zero: none yet).
    int edge_variant, mlp_variant, conv_variant, readout_variant;
    mutable ScorePlan ran;
    // training (train_net.hip): plain row-major fp32 copies of the weights the sampling kernels hold only in packed
    // form, and the step's activation buffers (created on first use)
    const float *t_w1f, *t_w2, *t_wk, *t_lin1, *t_lin2, *t_ro_w;
    struct arreau_train_ctx* train;
    int fused;               // 1: shape (C, D, W) = (128, 256, 4), the fused kernels' packed weights exist
    int packed_stale;        // 1 after arreau_model_update_train_weights: the sampling kernels' packed planes are out of date
    void* loop_stream;       // hipStream_t / hipEvent_t of arreau_sample_loop's graph mode (capture is not allowed on the
    void* loop_event;        //   legacy default stream callers usually pass); created on first use
    SampleGraphKey graph_key;  // what the cached executable graph of arreau_sample_loop was captured for
    void* retired_graph;     // hipGraphExec_t of the last arreau_sample_loop (+ the stream it was launched on): destroyed,
    void* retired_stream;    //   after that stream has drained, by the next loop or by arreau_model_destroy
    int32_t* status;         // device word of sticky ARREAU_STATUS_* bits (written by the kernels with atomicOr)
    float* fk;               // [L][O(o)][O(p)][C] fiber kernels / O (written once by the precompute kernel)
    const float* conv_bias;  // [L][C]
    const float* ln_w;       // [L][C]
    const float* ln_b;       // [L][C]
    const float* mlp;        // [L][4 quarters][ linear_1 rows of the quarter (out H/4, in C) | linear_2 columns of the
                             //  quarter (out C, in H/4) ], MFMA-packed: one linear stream per (layer, quarter)
    const float* mlp_bf16;   // the same stream as bf16x3 chunks (uint16 data), 24 KiB per output tile
    const float* mlp_f16;    // the same stream as fp16x3 chunks (uint16 data), 16 KiB per output tile
    const float* mlp_f16m;   // ... as fp16x3 chunks for v_mfma_f32_16x16x32_f16 (node_f16m.hip)
    const float* mb1;        // [L][H]
    const float* mb2;        // [L][C]
    const float* ls;         // [L][C] layer_scale (ones when absent)
    const float* embT;       // [S+78][C] x_embedder.weight transposed
    const float* ro_wT;      // [L][C][S+4] read_out weight transposed
    const float* ro_b;       // [L][S+4]
    const float* ro_pack;    // [L][(S+4 padded to 32)/32][C/32][1024] read_out weights as fp32-MFMA fragment streams
    const float* ro_wv;      // [L][C] vector read-out weights (column S of read_out_layers), contiguous
    float ro_bv_host[16];    // [L] vector read-out bias (host copy, passed by value)
    const float* t_emb_w;    // [32]
    const float* ve_sigmas;  // [T+1]
    const float* vp_alpha_bars;  // [T+1]
    const float* vp_betas;   // [T+1]
    const float* q1t;        // [T][S][S]
    const float* qmats;      // [T][S][S]
    int qmats_absorbing;     // 1 when every Qbar_t is diagonal + last ("mask") column: the D3PM update skips the dense S x S read
    // raw fiber-basis MLP (only used by the one-time precompute kernel)
    const float* fiber_w1;   // [C][3]
    const float* fiber_b1;   // [C]
    const float* fiber_w2;   // [D][C]
    const float* fiber_b2;   // [D]
    const float* fiber_wk;   // [L][C][D] conv.fiber_kernel.weight
};

// ---------------------------------------------------------------------------------------------
// MFMA building block.  All dense layers are evaluated "transposed":
//     Y^T[out, row] = W[out, in] . X^T[in, row]
// with v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD).  A 32x32 output tile lives in 16
// accumulator registers per lane: lane (h = lane>>5, j = lane&31) holds, in register r,
//     Y^T[32u + rho(r,h)][row j],   rho(r,h) = (r&3) + 8*(r>>2) + 4*h.
// Because the reduction index of the NEXT layer is this tile's row index, the accumulator is
// directly the B operand of the next MFMA chain (register r of tile t feeds the k-step whose two
// k values are rho(r,0) and rho(r,1)): activations never leave registers between layers.
// The A operand (weights) is pre-packed on the host so one 16-byte load per lane serves 4 k-steps:
//     P[u][t][q][lane][m] = W[out = 32u + (lane&31)][in = 32t + 8q + 4*(lane>>5) + m]
// (u: out tile, t: in tile, q: 0..3, m: 0..3) -- 1 KiB contiguous per wave-load.
// ---------------------------------------------------------------------------------------------
#define ARREAU_PACK_TILE_FLOATS 1024  // floats per (u,t) tile: 4 q * 64 lanes * 4

__device__ __forceinline__ f32x16 arreau_mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Weights are consumed as ONE linear stream of 16-byte fragments per wave (1 KiB per wave-load).  Output
// tiles are produced one at a time (out-tile-major): for output tile u the k-groups g = 0..G-1 (G = 4 * input
// tiles) are contiguous, 256 floats apart, and tile u+1 follows.  The stream is prefetched ARREAU_PF groups
// ahead through a register ring, so L2 latency hides behind ARREAU_PF * 4 * NCB MFMAs (64 cycles each).
// NCB = 32-row column blocks sharing each fragment.  f0 (first group of this tile within `region`) must be a
// compile-time constant after unrolling so that ring slots are static registers.
#define ARREAU_PF 8

template <int G, int NIN, int NCB>
__device__ __forceinline__ void arreau_stream_tile(f32x16 (&acc)[NCB], f32x4 (&ring)[ARREAU_PF],
                                                   const float* __restrict__ region, const int f0,
                                                   const f32x16 (&b)[NIN][NCB]) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int f = f0 + g;
        const f32x4 a = ring[f % ARREAU_PF];
        ring[f % ARREAU_PF] = *reinterpret_cast<const f32x4*>(region + (size_t)(f + ARREAU_PF) * 256);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = arreau_mfma(a[m], b[g >> 2][cb][4 * (g & 3) + m], acc[cb]);
        }
    }
    // pin the issue order inside this scheduling region: one fragment prefetch, then its 4*NCB MFMAs
#pragma unroll
    for (int g = 0; g < G; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);        // VMEM read
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * NCB, 0);  // MFMA
    }
}

// accumulator tile initialised with a bias: register r gets bias[32u + rho(r,h)]
__device__ __forceinline__ f32x16 arreau_bias_tile(const float* __restrict__ bias, int u, int h) {
    f32x16 r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(bias + 32 * u + 8 * q + 4 * h);
        r[4 * q] = v[0]; r[4 * q + 1] = v[1]; r[4 * q + 2] = v[2]; r[4 * q + 3] = v[3];
    }
    return r;
}

// Branch-free erf (two polynomial pieces, both evaluated, one selected): the library erff branches on
// |x|, which splits the fully unrolled MFMA chains into hundreds of basic blocks and wrecks register
// allocation.  Coefficients: N. Juffa's single-precision erf (max error < 1 ulp with an accurate exp);
// v_exp_f32 adds about 2e-7 relative on the exp term, far inside the 1e-5 parity budget.
__device__ __forceinline__ float arreau_erf(float a) {
    const float t = fabsf(a);
    const float s = a * a;
    float r = fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
    const float u = fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
    r = fmaf(r, s, u);
    r = fmaf(r, t, -1.06777877e-1f);
    r = fmaf(r, t, -6.34846687e-1f);
    r = fmaf(r, t, -1.28717512e-1f);
    r = fmaf(r, t, -t);
    r = 1.0f - __builtin_amdgcn_exp2f(r * 1.44269504088896341f);
    r = copysignf(r, a);
    float p = -5.96761703e-4f;
    p = fmaf(p, s, 4.99119423e-3f);
    p = fmaf(p, s, -2.67681349e-2f);
    p = fmaf(p, s, 1.12819925e-1f);
    p = fmaf(p, s, -3.76125336e-1f);
    p = fmaf(p, s, 1.28379166e-1f);
    p = fmaf(p, a, a);
    return t > 0.927734375f ? r : p;
}

// exact (erf) GELU, torch.nn.GELU() default
__device__ __forceinline__ float arreau_gelu(float x) {
    return 0.5f * x * (1.0f + arreau_erf(x * 0.70710678118654752440f));
}

// Noise of one reverse step: either the caller's arrays (parity mode: the reference's draws injected) or drawn in the
// kernel from Philox4x32-10 keyed by (seed, timestep, draw kind, element) -- no RNG launches, no noise arrays in HBM.
struct StepNoiseSrc {
    const float* z_lattice;  // [B,3]  or null
    const float* z_frac;     // [N,3]  or null
    const float* u_types;    // [N,S]  or null
    uint64_t seed;           // used when the arrays are null
    // keyed sampling (arreau_sample_loop_keyed; rules in include/arreau_hip.h): the stream seed of every crystal [B], or null.  With
    // it a draw of crystal b takes seeds[b] for `seed` and counts its element within the crystal; without it nothing changes.
    const uint64_t* seeds;
};

inline bool arreau_condition_empty(const SampleConditionDev* c) {
    return !c || !((c->x0 && c->pos_mask) || (c->a0 && c->type_mask) || (c->l0 && c->len_mask));
}
int arreau_condition_to_dev(const arreau_sample_condition* c, SampleConditionDev* out);  // update.hip
// Space-group symmetry (arreau_sample_loop_sym, arreau_reverse_step_sym): ARREAU_EINVAL unless every table pointer is given and
// every size is positive.  The kernels take the table struct by value and check every index before they follow it.
int arreau_symmetry_check(const arreau_symmetry* y, const char* who);  // update.hip

// Predictor-corrector sampling: ARREAU_EINVAL unless 0 <= steps <= ARREAU_MAX_CORRECTOR_STEPS and (steps == 0 or snr finite and > 0).
int arreau_corrector_check(int32_t steps, float snr, const char* who);
// DDIM-style sampling (arreau_sample_loop_eta, arreau_reverse_step_eta; the rules are stated in include/arreau_hip.h):
// ARREAU_EINVAL unless eta is finite and lies in [0, 1].
int arreau_eta_check(float eta, const char* who);  // update.hip
// Second-order multistep sampling (arreau_sample_loop_multistep, arreau_reverse_step_multistep): ARREAU_EINVAL unless the struct and
// its four history pointers are given.
int arreau_multistep_check(const arreau_multistep* ms, const char* who);  // update.hip
// Species control (arreau_sample_loop_species, arreau_reverse_step_species): ARREAU_EINVAL unless the struct is given and its
// temperature is finite and not negative; *out receives the struct the kernels take.
int arreau_species_check(const arreau_species_control* species, const char* who, arreau_species_control* out);  // update.hip

// Contact guidance (arreau_sample_loop_guided, arreau_contact_guidance_step; the rules are stated in include/arreau_hip.h).
// arreau_contact_guidance_check: ARREAU_EINVAL unless the struct is given, min_distance is finite and > 0, weight finite and >= 0 and
// max_shells in 1..ARREAU_SCREEN_MAX_SHELLS.  The launch reads st.frac / offsets / B / N, the per-crystal timesteps d_t and the cells
// d_lattice [B,9] the evaluation saw, and rewrites d_eps [N,3] in place (contact_guide.hip).
int arreau_contact_guidance_check(const arreau_contact_guidance* g, const char* who);
int arreau_launch_contact_guide(const arreau_model* m, const SampleState& st, const int32_t* d_t, const float* d_lattice, float* d_eps,
                                const arreau_contact_guidance& opt, hipStream_t s);

// XRD guidance (arreau_sample_loop_xrd_guided, arreau_xrd_guidance_step; the rules are stated in include/arreau_hip.h).
// arreau_xrd_guidance_check: ARREAU_EINVAL unless the struct is given, its arreau_xrd_params pass the xrd launch's validation, weight
// is finite and >= 0, the target is given and exactly one of the amplitude arrays is (a loop: the class weights).  The launch reads
// st.frac / types / offsets / B / N, the per-crystal timesteps d_t and the cells d_lattice [B,9] the evaluation saw, rewrites d_eps
// [N,3] in place and writes g to d_gradient [N,3] when that is given (xrd_guide.hip).
int arreau_xrd_guidance_check(const arreau_xrd_guidance* g, const char* who, bool step_export);
int arreau_launch_xrd_guide(const arreau_model* m, const SampleState& st, const int32_t* d_t, const float* d_lattice, float* d_eps,
                            const arreau_xrd_guidance& opt, float* d_gradient, hipStream_t s);

// One corrector move per crystal at timestep d_t[b]: z from the caller's d_z_frac [N,3], or (d_z_frac null) the Philox draw
// (seed, t, ARREAU_DRAW_Z_CORRECTOR, element, iter; 256 pass[0] + iter with opt.pass; keyed by opt.crystal_seeds when given).  Reads
// st.frac / offsets / B / N, opt.corr.snr, opt.pass, opt.crystal_seeds and of opt.cond the position mask (null / no mask: every atom moves).
int arreau_launch_corrector(const arreau_model* m, const SampleState& st, const int32_t* d_t, const float* d_eps, const float* d_z_frac,
                            uint64_t seed, uint32_t iter, const StepOptions& opt, hipStream_t s);

// RePaint resampling (arreau_sample_loop_resampled, arreau_resample_jump; the rules are stated in include/arreau_hip.h).
// arreau_resampling_check: ARREAU_EINVAL unless 1 <= passes <= ARREAU_MAX_RESAMPLE_PASSES and jump_length >= 1.
int arreau_resampling_check(int32_t passes, int32_t jump_length, const char* who);
// The jump s -> t of every crystal of `st`: (s, t) from the per-crystal arrays d_s / d_t, or, when those are null, the scalars s / t
// (the loop's block bottom and top).  Noise from the caller's arrays, or (all null) Philox (seed, t, kinds 6-8, element, pass).
// Loop form (loop != null): also the workspace cell and the per-crystal embedding of the next step for t, the device timestep
// set to t (loop->t_next = t, loop->t_cur = t + 1: the entry from which the next step advances) and loop->pass = `pass`.
struct JumpLoopDev {
    float* lattice_ws;  // [B,9]
    float* cvec;        // [B,C]
    int32_t* t_next;    // [B]
    int32_t* t_cur;     // [B]
    int32_t* pass;      // [1]
};
int arreau_launch_resample_jump(const arreau_model* m, const SampleState& st, const int32_t* d_s, const int32_t* d_t, int s, int t,
                                const int32_t* d_batch, const StepNoiseSrc& noise /* z_lattice: the lengths' draws */, uint32_t pass,
                                const SampleConditionDev* cond, const JumpLoopDev* loop,
                                const int32_t* d_length_tie /* lattice systems: the tie code per crystal (the TIE instance), or null */,
                                hipStream_t stream);

void arreau_train_ctx_destroy(struct arreau_train_ctx* t);
// The score network on the shape-general fp32 kernels (the training forward without its own graph construction): graph
// arrays and the embedded features x0 [N*16][C] (null: t.x already holds them) are the caller's; outputs as
// arreau_predict_scores.  Keeps every activation (a following arreau_train_backward is valid when keep_graph copies).  Records a
// general plan in m->ran.
struct arreau_graph_view {
    const int32_t *batch, *deg, *src;
    const float *lattice, *dir, *dist;
};
int arreau_general_network(arreau_model* m, const arreau_graph_view& g, const int32_t* d_off, int B, int N, float* d_eps,
                           float* d_logits, float* d_len0, hipStream_t s);
float* arreau_general_x0(arreau_model* m, int N, int B, hipStream_t s);  // (re)sizes the context; returns its layer-0 feature buffer
void arreau_model_retire_graph(arreau_model* m, void* exec, void* stream);  // takes ownership; frees the previous one

// CUs of the current device, queried once per process (one process drives one GPU); 256 if the query fails.  The persistent
// kernels launch one workgroup per CU.
inline int arreau_cu_count() {
    static const int n_cu = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            return (int)prop.multiProcessorCount;
        return 256;
    }();
    return n_cu;
}

// The plan of one evaluation of N atoms on this model (score_plan.h); reads the environment, so once per library call.
inline ScorePlan arreau_score_plan(const arreau_model* m, int N) {
    return score_plan(ScorePlanInputs{m->fused, m->C, m->D, m->H, m->L, m->k, m->S, m->f16_ok, m->fp8_ok, m->x8_ok, m->calibrating,
                                      m->edge_variant, m->mlp_variant, m->conv_variant, m->readout_variant, arreau_cu_count()},
                      score_switches(), N);
}

// Debug aid (api.hip, "uninitialised-state probe"): when a pollution pattern is set (arreau_debug_set_pollution), every
// kernel launch of the sampling path is preceded, on the same stream, by a kernel that fills every CU's LDS and vector
// registers with the pattern.  A kernel that reads LDS / registers it never wrote sees whatever the previous wave on its
// CU left there: alone on the GPU that is its own kernel's leftovers (the same every run), next to another stream's or
// process's kernels it is not -- the signature of the non-reproducibility DESIGN.md section 8 records.  With the probe the
// leftovers are under the test's control: outputs must be bit-identical for every pattern
// (tests/test_gpu_parity.py::test_outputs_do_not_depend_on_leftover_lds_or_registers).
extern unsigned arreau_debug_pollution;  // 0 = off (the product never sets it)
int arreau_debug_pollute(hipStream_t s);
#define ARREAU_LAUNCH(kernel, grid, block, smem, stream, ...)                      \
    do {                                                                           \
        if (arreau_debug_pollution) (void)arreau_debug_pollute(stream);            \
        hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);        \
    } while (0)

// launchers implemented in the other translation units ------------------------------------------
int arreau_launch_fiber_precompute(arreau_model* m, hipStream_t s);
int arreau_launch_neighbor(const float* cart, const float* lattice, const int32_t* offsets, const int32_t* batch, int B, int N,
                           float radius, int k, int32_t* deg, int32_t* src, int32_t* cell, float* dir, float* dist,
                           hipStream_t s);
// neighbour list + embedding of the sampler's node features in one launch (graph.hip; both read prep_kernel's outputs only)
int arreau_launch_neighbor_embed(const arreau_model* m, const float* cart, const float* lattice, const int32_t* offsets,
                                 const int32_t* batch, int B, int N, int32_t* deg, int32_t* src, int32_t* cell, float* dir,
                                 float* dist, const float* frac, const int32_t* types, const float* cvec, float* x0, hipStream_t s,
                                 int32_t* tick = nullptr /* sampling loop without a prep launch: see the kernel */,
                                 const int32_t* next_t = nullptr /* respaced loop: tick[b] = next_t[tick[b]] */,
                                 bool advance = true /* false: the loop form without advancing tick (a corrector's re-evaluation) */);
int arreau_launch_prep(const arreau_model* m, const float* frac, const float* lengths, const float* angles,
                       const int32_t* t, const int32_t* offsets, int B, int N, float* lattice, float* cart,
                       int32_t* batch, float* cvec, hipStream_t s, int32_t* t_next = nullptr, int32_t* t_cur = nullptr,
                       int t_offset = 0, const int32_t* next_t = nullptr /* respaced loop: t_next[b] = next_t[t] */);
// What one reverse-update launch reads besides the state and the options.
struct ReverseInputs {
    const int32_t* t;                  // [B] the timestep each crystal leaves
    const float *eps, *logits, *len0;  // the network's outputs
    StepNoiseSrc noise;
    const float* gs_atoms = nullptr;   // pool these per-atom read-outs into len0 first
    const int32_t* batch = nullptr;    // crystal index of each atom, if the caller has it
    // sampling loop: also prepare the next step (workspace lattice + per-crystal embedding for timestep t - 1), see reverse_crystal_block
    float* lattice_ws = nullptr;
    float* cvec_next = nullptr;
};
int arreau_launch_reverse(const arreau_model* m, const SampleState& st, const ReverseInputs& in, const StepOptions& opt, hipStream_t s);
// The launchers below execute the plan they are given (score_plan.h); they refuse shapes their kernels do not take and launch.
int arreau_launch_edge(const arreau_model* m, const ScorePlan& plan, const float* dir, const float* dist, const int32_t* deg,
                       const int32_t* batch, const float* lattice, int N, float* kbuf, hipStream_t s);
int arreau_launch_edge_bf16x6(const arreau_model* m, const float* dir, const float* dist, const int32_t* deg,
                              const int32_t* batch, const float* lattice, int N, float* kbuf, hipStream_t s);
int arreau_launch_edge_f16x3(const arreau_model* m, const ScorePlan& plan, const float* dir, const float* dist, const int32_t* deg,
                             const int32_t* batch, const float* lattice, int N, float* kbuf, hipStream_t s);
int arreau_launch_embed(const arreau_model* m, const float* frac, const int32_t* types, const float* lattice,
                        const int32_t* batch, const float* cvec, int N, float* x0, hipStream_t s);
int arreau_launch_embed_general(const arreau_model* m, const float* x, const float* vec, int N, float* x0, hipStream_t s);
int arreau_launch_batch_index(const int32_t* offsets, int B, int N, int32_t* batch, hipStream_t s);
// kbuf: the per-layer edge kernels K [L][N*k*16][C] as fp32 -- the K pair: an edge kernel that projects in place + the streamed conv
// kernel or the small-layer kernel, for launches too small for the basis form -- or (plan.basis_form) the stash of windowed basis
// planes, which each layer's message kernel projects itself (conv_proj.hip).  All forms evaluate the same numbers: the basis form
// with three fp16 cross products (!plan.cross_fp8) is bit-identical to the K pair, with the fp8 cross products close to it, not equal.
int arreau_launch_node_layer(const arreau_model* m, const ScorePlan& plan, int layer, const float* kbuf, const int32_t* deg,
                             const int32_t* src, const float* x_in, float* x_conv, float* x_out, float* xbar,
                             float* vsum, int N, hipStream_t s);
void arreau_prof_conv(int end, hipStream_t s);  // api.hip: hipEvents around the message kernel while bench.py profiles
int arreau_launch_conv_proj(const arreau_model* m, const ScorePlan& plan, int layer, const float* basis, const int32_t* deg,
                            const int32_t* src, const float* x_in, float* x_conv, int N, hipStream_t s);

int arreau_launch_mlp_bf16x6(const arreau_model* m, int layer, const float* x_conv, const float* x_in, float* x_out,
                             float* xbar, float* vsum, int N, hipStream_t s);
bool arreau_mlp_train_forward_available(const arreau_model* m);
int arreau_launch_mlp_train_forward(const arreau_model* m, int layer, const float* x_conv, const float* x_in, float* x_out, float* xhat,
                                    float* rstd, float* xn, float* hpre, float* h, float* out, int N, hipStream_t s,
                                    // round 5: the spatial conv + spherical mix of the layer inside the same launch (kl = the layer's kernels,
                                    // rows kl_pitch floats apart; x1 receives the spatial conv's output; x_conv is not read) -- null: x_conv given
                                    const float* kl = nullptr, int kl_pitch = 0, const int32_t* deg = nullptr, const int32_t* src = nullptr,
                                    const float* fk = nullptr, float* x1 = nullptr);
int arreau_repack_mlp_f16x3_m16(arreau_model* m, hipStream_t s);
// the tile form: nb nodes per wave, a weight ring of `slots` chunks (plan.mlp_nb, plan.mlp_slots)
int arreau_launch_mlp_f16x3_m16(const arreau_model* m, int nb, int slots, int layer, const float* x_conv, const float* x_in,
                                float* x_out, float* xbar, float* vsum, int N, hipStream_t s);
// one launch per layer for small launches (node_f16m.hip): conv_kernel_streamed<128> + the split MLP form
int arreau_launch_small_layer(const arreau_model* m, int layer, const float* kbuf, const int32_t* deg, const int32_t* src,
                              const float* x_in, float* x_out, float* xbar, float* vsum, int Ntot, hipStream_t s);
int arreau_launch_mlp_f16x3_m16_split(const arreau_model* m, int layer, const float* x_conv, const float* x_in, float* x_out,
                                      float* xbar, float* vsum, int N, hipStream_t s);
int arreau_launch_readout(const arreau_model* m, ScorePlan::Readout kernel, const float* xbar, const float* vsum,
                          const int32_t* offsets, int B, int N, float* gs, float* eps, float* logits, float* len0, hipStream_t s);
