// RePaint resampling (Lugmayr et al., CVPR 2022): the forward jump of the whole sampler state from a block's bottom s up to its
// top t, in closed form (rules in include/arreau_hip.h, section "RePaint resampling").  One launch:
//   the first B workgroups (256 threads, one per crystal, like reverse_crystal_block): VP_lattice.forward s -> t of the lengths,
//          the cell, and in the loop the next step's set-up for t (workspace cell, per-crystal embedding, device timestep);
//   the others, four waves each, one wave per atom (like reverse_atoms_body): VE_pbc.forward s -> t of the position, then
//          D3PM.q_sample s -> t of the species as a Gumbel arg-max over the S classes across the 64 lanes.
// The two parts touch disjoint data.  Noise: the caller's arrays (arreau_resample_jump) or Philox (seed, t, kind 6/7/8,
// element, pass) drawn in the kernel (the loop).
#include <cmath>

#include "update_dev.h"

namespace {
constexpr int JUMP_THREADS = 256;

struct JumpTimes {
    const int32_t* s_of;  // [B] or null: `s`
    const int32_t* t_of;  // [B] or null: `t`
    int s, t;
};

// (s, t) of crystal b, clamped to 1 <= t <= T and 0 <= s <= t - 1; `bad` when either was moved
__device__ __forceinline__ void jump_pair(const JumpTimes& jt, int b, int T, int& s, int& t, bool& bad) {
    const int tr = jt.t_of ? jt.t_of[b] : jt.t, sr = jt.s_of ? jt.s_of[b] : jt.s;
    t = tr < 1 ? 1 : (tr > T ? T : tr);
    s = sr < 0 ? 0 : (sr > t - 1 ? t - 1 : sr);
    bad = t != tr || s != sr;
}

struct JumpNoise {
    const float* z_frac;     // [N,3] or null
    const float* z_lengths;  // [B,3] or null
    const float* u_types;    // [N,S] or null
    uint64_t seed;
    uint32_t pass;           // counter word3 of the Philox draws
    const uint64_t* seeds;   // keyed sampling: the stream seed of every crystal [B] (StepNoiseSrc::seeds), or null
};
// the keys of the jump's Philox draws (update_dev.h: atom_draw_key / length_draw_key)
__device__ __forceinline__ StepNoiseSrc jump_key_src(const JumpNoise& n) { return StepNoiseSrc{nullptr, nullptr, nullptr, n.seed, n.seeds}; }

// TIE: lattice systems (arreau_resample_jump_tied, the tied loop): the axes tied by length_tie[b] jump together from the leader's
// length with the leader's draw (rule 2 of the section in include/arreau_hip.h); a crystal whose lengths len_mask knows is not tied.
// Without TIE neither pointer is read.
template <bool TIE>
__global__ __launch_bounds__(JUMP_THREADS) void resample_jump_kernel(
    int B, int N, float* __restrict__ frac, int32_t* __restrict__ types, float* __restrict__ lengths, const float* __restrict__ angles,
    JumpTimes jt, const int32_t* __restrict__ offsets, const int32_t* __restrict__ batch, JumpNoise noise,
    const float* __restrict__ ve_sigmas, const float* __restrict__ alpha_bars, const float* __restrict__ qmats, int S, int T,
    int absorbing, const int32_t* __restrict__ const_types, const float* __restrict__ fixed_lengths,
    const uint8_t* __restrict__ type_mask, float* __restrict__ lattice, JumpLoopDev loop, const float* __restrict__ betas,
    const float* __restrict__ t_emb_w, const float* __restrict__ embT, int C, int32_t* __restrict__ status,
    const int32_t* __restrict__ length_tie, const uint8_t* __restrict__ len_mask) {
    if ((int)blockIdx.x < B) {
        // ---- lattice part: crystal b ----------------------------------------------------------------------------------
        __shared__ float newlen[3];
        __shared__ float feat[ARREAU_T_EMB_DIM + ARREAU_N_CRYSTAL_FEATS];
        const int b = blockIdx.x;
        int s, t;
        bool bad;
        jump_pair(jt, b, T, s, t, bad);
        if (threadIdx.x == 0 && bad) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
        if constexpr (TIE) {
            // the tied axes jump from the leader's length with the leader's draw (element 3 b): every one computes the same bits
            __shared__ float oldlen[3];
            const int code = length_tie_code(length_tie, len_mask, b, status, threadIdx.x == 0);
            if (threadIdx.x < 3) oldlen[threadIdx.x] = lengths[3 * b + threadIdx.x];
            __syncthreads();
            if (threadIdx.x < 3) {
                const int g = 3 * b + (int)threadIdx.x;
                const bool tied = length_tied(code, threadIdx.x);
                float l = oldlen[threadIdx.x];
                if (fixed_lengths == nullptr) {  // a fixed cell is held (kernel argument: uniform)
                    const float ratio = s > 0 ? alpha_bars[t] / alpha_bars[s] : alpha_bars[t];
                    const int e = tied ? 3 * b : g;
                    const DrawKey dk = length_draw_key(jump_key_src(noise), b);
                    const float z = noise.z_lengths ? noise.z_lengths[e]
                                                    : philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_JUMP_LENGTHS,
                                                                    dk.atom + (tied ? 0u : threadIdx.x), noise.pass);
                    l = sqrtf(ratio) * (tied ? oldlen[0] : l) + sqrtf(1.0f - ratio) * z;
                    lengths[g] = l;
                }
                newlen[threadIdx.x] = l;
            }
        } else
        if (threadIdx.x < 3) {
            const int g = 3 * b + (int)threadIdx.x;
            float l = lengths[g];
            if (fixed_lengths == nullptr) {  // a fixed cell is held (kernel argument: uniform)
                // VP_lattice.forward composed (diffusion_helpers.py:156-163): abar_{t|s} = abar_t / abar_s, abar_0 = 1
                const float ratio = s > 0 ? alpha_bars[t] / alpha_bars[s] : alpha_bars[t];
                const DrawKey dk = length_draw_key(jump_key_src(noise), b);
                const float z = noise.z_lengths ? noise.z_lengths[g]
                                                : philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_JUMP_LENGTHS, dk.atom + threadIdx.x, noise.pass);
                l = sqrtf(ratio) * l + sqrtf(1.0f - ratio) * z;
                lengths[g] = l;
            }
            newlen[threadIdx.x] = l;
        }
        __syncthreads();
        const float* ang = angles + 3 * b;
        if (threadIdx.x == 0) {
            float Lm[9];
            arreau_prep_cell(newlen, ang, Lm);  // lattice_from_params (lattice_helpers.py:55-105)
#pragma unroll
            for (int q = 0; q < 9; ++q) lattice[9 * b + q] = Lm[q];
            if (loop.lattice_ws) {
#pragma unroll
                for (int q = 0; q < 9; ++q) loop.lattice_ws[9 * b + q] = Lm[q];
                // the next step runs at t: the prep-per-step form reads t_next, the form without prep advances t_cur first
                // (t + 1 -> t, through the schedule's "one above" entry in a respaced loop)
                loop.t_next[b] = t;
                loop.t_cur[b] = t + 1;
                if (b == 0) loop.pass[0] = (int32_t)noise.pass;
            }
        }
        if (loop.lattice_ws)  // (kernel argument: uniform) the per-crystal embedding of the step at t (barriers inside)
            arreau_prep_cvec(t, offsets[b + 1] - offsets[b], newlen, ang, betas, t_emb_w, embT, S, C, T, feat, loop.cvec + (size_t)b * C,
                             status);
        return;
    }
    // ---- atom part: one wave per atom -----------------------------------------------------------------------------------
    const int lane = threadIdx.x & 63;
    const int i = ((int)blockIdx.x - B) * 4 + (int)(threadIdx.x >> 6);
    if (i >= N) return;  // wave-uniform; no block-level barrier below
    int lo = 0, hi = B;
    if (batch != nullptr) {
        lo = batch[i];
    } else
    while (hi - lo > 1) {  // crystal of this atom: the 64-ary search of reverse_one_atom
        const int span = hi - lo, step = (span + 63) >> 6;
        const int probe = lo + lane * step;
        const bool le = probe < hi && offsets[probe] <= i;
        const int c = __builtin_popcountll(__ballot(le));
        lo = lo + (c - 1) * step;
        hi = min(lo + step, hi);
    }
    int s, t;
    bool bad;
    jump_pair(jt, lo, T, s, t, bad);  // (flagged by the crystal's workgroup)
    const DrawKey dk = atom_draw_key(jump_key_src(noise), offsets, lo, i);  // (keyed sampling: the crystal's seed, the atom's index in it)
    if (lane < 3) {
        // VE_pbc.forward composed (diffusion_helpers.py:43-47): std sqrt(sig_t^2 - sig_s^2), formed without cancellation
        const float st = ve_sigmas[t], ss = ve_sigmas[s];
        const float sd = sqrtf((st - ss) * (st + ss));
        const size_t g = 3 * (size_t)i + lane;
        const float z = noise.z_frac ? noise.z_frac[g] : philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_JUMP_FRAC, 3u * dk.atom + (uint32_t)lane, noise.pass);
        frac[g] = remainder_one(frac[g] + sd * z);
    }
    // species held by the loop: constant species, known species of a condition (wave-uniform)
    if (const_types != nullptr || (type_mask != nullptr && type_mask[i])) return;
    // D3PM.q_sample (d3pm.py:119-127) from x_s with Qbar_{t-s} = q_mats[t-s-1]: the rule and tie rule of noise_atoms_kernel
    int xs = types[i];
    if ((xs < 0 || xs >= S) && lane == 0) atomicOr(status, ARREAU_STATUS_BAD_TYPE);  // clamped, but flagged
    xs = xs < 0 ? 0 : (xs >= S ? S - 1 : xs);
    const float* qrow = qmats + ((size_t)(t - s - 1) * S + xs) * S;
    const int mask = S - 1;
    const bool have_u = noise.u_types != nullptr;
    float best = -INFINITY;
    int besti = 0x7fffffff;
    for (int c = lane; c < S; c += 64) {
        // absorbing chain: row xs is zero off the diagonal and the mask column (checked at model creation), so those entries are
        // the exact zeros the dense read would give
        const float q = (!absorbing || c == xs || c == mask) ? qrow[c] : 0.0f;
        const uint32_t e = dk.atom * (uint32_t)S + (uint32_t)c;
        const float uu = have_u ? noise.u_types[(size_t)i * S + c] : philox_uniform(dk.seed, (uint32_t)t, ARREAU_DRAW_U_JUMP_TYPES, e, noise.pass);
        const float u = fminf(fmaxf(uu, D3PM_EPS), 1.0f);
        const float val = logf(q + D3PM_EPS) + (-logf(-logf(u)));
        if (val > best) { best = val; besti = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(besti, off, 64);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }  // first index wins ties
    }
    if (lane == 0) types[i] = besti;
}
}  // namespace

int arreau_resampling_check(int32_t passes, int32_t jump_length, const char* who) {
    if (passes < 1 || passes > ARREAU_MAX_RESAMPLE_PASSES) {
        arreau_set_error(std::string(who) + ": resampling passes must lie in 1.." + std::to_string(ARREAU_MAX_RESAMPLE_PASSES));
        return ARREAU_EINVAL;
    }
    if (jump_length < 1) {
        arreau_set_error(std::string(who) + ": the resampling jump length must be >= 1");
        return ARREAU_EINVAL;
    }
    return ARREAU_OK;
}

int arreau_launch_resample_jump(const arreau_model* m, const SampleState& st, const int32_t* d_s, const int32_t* d_t, int s, int t,
                                const int32_t* d_batch, const StepNoiseSrc& noise, uint32_t pass, const SampleConditionDev* cond,
                                const JumpLoopDev* loop, const int32_t* d_length_tie, hipStream_t stream) {
    if (st.B <= 0) return ARREAU_OK;
    const uint8_t* type_mask = (cond && cond->a0 && cond->type_mask) ? cond->type_mask : nullptr;
    const uint8_t* len_mask = (cond && cond->l0 && cond->len_mask) ? cond->len_mask : nullptr;
    const JumpLoopDev lp = loop ? *loop : JumpLoopDev{};
    const unsigned blocks = (unsigned)st.B + (unsigned)((st.N + 3) / 4);
    auto kernel = d_length_tie ? resample_jump_kernel<true> : resample_jump_kernel<false>;
    ARREAU_LAUNCH(kernel, dim3(blocks), dim3(JUMP_THREADS), 0, stream, st.B, st.N, st.frac, st.types, st.lengths, st.angles,
                  JumpTimes{d_s, d_t, s, t}, st.offsets, d_batch, JumpNoise{noise.z_frac, noise.z_lattice, noise.u_types, noise.seed, pass, noise.seeds},
                  m->ve_sigmas, m->vp_alpha_bars, m->qmats, m->S, m->T, m->qmats_absorbing, st.const_types, st.fixed_lengths, type_mask,
                  st.lattice, lp, m->vp_betas, m->t_emb_w, m->embT, m->C, m->status, d_length_tie, len_mask);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

static int resample_jump(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                         const int32_t* d_s, const int32_t* d_t, const int32_t* d_off, int32_t B, int32_t N, const float* d_z_frac,
                         const float* d_z_lengths, const float* d_u_types, const int32_t* d_const_types, const float* d_fixed_lengths,
                         const arreau_sample_condition* cond, float* d_lattice, const int32_t* d_length_tie, void* stream,
                         const char* who) {
    ARREAU_REQUIRE(m && d_frac && d_types && d_lengths && d_angles && d_s && d_t && d_off && d_z_frac && d_z_lengths && d_u_types &&
                       d_lattice, std::string(who) + ": null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, std::string(who) + ": bad size");
    SampleConditionDev c;
    int rc;
    if ((rc = arreau_condition_to_dev(cond, &c))) return rc;
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return arreau_launch_resample_jump(m, st, d_s, d_t, 0, 0, /*d_batch=*/nullptr, StepNoiseSrc{d_z_lengths, d_z_frac, d_u_types, 0}, 0u, &c,
                                       /*loop=*/nullptr, d_length_tie, (hipStream_t)stream);
}

extern "C" int arreau_resample_jump(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                    const int32_t* d_s, const int32_t* d_t, const int32_t* d_off, int32_t B, int32_t N,
                                    const float* d_z_frac, const float* d_z_lengths, const float* d_u_types,
                                    const int32_t* d_const_types, const float* d_fixed_lengths, const arreau_sample_condition* cond,
                                    float* d_lattice, void* stream) {
    return resample_jump(m, d_frac, d_types, d_lengths, d_angles, d_s, d_t, d_off, B, N, d_z_frac, d_z_lengths, d_u_types, d_const_types,
                         d_fixed_lengths, cond, d_lattice, nullptr, stream, "arreau_resample_jump");
}

// Forward noising of a clean state to level t (rules in include/arreau_hip.h, section "Starting the sampler from given crystals"):
// the jump (0, t) of every crystal with the kernel's own Philox draws, pass word 0 -- a word the resampled loop never uses for the
// jump kinds.  Outside a loop: no device timestep, no next step's set-up.
static int noise_state(const char* who, const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                       const int32_t* d_off, int32_t B, int32_t N, int32_t t, uint64_t seed, const int32_t* d_const_types,
                       const float* d_fixed_lengths, float* d_lattice, const int32_t* d_length_tie, const uint64_t* d_crystal_seeds,
                       void* stream) {
    ARREAU_REQUIRE(m && d_frac && d_types && d_lengths && d_angles && d_off && d_lattice, std::string(who) + ": null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, std::string(who) + ": bad size");
    ARREAU_REQUIRE(t >= 1 && t <= m->T, std::string(who) + ": t must lie in 1..T");
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return arreau_launch_resample_jump(m, st, /*d_s=*/nullptr, /*d_t=*/nullptr, 0, t, /*d_batch=*/nullptr,
                                       StepNoiseSrc{.seed = seed, .seeds = d_crystal_seeds}, /*pass=*/0u, /*cond=*/nullptr, /*loop=*/nullptr,
                                       d_length_tie, (hipStream_t)stream);
}

extern "C" int arreau_noise_state(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                  const int32_t* d_off, int32_t B, int32_t N, int32_t t, uint64_t seed, const int32_t* d_const_types,
                                  const float* d_fixed_lengths, float* d_lattice, const int32_t* d_length_tie, void* stream) {
    return noise_state("arreau_noise_state", m, d_frac, d_types, d_lengths, d_angles, d_off, B, N, t, seed, d_const_types, d_fixed_lengths,
                       d_lattice, d_length_tie, nullptr, stream);
}

// Keyed sampling (rules in include/arreau_hip.h): arreau_noise_state with the table of stream seeds; NULL = arreau_noise_state.
extern "C" int arreau_noise_state_keyed(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                        const int32_t* d_off, int32_t B, int32_t N, int32_t t, uint64_t seed,
                                        const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                        const int32_t* d_length_tie, const uint64_t* d_crystal_seeds, void* stream) {
    return noise_state("arreau_noise_state_keyed", m, d_frac, d_types, d_lengths, d_angles, d_off, B, N, t, seed, d_const_types,
                       d_fixed_lengths, d_lattice, d_length_tie, d_crystal_seeds, stream);
}

// arreau_resample_jump with the lattice-system tie of the lengths (rules in include/arreau_hip.h); NULL = arreau_resample_jump.
extern "C" int arreau_resample_jump_tied(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                         const int32_t* d_s, const int32_t* d_t, const int32_t* d_off, int32_t B, int32_t N,
                                         const float* d_z_frac, const float* d_z_lengths, const float* d_u_types,
                                         const int32_t* d_const_types, const float* d_fixed_lengths, const arreau_sample_condition* cond,
                                         float* d_lattice, const int32_t* d_length_tie, void* stream) {
    return resample_jump(m, d_frac, d_types, d_lengths, d_angles, d_s, d_t, d_off, B, N, d_z_frac, d_z_lengths, d_u_types, d_const_types,
                         d_fixed_lengths, cond, d_lattice, d_length_tie, stream, "arreau_resample_jump_tied");
}
