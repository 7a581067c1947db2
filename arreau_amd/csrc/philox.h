// Counter-based random numbers for the in-kernel noise of the sampling loop: Philox4x32-10 (Salmon et al., SC'11;
// checked against the Random123 known-answer vectors in tests/test_cabi_exports.py via arreau_philox_fill).
// One call per drawn element, keyed by what the number is FOR, never by which thread draws it:
//     counter = (element index, timestep, draw kind, word3),  key = the 64-bit seed
// (word3 = 0 for every draw but the corrector's, whose iteration index it holds, and those of a resampled loop: pass r of a block
// adds 256 r, and the jump in front of pass r draws with word3 = r)
// so the noise of (seed, timestep, kind, element) is the same whatever the batch composition, launch geometry or
// replay mechanism (eager loop or hipGraph).  The three draws of a step (diffusion_helpers.py:193-197, :79; d3pm.py:206):
#pragma once
#include <stdint.h>

#define ARREAU_DRAW_Z_LATTICE 0u  // randn [B,3]
#define ARREAU_DRAW_Z_FRAC 1u     // randn [N,3]
#define ARREAU_DRAW_U_TYPES 2u    // rand  [N,S]
// conditioned sampling (arreau_sample_loop_conditioned): the forward-noising draws of the known components
#define ARREAU_DRAW_Z_KNOWN_FRAC 3u     // randn [N,3]  VE_pbc.forward of a known position (diffusion_helpers.py:43-47)
#define ARREAU_DRAW_Z_KNOWN_LENGTHS 4u  // randn [B,3]  VP_lattice.forward of a known length (diffusion_helpers.py:156-163)
// predictor-corrector sampling (arreau_sample_loop_corrected): the Langevin noise of corrector iteration j, counter word3 = j
#define ARREAU_DRAW_Z_CORRECTOR 5u      // randn [N,3]
// RePaint resampling (arreau_sample_loop_resampled, arreau_resample_jump): the forward jump from a block's bottom s to its top t,
// keyed by t, word3 = the pass r the jump precedes
#define ARREAU_DRAW_Z_JUMP_FRAC 6u      // randn [N,3]  VE_pbc.forward s -> t of the positions
#define ARREAU_DRAW_Z_JUMP_LENGTHS 7u   // randn [B,3]  VP_lattice.forward s -> t of the lengths
#define ARREAU_DRAW_U_JUMP_TYPES 8u     // rand  [N,S]  D3PM.q_sample s -> t of the species
// keyed forward noising of the training / validation loss (arreau_diffusion_noise_keyed): word3 = the crystal's id, the element
// is counted within the crystal, so a crystal's draws do not depend on the batch around it
#define ARREAU_DRAW_U_TIMESTEP 9u        // rand  [1]    the timestep uniform: element 0 at counter timestep 0
#define ARREAU_DRAW_Z_TRAIN_FRAC 10u     // randn [n,3]  element 3 a + d, a the atom's index within its crystal
#define ARREAU_DRAW_U_TRAIN_TYPES 11u    // rand  [n,S]  element a S + s
#define ARREAU_DRAW_Z_TRAIN_LENGTHS 12u  // randn [3]    element d
// keyed sampling (arreau_sample_loop_keyed; rules in include/arreau_hip.h): the initial state of a crystal, at counter timestep 0
// under the crystal's stream seed, elements counted within the crystal
#define ARREAU_DRAW_Z_INIT_LENGTHS 13u   // randn [3]    element d
#define ARREAU_DRAW_Z_INIT_FRAC 14u      // randn [n,3]  element 3 a + d
#define ARREAU_DRAW_U_INIT_ANGLES 15u    // rand  [k]    element j: the j-th uniform the crystal's angle draw consumes
// the counter tag of the stream seed itself: words 0 and 1 of philox4x32_10((key lo, key hi, TAG, 0), seed) (host, exact integers)
#define ARREAU_STREAM_SEED_TAG 0x4B455953u  // "KEYS"

struct Philox4 { uint32_t x[4]; };

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// uniform in [0, 1) with 24 random bits (every value exactly representable; 1.0 cannot occur)
__host__ __device__ inline float philox_uniform(uint64_t seed, uint32_t timestep, uint32_t kind, uint32_t element, uint32_t word3 = 0u) {
    const Philox4 r = philox4x32_10(element, timestep, kind, word3, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(r.x[0] >> 8) * (1.0f / 16777216.0f);
}

// keyed sampling, rule 1: the stream seed of (seed, key), 0 <= key < 2^63
__host__ __device__ inline uint64_t arreau_stream_seed(uint64_t seed, uint64_t key) {
    const Philox4 r = philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), ARREAU_STREAM_SEED_TAG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (uint64_t)r.x[0] | ((uint64_t)r.x[1] << 32);
}

#ifdef __HIPCC__
// standard normal by Box-Muller from two words of one Philox call: u1 in (0, 1], u2 in [0, 1)
__device__ inline float philox_normal(uint64_t seed, uint32_t timestep, uint32_t kind, uint32_t element, uint32_t word3 = 0u) {
    const Philox4 r = philox4x32_10(element, timestep, kind, word3, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = ((float)(r.x[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(r.x[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}
#endif
