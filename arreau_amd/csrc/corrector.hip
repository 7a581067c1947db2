// Predictor-corrector sampling: the Langevin corrector move on the fractional coordinates (rule in include/arreau_hip.h,
// section "predictor-corrector sampling").  One 256-thread workgroup per crystal, like reverse_crystal_block:
//   pass 1 strides over the crystal's 3 n components and sums |eps|^2 and |z|^2 over the atoms it moves (wave64 butterfly,
//          then the four wave sums in wave order through LDS -- a fixed order, no float atomics, so eager runs, graph replay and
//          segmented runs give the same bits);
//   pass 2 applies x <- remainder(x - a eps + c z, 1), drawing z again instead of staging it (no size cap on the crystal).
// z comes from the caller's array (arreau_corrector_step) or from Philox (seed, t, kind 5, element, iteration) in the loop
// (256 r + iteration in pass r of a resampled loop: the RESAMPLE instance).
#include <cmath>

#include "update_dev.h"

namespace {
constexpr int CORR_THREADS = 256;

// COND: a position mask is read (known atoms are not moved and not counted).  corrector_kernel<false, ...> reads no mask.
// RESAMPLE: a move of a resampled loop (arreau_sample_loop_resampled) in pass r of a block, r read from the loop's device word
// `pass` (see reverse_kernel); its draws take counter word3 = 256 r + iter.  Without RESAMPLE `pass` is not read.
template <bool COND, bool RESAMPLE>
__global__ __launch_bounds__(CORR_THREADS) void corrector_kernel(float* __restrict__ frac, const int32_t* __restrict__ tstep,
                                                                 const int32_t* __restrict__ offsets, int T,
                                                                 const float* __restrict__ eps, const float* __restrict__ z_frac,
                                                                 uint64_t seed, uint32_t iter, float snr,
                                                                 const float* __restrict__ ve_sigmas,
                                                                 const uint8_t* __restrict__ pos_mask, int32_t* __restrict__ status,
                                                                 const int32_t* __restrict__ pass,
                                                                 const uint64_t* __restrict__ seeds /* keyed sampling, or null */) {
    if constexpr (RESAMPLE) iter += 256u * (uint32_t)pass[0];  // the counter word of pass r
    __shared__ float part[2][CORR_THREADS / 64];
    const int b = blockIdx.x;
    const int t_raw = tstep[b];
    if (threadIdx.x == 0 && (t_raw < 1 || t_raw > T)) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
    const int t = t_raw < 1 ? 1 : (t_raw > T ? T : t_raw);
    const int first = offsets[b], last = offsets[b + 1];
    const size_t g0 = 3 * (size_t)first;
    const int n3 = 3 * (last - first);
    // (the array-or-generator choice is made on the kernel argument itself, as in reverse_one_atom)
    const bool have_z = z_frac != nullptr;
    // keyed sampling (rules in include/arreau_hip.h): the crystal's stream seed, elements counted from its first component
    const bool keyed = seeds != nullptr;  // (kernel argument: uniform)
    const uint64_t dseed = keyed ? seeds[b] : seed;
    const uint32_t e0 = keyed ? 0u : (uint32_t)g0;
    auto draw_z = [&](size_t g) {
        return have_z ? z_frac[g] : philox_normal(dseed, (uint32_t)t, ARREAU_DRAW_Z_CORRECTOR, e0 + (uint32_t)(g - g0), iter);
    };
    float ee = 0.0f, zz = 0.0f;
    for (int c = threadIdx.x; c < n3; c += CORR_THREADS) {
        const size_t g = g0 + c;
        if (COND && pos_mask[g / 3]) continue;
        const float e = eps[g], z = draw_z(g);
        ee = fmaf(e, e, ee);
        zz = fmaf(z, z, zz);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ee += __shfl_xor(ee, off, 64);
        zz += __shfl_xor(zz, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = ee;
        part[1][threadIdx.x >> 6] = zz;
    }
    __syncthreads();
    ee = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    zz = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    // a = 2 r^2 sig^2 q^2, c = 2 r sig^2 q with q = |z| / |eps|: never 1 / sig^2 (the score's own size) at small sig
    const float sig = ve_sigmas[t];
    const float sig2 = sig * sig;
    const float q = sqrtf(zz) / sqrtf(ee);
    const float cz = 2.0f * snr * sig2 * q;
    const float a = cz * snr * q;
    // |eps|^2 of 0 or not finite (also: nothing to move), or coefficients beyond fp32: the crystal is left unmoved
    if (!(ee > 0.0f && isfinite(ee) && isfinite(a) && isfinite(cz))) return;  // (block-uniform)
    for (int c = threadIdx.x; c < n3; c += CORR_THREADS) {
        const size_t g = g0 + c;
        if (COND && pos_mask[g / 3]) continue;
        const float d = cz * draw_z(g) - a * eps[g];
        frac[g] = remainder_one(frac[g] + d);
    }
}

}  // namespace

int arreau_corrector_check(int32_t steps, float snr, const char* who) {
    if (steps < 0 || steps > ARREAU_MAX_CORRECTOR_STEPS) {
        arreau_set_error(std::string(who) + ": corrector steps must lie in 0.." + std::to_string(ARREAU_MAX_CORRECTOR_STEPS));
        return ARREAU_EINVAL;
    }
    if (steps > 0 && !(snr > 0.0f && std::isfinite(snr))) {
        arreau_set_error(std::string(who) + ": the corrector's snr must be finite and > 0");
        return ARREAU_EINVAL;
    }
    return ARREAU_OK;
}

int arreau_launch_corrector(const arreau_model* m, const SampleState& st, const int32_t* d_t, const float* d_eps, const float* d_z_frac,
                            uint64_t seed, uint32_t iter, const StepOptions& opt, hipStream_t s) {
    if (st.B <= 0 || st.N <= 0) return ARREAU_OK;
    const uint8_t* mask = (opt.cond && opt.cond->x0 && opt.cond->pos_mask) ? opt.cond->pos_mask : nullptr;
    auto kernel = mask ? (opt.pass ? corrector_kernel<true, true> : corrector_kernel<true, false>)
                       : (opt.pass ? corrector_kernel<false, true> : corrector_kernel<false, false>);
    ARREAU_LAUNCH(kernel, dim3(st.B), dim3(CORR_THREADS), 0, s, st.frac, d_t, st.offsets, m->T, d_eps, d_z_frac, seed, iter, opt.corr.snr,
                  m->ve_sigmas, mask, m->status, opt.pass, opt.crystal_seeds);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

extern "C" int arreau_corrector_step(const arreau_model* m, float* d_frac, const int32_t* d_t, const int32_t* d_off, int32_t B,
                                     int32_t N, const float* d_eps, const float* d_z_frac, float snr,
                                     const arreau_sample_condition* condition, void* stream) {
    ARREAU_REQUIRE(m && d_frac && d_t && d_off && d_eps && d_z_frac, "arreau_corrector_step: null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, "arreau_corrector_step: bad size");
    int rc;
    if ((rc = arreau_corrector_check(1, snr, "arreau_corrector_step"))) return rc;
    SampleConditionDev c;
    if ((rc = arreau_condition_to_dev(condition, &c))) return rc;
    return arreau_launch_corrector(m, SampleState{.frac = d_frac, .offsets = d_off, .B = B, .N = N}, d_t, d_eps, d_z_frac, 0, 0u,
                                   StepOptions{.cond = &c, .corr = {1, snr}}, (hipStream_t)stream);
}
