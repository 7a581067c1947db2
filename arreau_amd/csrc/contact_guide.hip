// Contact guidance of the sampling step (arreau_launch_contact_guide, arreau_contact_guidance_step; the rules are written out in
// include/arreau_hip.h, section "contact guidance"): the gradient of the penalty U = 1/2 sum 1/2 (d0 - d)^2 over every contact
// shorter than d0, found by the screen's exact image search, preconditioned by the cell and added to the network's eps in place.
// One launch, one workgroup of four waves per crystal, one wave per atom, no float atomics: lane l of atom i's wave adds the
// contacts it meets at e = l, l + 64, ... of the range e = j M + m, the 64 partial sums are folded by the butterfly xor 32 .. 1
// (every lane ends with the same bits), a wave adds its atoms' energies in ascending i and the four waves are added in wave
// order through LDS.  Nothing depends on the grid, on the crystal's place in the batch or on eager versus replay.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

namespace {

__global__ __launch_bounds__(CRYSTAL_THREADS) void contact_guide_kernel(
    const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ tstep, int B, int N, int T, const float* __restrict__ ve_sigmas, float d0, float md2 /* d0^2 */,
    float weight, int max_shells, float* __restrict__ eps, float* __restrict__ o_energy, int32_t* __restrict__ o_contacts,
    int32_t* __restrict__ o_flags, int32_t* __restrict__ status) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float spos[3 * CRYSTAL_LDS_ATOMS];
    __shared__ float s_u[CRYSTAL_WAVES];
    __shared__ int s_cnt[CRYSTAL_WAVES];
    __shared__ int s_zero[CRYSTAL_WAVES];

    // ---- the cell (every thread computes the same values); a flagged crystal keeps its eps
    crystal_cell cell;
    const bool cell_bad = bad || crystal_cell_measure(Lm, d0, max_shells, cell);
    if (bad || cell_bad || n == 0) {  // (workgroup-uniform)
        if (tid == 0) {
            if (o_energy) o_energy[b] = 0.0f;
            if (o_contacts) o_contacts[b] = 0;
            if (o_flags) o_flags[b] = bad ? ARREAU_GUIDE_NONFINITE : ((cell_bad ? ARREAU_GUIDE_CELL : 0) | (n == 0 ? ARREAU_GUIDE_EMPTY : 0));
        }
        return;
    }
    crystal_cell_images(cell);

    // g = D L^-1: the rows c_k of the adjugate and the signed volume
    float c0[3], c1[3], c2[3];
    cross_rn(Lm + 3, Lm + 6, c0);
    cross_rn(Lm + 6, Lm, c1);
    cross_rn(Lm, Lm + 3, c2);
    const float vol = dot3_rn(Lm[0], Lm[1], Lm[2], c0[0], c0[1], c0[2]);

    const int t_raw = tstep[b];
    if (tid == 0 && (t_raw < 1 || t_raw > T)) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
    const int t = t_raw < 1 ? 1 : (t_raw > T ? T : t_raw);
    const float sig = ve_sigmas[t];
    const float coef = __fdiv_rn(weight, __fmul_rn(sig, sig));

    const crystal_positions position = crystal_stage_positions(spos, frac, Lm, first, n);

    // ---- one wave per atom: i = wave, wave + 4, ...
    float u_wave = 0.0f;  // the wave's energies, ascending i (the same bits in every lane)
    int cnt = 0, zero = 0;  // this lane's ordered contacts and skipped overlaps
    for (int i = wave; i < n; i += CRYSTAL_WAVES) {
        const float pix = position(i, 0), piy = position(i, 1), piz = position(i, 2);
        float Dx = 0.0f, Dy = 0.0f, Dz = 0.0f, u = 0.0f;
        crystal_walk((unsigned long long)n * cell.M, cell.M, (unsigned)lane, 64u, [&](unsigned j, unsigned m) {
            if ((int)j == i) return;  // self images exert no force on positions
            const crystal_contact k = crystal_contact_at(cell, Lm, position, (int)j, m, pix, piy, piz);
            if (!(k.d2 < md2)) return;
            if (k.d2 == 0.0f) { zero = 1; return; }
            const float d = sqrtf(k.d2);  // correctly rounded
            const float gap = __fsub_rn(d0, d);
            const float f = __fdiv_rn(gap, d);
            Dx = __fadd_rn(Dx, __fmul_rn(f, k.dx));
            Dy = __fadd_rn(Dy, __fmul_rn(f, k.dy));
            Dz = __fadd_rn(Dz, __fmul_rn(f, k.dz));
            u = __fadd_rn(u, __fmul_rn(gap, gap));
            ++cnt;
        });
        Dx = crystal_wave_sum(Dx); Dy = crystal_wave_sum(Dy); Dz = crystal_wave_sum(Dz);
        u_wave = __fadd_rn(u_wave, crystal_wave_sum(u));
        if (lane < 3) {  // g_k = (D . c_k) / V, eps' = eps + (w / sig^2) g_k
            const float* ck = lane == 0 ? c0 : (lane == 1 ? c1 : c2);
            const float g = __fdiv_rn(dot3_rn(Dx, Dy, Dz, ck[0], ck[1], ck[2]), vol);
            const size_t at = 3 * ((size_t)first + i) + lane;  // first + i < N: the offsets are clamped
            eps[at] = __fadd_rn(eps[at], __fmul_rn(coef, g));
        }
    }

    // ---- the crystal's diagnostics: integer sums in any order, the four energies in wave order
    if (o_energy == nullptr && o_contacts == nullptr && o_flags == nullptr) return;  // (kernel arguments: uniform)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        zero |= __shfl_xor(zero, off, 64);
    }
    if (lane == 0) { s_u[wave] = u_wave; s_cnt[wave] = cnt; s_zero[wave] = zero; }
    __syncthreads();
    if (tid == 0) {
        const float usum = __fadd_rn(__fadd_rn(__fadd_rn(s_u[0], s_u[1]), s_u[2]), s_u[3]);
        if (o_energy) o_energy[b] = __fmul_rn(0.25f, usum);
        if (o_contacts) o_contacts[b] = (s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]) / 2;
        if (o_flags) o_flags[b] = (s_zero[0] | s_zero[1] | s_zero[2] | s_zero[3]) ? ARREAU_GUIDE_OVERLAP : 0;
    }
}

}  // namespace

int arreau_contact_guidance_check(const arreau_contact_guidance* g, const char* who) {
    ARREAU_REQUIRE(g != nullptr, std::string(who) + ": null contact guidance");
    ARREAU_REQUIRE(std::isfinite(g->min_distance) && g->min_distance > 0.f, std::string(who) + ": the guidance's min_distance must be finite and > 0");
    ARREAU_REQUIRE(std::isfinite(g->weight) && g->weight >= 0.f, std::string(who) + ": the guidance's weight must be finite and >= 0");
    ARREAU_REQUIRE(g->max_shells >= 1 && g->max_shells <= ARREAU_SCREEN_MAX_SHELLS, std::string(who) + ": the guidance's max_shells must lie in 1..8");
    return ARREAU_OK;
}

int arreau_launch_contact_guide(const arreau_model* m, const SampleState& st, const int32_t* d_t, const float* d_lattice, float* d_eps,
                                const arreau_contact_guidance& opt, hipStream_t s) {
    if (st.B <= 0) return ARREAU_OK;  // (N == 0: the crystals are EMPTY, which the diagnostics say)
    const float md2 = (float)((double)opt.min_distance * (double)opt.min_distance);
    ARREAU_LAUNCH(contact_guide_kernel, dim3((unsigned)st.B), dim3(CRYSTAL_THREADS), 0, s, st.frac, d_lattice, st.offsets, d_t, st.B, st.N,
                  m->T, m->ve_sigmas, opt.min_distance, md2, opt.weight, (int)opt.max_shells, d_eps, opt.d_energy, opt.d_contacts,
                  opt.d_flags, m->status);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

extern "C" int arreau_contact_guidance_step(const arreau_model* m, const float* d_frac, const float* d_lattice, const int32_t* d_t,
                                            const int32_t* d_off, int32_t B, int32_t N, float* d_eps,
                                            const arreau_contact_guidance* guidance, void* stream) {
    int rc;
    if ((rc = arreau_contact_guidance_check(guidance, "arreau_contact_guidance_step"))) return rc;
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_contact_guidance_step: bad size");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(m && d_lattice && d_t && d_off && ((d_frac && d_eps) || N == 0), "arreau_contact_guidance_step: null pointer");
    return arreau_launch_contact_guide(m, SampleState{.frac = const_cast<float*>(d_frac), .offsets = d_off, .B = B, .N = N}, d_t, d_lattice,
                                       d_eps, *guidance, (hipStream_t)stream);
}
