// XRD guidance of the sampling step (arreau_launch_xrd_guide, arreau_xrd_guidance_step; the rules are written out in
// include/arreau_hip.h, section "XRD guidance"): the gradient of the cosine distance between the crystal's powder pattern and a
// target pattern with respect to every atom's position, preconditioned by the cell and added to the network's eps in place.  One
// launch, one workgroup of four waves per crystal, no float atomics.  Two walks of reciprocal space (xrd_dev.h, shared with
// xrd.hip): the forward walk leaves the pattern P in LDS -- arreau_crystal_xrd's bits --; the distance and its derivative u with
// respect to the pattern follow in float64 and u replaces P; the second walk forms the same reflections again, compacts a round's
// kept ones into LDS, thread r takes list entry r's coefficient kappa * sum_p u(p) G(p) over its window, and then wave v adds the
// round's terms to its atoms v, v + 4, ...: lane l takes list entries l, l + 64, ..., the 64 partial sums are folded by the
// butterfly xor 32 .. 1 and lane 0 adds the round's sum to the atom's float64 accumulator in LDS.  Nothing depends on the grid, on
// the crystal's place in the batch or on eager versus replay.
//
// Per (atom, kept reflection) one sincospif of the float32 reduced phase, as in the forward structure factor; everything after it
// -- Re F sin - Im F cos, the coefficient, the three components of G, the sums -- is float64.  A crystal of more than 256 atoms is
// flagged LARGE and left alone: the accumulators and the staged atoms are LDS-resident.
//
// LDS per workgroup: 43376 B as the compiler reports it (group_segment_fixed_size), with 146 VGPRs and no scratch: three waves per
// SIMD by registers.  What the bytes
// are: pattern / u 4096 floats 16384 B, wrapped coordinates 3072 B, amplitudes 1024 B, a round's list (2 theta and coefficient as
// double, G as three doubles, amplitude, Re F, Im F, packed hkl, first and last grid point) 256 * 64 = 16384 B, the accumulators
// 3 * 256 doubles 6144 B, 4 slots and 12 doubles of partial sums.
#include "internal.h"
#include "xrd_dev.h"
#include <cmath>

namespace {

struct xrd_guide_args {
    const float* target;         // [B, n_points]
    const float* class_weights;  // [S] or null
    const float* atom_weights;   // [N] or null (exactly one of the two)
    const int32_t* types;        // [N] (read with class_weights)
    int S;
    float weight;
    const int32_t* tstep;        // [B]
    int T;
    const float* ve_sigmas;      // [T+1]
    float* eps;                  // [N,3] in place
    float* gradient;             // [N,3] or null: g itself
    float* o_distance;
    int32_t* o_reflections;
    int32_t* o_flags;
    int32_t* status;
};

// three float64 sums over the workgroup in a fixed order: the butterfly xor 32 .. 1 within a wave, then the waves in wave order.
// One barrier; s_red are 3 * CRYSTAL_WAVES doubles the caller leaves alone until every thread has returned.
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, int lane, int wave, double* s_red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); c += __shfl_xor(c, off, 64);
    }
    if (lane == 0) { s_red[3 * wave] = a; s_red[3 * wave + 1] = b; s_red[3 * wave + 2] = c; }
    __syncthreads();
    a = s_red[0]; b = s_red[1]; c = s_red[2];
#pragma unroll
    for (int w = 1; w < CRYSTAL_WAVES; ++w) { a += s_red[3 * w]; b += s_red[3 * w + 1]; c += s_red[3 * w + 2]; }
}

__global__ __launch_bounds__(CRYSTAL_THREADS) void xrd_guide_kernel(
    const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets, int B, int N, xrd_plan P,
    xrd_guide_args g) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int first, n;
    float Lm[9];
    // the amplitude of atom a: its own, or that of its current class (a class outside 0..S-1 does not scatter)
    auto amplitude = [&](int a) -> float {
        const size_t at = (size_t)first + a;
        if (g.atom_weights) return g.atom_weights[at];
        const int c = g.types[at];
        return c >= 0 && c < g.S ? g.class_weights[c] : 0.0f;
    };
    int wbad = 0;
    bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [&] {
        for (int a = tid; a < n; a += CRYSTAL_THREADS) wbad |= !isfinite(amplitude(a));
    });
    bad |= __syncthreads_or(wbad) != 0;

    __shared__ float s_pat[ARREAU_XRD_MAX_POINTS];  // P, then u
    __shared__ float s_x[3 * CRYSTAL_LDS_ATOMS], s_w[CRYSTAL_LDS_ATOMS];
    __shared__ double s_tt[CRYSTAL_THREADS], s_coef[CRYSTAL_THREADS], s_g[3 * CRYSTAL_THREADS];
    __shared__ float s_amp[CRYSTAL_THREADS], s_re[CRYSTAL_THREADS], s_im[CRYSTAL_THREADS];
    __shared__ int s_lo[CRYSTAL_THREADS], s_hi[CRYSTAL_THREADS], s_hkl[CRYSTAL_THREADS];
    __shared__ double s_acc[3 * CRYSTAL_LDS_ATOMS];
    __shared__ double s_red[3 * CRYSTAL_WAVES];
    __shared__ int s_slots[CRYSTAL_WAVES];

    const float qnan = __int_as_float(0x7fc00000);
    // a flagged crystal (workgroup-uniform): its eps stays as it is, g = 0, the distance is NaN, the count 0
    auto skip = [&](int flags) {
        if (g.gradient)
            for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) g.gradient[3 * (size_t)first + a] = 0.0f;
        if (tid == 0) {
            if (g.o_distance) g.o_distance[b] = qnan;
            if (g.o_reflections) g.o_reflections[b] = 0;
            if (g.o_flags) g.o_flags[b] = flags;
        }
    };
    if (bad) {
        skip(ARREAU_XRD_NONFINITE);
        return;
    }
    xrd_cell cell;
    const int cell_flag = xrd_cell_measure(Lm, n, P, cell);
    if (cell_flag) {
        skip(cell_flag);
        return;
    }
    if (n > CRYSTAL_LDS_ATOMS) {
        skip(ARREAU_XGUIDE_LARGE);
        return;
    }
    // ---- the target row: finite, not negative, not all zero
    const float* const q_row = g.target + (size_t)b * P.n_points;
    int q_bad = 0, q_some = 0;
    for (int p = tid; p < P.n_points; p += CRYSTAL_THREADS) {
        const float q = q_row[p];
        q_bad |= !isfinite(q) || q < 0.0f;
        q_some |= q > 0.0f;
    }
    q_bad = __syncthreads_or(q_bad);
    q_some = __syncthreads_or(q_some);
    if (q_bad || !q_some) {
        skip(ARREAU_XGUIDE_NO_TARGET);
        return;
    }

    // ---- rule 1: the pattern, by the xrd launch's walk on the staged atoms (n <= 256)
    for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) {
        s_x[a] = crystal_wrap(frac[3 * (size_t)first + a]);
        s_acc[a] = 0.0;
    }
    for (int a = tid; a < n; a += CRYSTAL_THREADS) s_w[a] = amplitude(a);
    for (int p = tid; p < P.n_points; p += CRYSTAL_THREADS) s_pat[p] = 0.f;
    __syncthreads();
    const xrd_atoms atoms{s_x, s_w, frac, nullptr, (size_t)first, true};
    const int kept = xrd_pattern_walk(P, cell, n, atoms, s_pat, xrd_round_lds{s_tt, s_amp, s_lo, s_hi, s_slots});

    // ---- rule 2: the distance; float64 sums of this thread's points p = tid (mod 256) in ascending order, then block_sum3
    double pq = 0., pp = 0., qq = 0.;
    for (int p = tid; p < P.n_points; p += CRYSTAL_THREADS) {
        const double x = (double)s_pat[p], q = (double)q_row[p];
        pq += x * q; pp += x * x; qq += q * q;
    }
    block_sum3(pq, pp, qq, lane, wave, s_red);
    if (!(pp > 0.) || !isfinite(pp)) {  // nothing scatters in range (or the pattern left float64)
        skip(ARREAU_XGUIDE_DARK);
        return;
    }
    const double inv_norms = 1.0 / (sqrt(pp) * sqrt(qq));
    const double dist = 0.5 * (1.0 - pq * inv_norms);
    // ---- rule 3: u = -(1/2) (Q / (|P||Q|) - (P.Q) P / (|P|^3 |Q|)) over P, this thread's own points
    const double ratio = pq / pp;
    for (int p = tid; p < P.n_points; p += CRYSTAL_THREADS)
        s_pat[p] = (float)(-0.5 * inv_norms * ((double)q_row[p] - ratio * (double)s_pat[p]));
    __syncthreads();

    // ---- rules 4 and 5: the second walk
    const double inv_sigma = 1.0 / P.sigma;
    xrd_box_walk(cell, [&](bool valid, unsigned uh, unsigned m) {
        const xrd_reflection r = xrd_reflection_at(P, cell, n, atoms, valid, uh, m);
        int total;
        const int rank = crystal_compact(r.keep, lane, wave, s_slots, total);
        if (r.keep) {
            s_tt[rank] = r.tt; s_lo[rank] = r.lo; s_hi[rank] = r.hi; s_re[rank] = r.re; s_im[rank] = r.im; s_coef[rank] = r.kappa;
            s_g[3 * rank] = r.gx; s_g[3 * rank + 1] = r.gy; s_g[3 * rank + 2] = r.gz;
            s_hkl[rank] = r.h | ((r.k + 128) << 8) | ((r.l + 128) << 16);  // h in 0..127, k and l in -127..127
        }
        __syncthreads();  // (also: every thread has read the slots before the next round writes them)
        // thread e takes list entry e: c = sum over its window of u(p) G(p), ascending p; the coefficient kappa c
        if (tid < total) {
            const double te = s_tt[tid];
            const int ehi = s_hi[tid];
            double c = 0.;
            for (int p = s_lo[tid]; p <= ehi; ++p) {
                float G;
                if (xrd_gaussian(P, p, te, inv_sigma, G)) c += (double)s_pat[p] * (double)G;
            }
            s_coef[tid] *= c;
        }
        __syncthreads();
        // wave v owns atoms v, v + 4, ...; lane l takes entries l, l + 64, ...
        for (int a = wave; a < n; a += CRYSTAL_WAVES) {
            const float x = s_x[3 * a], y = s_x[3 * a + 1], z = s_x[3 * a + 2];
            double ax = 0., ay = 0., az = 0.;
            for (int e = lane; e < total; e += 64) {
                const int code = s_hkl[e];
                const float hf = (float)(code & 255), kf = (float)(((code >> 8) & 255) - 128), lf = (float)(((code >> 16) & 255) - 128);
                float s, co;
                sincospif(__fmul_rn(2.0f, xrd_phase(hf, kf, lf, x, y, z)), &s, &co);
                const double f = s_coef[e] * ((double)s_re[e] * (double)s - (double)s_im[e] * (double)co);
                ax += f * s_g[3 * e]; ay += f * s_g[3 * e + 1]; az += f * s_g[3 * e + 2];
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                ax += __shfl_xor(ax, off, 64); ay += __shfl_xor(ay, off, 64); az += __shfl_xor(az, off, 64);
            }
            if (lane == 0) { s_acc[3 * a] += ax; s_acc[3 * a + 1] += ay; s_acc[3 * a + 2] += az; }
        }
        // (the next round writes the list after the barrier of its crystal_compact, the coefficients after one more)
    });
    __syncthreads();

    // ---- rules 5 and 6: D_a = -4 pi w_a (the sum), g_a = D_a L^-1, eps' = eps + (w / sigma_t^2) g
    const int t_raw = g.tstep[b];
    if (tid == 0 && (t_raw < 1 || t_raw > g.T)) atomicOr(g.status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
    const int t = t_raw < 1 ? 1 : (t_raw > g.T ? g.T : t_raw);
    const float sig = g.ve_sigmas[t];
    const float coef = __fdiv_rn(g.weight, __fmul_rn(sig, sig));
    for (int a = tid; a < n; a += CRYSTAL_THREADS) {
        const double ww = -12.56637061435917295385 * (double)s_w[a];
        const double Dx = ww * s_acc[3 * a], Dy = ww * s_acc[3 * a + 1], Dz = ww * s_acc[3 * a + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gk = (float)((Dx * cell.R[3 * k] + Dy * cell.R[3 * k + 1]) + Dz * cell.R[3 * k + 2]);
            const size_t at = 3 * ((size_t)first + a) + k;  // first + a < N: the offsets are clamped
            if (g.gradient) g.gradient[at] = gk;
            g.eps[at] = __fadd_rn(g.eps[at], __fmul_rn(coef, gk));
        }
    }
    if (tid == 0) {
        if (g.o_distance) g.o_distance[b] = (float)dist;
        if (g.o_reflections) g.o_reflections[b] = 2 * kept;
        if (g.o_flags) g.o_flags[b] = 0;
    }
}

}  // namespace

int arreau_xrd_guidance_check(const arreau_xrd_guidance* g, const char* who, bool step_export) {
    const std::string name(who);
    ARREAU_REQUIRE(g != nullptr, name + ": null xrd guidance");
    xrd_plan plan;
    int rc;
    if ((rc = arreau_xrd_plan_of(&g->params, (name + ": the xrd guidance").c_str(), &plan))) return rc;
    ARREAU_REQUIRE(std::isfinite(g->weight) && g->weight >= 0.f, name + ": the xrd guidance's weight must be finite and >= 0");
    ARREAU_REQUIRE(g->d_target != nullptr, name + ": the xrd guidance needs its target patterns");
    ARREAU_REQUIRE((g->d_class_weights != nullptr) != (g->d_atom_weights != nullptr),
                   name + ": the xrd guidance takes exactly one of class weights and atom weights");
    ARREAU_REQUIRE(step_export || g->d_atom_weights == nullptr, name + ": the xrd guidance of a loop takes class weights (atom weights: the step export)");
    return ARREAU_OK;
}

int arreau_launch_xrd_guide(const arreau_model* m, const SampleState& st, const int32_t* d_t, const float* d_lattice, float* d_eps,
                            const arreau_xrd_guidance& opt, float* d_gradient, hipStream_t s) {
    if (st.B <= 0) return ARREAU_OK;  // (N == 0: the crystals are EMPTY, which the diagnostics say)
    xrd_plan plan;
    int rc;
    if ((rc = arreau_xrd_plan_of(&opt.params, "xrd guidance", &plan))) return rc;
    const xrd_guide_args args{opt.d_target, opt.d_class_weights, opt.d_atom_weights, st.types, m->S, opt.weight, d_t, m->T, m->ve_sigmas,
                              d_eps, d_gradient, opt.d_distance, opt.d_reflections, opt.d_flags, m->status};
    ARREAU_LAUNCH(xrd_guide_kernel, dim3((unsigned)st.B), dim3(CRYSTAL_THREADS), 0, s, st.frac, d_lattice, st.offsets, st.B, st.N, plan, args);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

extern "C" int arreau_xrd_guidance_step(const arreau_model* m, const float* d_frac, const int32_t* d_types, const float* d_lattice,
                                        const int32_t* d_t, const int32_t* d_off, int32_t B, int32_t N, float* d_eps,
                                        const arreau_xrd_guidance* guidance, float* d_gradient, void* stream) {
    int rc;
    if ((rc = arreau_xrd_guidance_check(guidance, "arreau_xrd_guidance_step", true))) return rc;
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_xrd_guidance_step: bad size");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(m && d_lattice && d_t && d_off && ((d_frac && d_eps && (d_types || guidance->d_atom_weights)) || N == 0),
                   "arreau_xrd_guidance_step: null pointer");
    return arreau_launch_xrd_guide(m, SampleState{.frac = const_cast<float*>(d_frac), .types = const_cast<int32_t*>(d_types), .offsets = d_off,
                                                  .B = B, .N = N},
                                   d_t, d_lattice, d_eps, *guidance, d_gradient, (hipStream_t)stream);
}
