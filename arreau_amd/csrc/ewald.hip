// Ewald electrostatics of a batch of crystals (arreau_crystal_ewald; the rules are written out in include/arreau_hip.h): per
// crystal the energy of the caller's point charges on its sites with its real-space, reciprocal-space, self and background parts,
// per atom the site potential.  The first kernel that walks both spaces: the screen's image walk (crystal_dev.h) for the erfc
// sum, the powder pattern's box walk (xrd_dev.h) for the structure-factor sum.  One launch, one workgroup of four waves per
// crystal, no atomics; needs no arreau_model.
//
// Split of precisions: the displacement and d2 of a pair are the screen's float32 expression bit for bit (crystal_contact_at), the
// cut is on that float32 d2; the reduced phase and its sine and cosine are the powder pattern's float32 (xrd_phase, sincospif);
// everything else -- the cell, alpha, the cuts, r, erfc, exp, every product and every sum -- is float64.
// Order: real space, one wave per atom, lane t adds the entries e = t, t + 64, ... in ascending order, then the butterfly;
// reciprocal space, a thread per box entry of a round of 256 forms S(G), the round's kept entries are compacted in thread order
// (crystal_compact) and thread t adds them one after another to its atoms t, t + 256, ...; the potentials in volts (K times
// the sums) and the energies (1 / 2) sum q phi, one thread in atom order.
// The two parts of the potential meet in global memory (out.potential the real part, out.work the reciprocal part) behind a
// workgroup barrier.
//
// LDS per workgroup: spos, s_x 2 * 3072 B, s_q 1024 B, a round's list (two doubles and three floats) 256 * 28 = 7168 B, the slots
// and the waves' counts 48 B.
#include "internal.h"
#include "xrd_dev.h"
#include <cmath>

namespace {

// what the host derives from arreau_ewald_params (rule 1)
struct ewald_plan {
    double s, alpha;  // sqrt(-ln accuracy); 0: per crystal
    int max_shells, max_index;
};

constexpr double EWALD_PI = 3.14159265358979323846, EWALD_SQRT_PI = 1.77245385090551602730;

// v <- v + shuffle_xor(v, w), w = 32 .. 1, float64: every lane ends with the same bits
__device__ __forceinline__ double ewald_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_ewald_kernel(
    const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets, const float* __restrict__ charges,
    int B, int N, ewald_plan P, arreau_ewald_result out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int first, n;
    float Lm[9];
    int unassigned = 0;
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [&] {
        for (int a = tid; a < n; a += CRYSTAL_THREADS) unassigned |= !isfinite(charges[(size_t)first + a]);
    });
    unassigned = __syncthreads_or(unassigned);

    __shared__ float spos[3 * CRYSTAL_LDS_ATOMS], s_x[3 * CRYSTAL_LDS_ATOMS], s_q[CRYSTAL_LDS_ATOMS];
    __shared__ double s_cre[CRYSTAL_THREADS], s_cim[CRYSTAL_THREADS];
    __shared__ float s_h[CRYSTAL_THREADS], s_k[CRYSTAL_THREADS], s_l[CRYSTAL_THREADS];
    __shared__ int s_slots[CRYSTAL_WAVES];
    __shared__ unsigned long long s_cnt[CRYSTAL_WAVES];

    double* const phi = out.potential + first;  // the real part, at the end the potential
    double* const rec = out.work + first;       // the reciprocal part
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    // a flagged crystal (workgroup-uniform): the reals and the potentials are NaN, the counts 0
    auto blank = [&](int flags) {
        for (int a = tid; a < n; a += CRYSTAL_THREADS) phi[a] = qnan;
        if (tid == 0) {
            out.energy[b] = qnan; out.real[b] = qnan; out.reciprocal[b] = qnan; out.self[b] = qnan; out.background[b] = qnan;
            out.net_charge[b] = qnan; out.alpha[b] = qnan; out.volume[b] = qnan;
            out.n_pairs[b] = 0; out.n_reciprocal[b] = 0; out.flags[b] = flags;
        }
    };
    if (bad) {
        blank(ARREAU_EWALD_NONFINITE);
        return;
    }
    // ---- rules 1 and 2: the cell, alpha and the cuts, the images and the box (every thread computes the same values)
    xrd_cell box;
    double A[9], det;
    if (!xrd_cell_rows(Lm, box, A, det)) {
        blank(ARREAU_EWALD_CELL);
        return;
    }
    if (n == 0) {
        blank(ARREAU_EWALD_EMPTY);
        return;
    }
    const double V = fabs(det);
    const double alpha = P.alpha > 0. ? P.alpha : EWALD_SQRT_PI * cbrt(sqrt((double)n) / V);
    const double r_cut = P.s / alpha, g_cut = alpha * P.s / EWALD_PI;
    crystal_cell cell;
    if (crystal_cell_measure(Lm, (float)r_cut, P.max_shells, cell)) {
        blank(ARREAU_EWALD_CELL);
        return;
    }
    if (!xrd_cell_box(A, det, g_cut, P.max_index, box)) {
        blank(ARREAU_EWALD_RANGE);
        return;
    }
    if (unassigned) {
        blank(ARREAU_EWALD_UNASSIGNED);
        return;
    }
    crystal_cell_images(cell);

    // ---- the atoms: wrapped coordinates and charges, and the Cartesian positions, in LDS when the crystal fits
    const bool staged = n <= CRYSTAL_LDS_ATOMS;
    if (staged) {
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) s_x[a] = crystal_wrap(frac[3 * (size_t)first + a]);
        for (int a = tid; a < n; a += CRYSTAL_THREADS) s_q[a] = charges[(size_t)first + a];
    }
    const crystal_positions position = crystal_stage_positions(spos, frac, Lm, first, n);  // (its barrier covers s_x and s_q)
    const xrd_atoms atoms{s_x, s_q, frac, charges, (size_t)first, staged};
    auto charge = [&](int a) { return (double)(staged ? s_q[a] : charges[(size_t)first + a]); };

    // ---- rule 3: real space.  Wave w owns the atoms w, w + 4, ...; its lanes share the range e = j M + m.
    const float r2 = (float)(r_cut * r_cut);
    const unsigned long long span = (unsigned long long)n * cell.M;
    unsigned long long pairs = 0;
    int overlap = 0;
    for (int a = wave; a < n; a += CRYSTAL_WAVES) {
        const float pix = position(a, 0), piy = position(a, 1), piz = position(a, 2);
        double part = 0.;
        crystal_walk(span, cell.M, (unsigned long long)lane, 64u, [&](unsigned j, unsigned m) {
            if ((int)j == a && m == cell.centre) return;  // the atom itself
            const crystal_contact k = crystal_contact_at(cell, Lm, position, (int)j, m, pix, piy, piz);
            if (!(k.d2 <= r2)) return;
            if (k.d2 == 0.f) {
                overlap = 1;
                return;
            }
            ++pairs;
            const double r = sqrt((double)k.d2);
            part += charge((int)j) * erfc(alpha * r) / r;
        });
        part = ewald_wave_sum(part);
        if (lane == 0) phi[a] = part;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) pairs += __shfl_xor(pairs, off);  // (an integer sum: any order gives the same value)
    if (lane == 0) s_cnt[wave] = pairs;

    // ---- rule 4: reciprocal space.  Thread t owns the atoms t, t + 256, ... and their entry of `rec` throughout.
    for (int a = tid; a < n; a += CRYSTAL_THREADS) rec[a] = 0.;
    double own = 0.;
    const double pref = 2.0 / (EWALD_PI * V), g2_cut = g_cut * g_cut, eta = (EWALD_PI * EWALD_PI) / (alpha * alpha);
    int kept = 0;
    xrd_box_walk(box, [&](bool valid, unsigned uh, unsigned m) {
        const xrd_point pt = xrd_point_at(box, valid, uh, m);
        const bool keep = pt.half && pt.d2 > 0. && pt.d2 <= g2_cut;
        const float hf = (float)pt.h, kf = (float)pt.k, lf = (float)pt.l;
        double re = 0., im = 0.;
        if (keep) {
            for (int a = 0; a < n; ++a) {
                float x, y, z, q;
                atoms(a, x, y, z, q);
                float s, co;
                sincospif(__fmul_rn(2.0f, xrd_phase(hf, kf, lf, x, y, z)), &s, &co);
                re += (double)q * (double)co;
                im += (double)q * (double)s;
            }
        }
        int total;
        const int rank = crystal_compact(keep, lane, wave, s_slots, total);
        if (keep) {
            const double w = pref * (exp(-eta * pt.d2) / pt.d2);
            s_cre[rank] = w * re; s_cim[rank] = w * im;
            s_h[rank] = hf; s_k[rank] = kf; s_l[rank] = lf;
        }
        __syncthreads();  // (also: every thread has read the slots before the next round writes them)
        for (int a = tid; a < n; a += CRYSTAL_THREADS) {
            float x, y, z, q;
            atoms(a, x, y, z, q);
            double acc = staged ? own : rec[a];  // (a staged crystal's thread has one atom: its sum stays in a register)
            for (int e = 0; e < total; ++e) {  // ascending box index
                float s, co;
                sincospif(__fmul_rn(2.0f, xrd_phase(s_h[e], s_k[e], s_l[e], x, y, z)), &s, &co);
                acc += s_cre[e] * (double)co + s_cim[e] * (double)s;
            }
            if (staged) own = acc;
            else rec[a] = acc;
        }
        kept += total;  // (the next round's list is written behind crystal_compact's barrier: every thread has left this loop)
    });

    if (staged && tid < n) rec[tid] = own;

    // ---- rules 5 and 6: the parts meet (the barrier publishes phi, rec and s_cnt); one thread, atom order
    if (__syncthreads_or(overlap)) {
        blank(ARREAU_EWALD_OVERLAP);
        return;
    }
    if (tid == 0) {
        double Q = 0., Qabs = 0.;
        for (int a = 0; a < n; ++a) {
            const double q = charge(a);
            Q = __dadd_rn(Q, q);
            Qabs = __dadd_rn(Qabs, fabs(q));
        }
        // the parts in volts: K times the sums, which are in e / A
        const double k = ARREAU_EWALD_K, self_c = -2.0 * alpha / EWALD_SQRT_PI, bg = __dmul_rn(k, -EWALD_PI * Q / (V * alpha * alpha));
        double e_all = 0., e_real = 0., e_rec = 0., e_self = 0., e_bg = 0.;
        for (int a = 0; a < n; ++a) {
            const double q = charge(a), pr = __dmul_rn(k, phi[a]), pg = __dmul_rn(k, rec[a]), ps = __dmul_rn(k, __dmul_rn(self_c, q));
            const double p = __dadd_rn(__dadd_rn(__dadd_rn(pr, pg), ps), bg);
            phi[a] = p;
            e_all = __dadd_rn(e_all, __dmul_rn(q, p));
            e_real = __dadd_rn(e_real, __dmul_rn(q, pr));
            e_rec = __dadd_rn(e_rec, __dmul_rn(q, pg));
            e_self = __dadd_rn(e_self, __dmul_rn(q, ps));
            e_bg = __dadd_rn(e_bg, __dmul_rn(q, bg));
        }
        out.energy[b] = 0.5 * e_all; out.real[b] = 0.5 * e_real; out.reciprocal[b] = 0.5 * e_rec;  // (e V = eV; the halves are exact)
        out.self[b] = 0.5 * e_self; out.background[b] = 0.5 * e_bg;
        out.net_charge[b] = Q; out.alpha[b] = alpha; out.volume[b] = V;
        unsigned long long total_pairs = 0;
        for (int w = 0; w < CRYSTAL_WAVES; ++w) total_pairs += s_cnt[w];
        out.n_pairs[b] = (int64_t)total_pairs;
        out.n_reciprocal[b] = 2 * kept;
        out.flags[b] = fabs(Q) > 1e-6 * Qabs ? ARREAU_EWALD_CHARGED : 0;
    }
}

}  // namespace

extern "C" int arreau_crystal_ewald(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, const float* d_charges,
                                    int32_t B, int32_t N, const arreau_ewald_params* params, arreau_ewald_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_ewald: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_ewald: bad size");
    const arreau_ewald_params& p = *params;
    ARREAU_REQUIRE(p.accuracy > 0. && p.accuracy < 1., "arreau_crystal_ewald: accuracy must lie in (0, 1)");
    ARREAU_REQUIRE(std::isfinite(p.alpha) && p.alpha >= 0., "arreau_crystal_ewald: alpha must be finite and >= 0");
    ARREAU_REQUIRE(p.max_shells >= 1 && p.max_shells <= ARREAU_SCREEN_MAX_SHELLS, "arreau_crystal_ewald: max_shells must lie in 1..8");
    ARREAU_REQUIRE(p.max_index >= 1 && p.max_index <= ARREAU_XRD_MAX_INDEX, "arreau_crystal_ewald: max_index must lie in 1..127");
    ewald_plan plan;
    plan.s = std::sqrt(-std::log(p.accuracy));
    ARREAU_REQUIRE(std::isfinite(plan.s) && plan.s > 0., "arreau_crystal_ewald: accuracy outside what float64 holds");
    plan.alpha = p.alpha; plan.max_shells = p.max_shells; plan.max_index = p.max_index;
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_charges) || N == 0), "arreau_crystal_ewald: null pointer");
    ARREAU_REQUIRE(out->energy && out->real && out->reciprocal && out->self && out->background && out->net_charge && out->alpha && out->volume &&
                       out->n_pairs && out->n_reciprocal && out->flags && ((out->potential && out->work) || N == 0),
                   "arreau_crystal_ewald: null result array");
    ARREAU_LAUNCH(crystal_ewald_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_lattice, d_crystal_offsets,
                  d_charges, (int)B, (int)N, plan, *out);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
