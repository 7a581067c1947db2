// Powder X-ray diffraction patterns of a batch of crystals (arreau_crystal_xrd; the rules are written out in include/arreau_hip.h):
// per crystal the structure-factor sum over the reciprocal-lattice points of one half space inside the 2 theta range, each
// reflection's Lorentz-polarisation-weighted intensity, and the pattern -- the reflections as Gaussians on a fixed 2 theta grid.
// The first per-crystal kernel that walks reciprocal space: the flat range it deals to its threads (crystal_walk_chunks) is the
// box index e = (h W_2 + (k + H_2)) W_3 + (l + H_3), not an image index.  One launch, one workgroup of four waves per crystal, a
// thread per reflection of a round of 256 box entries, no atomics; needs no arreau_model.
//
// Per reflection d*^2, the 2 theta cut, theta = asin, the Lorentz-polarisation factor and the Debye-Waller factor are float64 from
// the float32 cell taken as exact (one asin and one sqrt per KEPT reflection, nothing per atom); the atom sum is float32 in atom
// order, the phase reduced in revolutions (t - rint(t)) before sincospif; the Gaussians are float32 of a float64 difference g - 2
// theta_hkl.  A round's kept reflections are compacted in thread order (crystal_compact) and added one after another; thread t
// owns the grid points p = t (mod 256) throughout, so every point receives its terms in ascending box index whatever the launch
// or the batch, and the pattern needs no barrier of its own.
//
// LDS per workgroup: 25888 B as the compiler reports it (group_segment_fixed_size), with 123 VGPRs and no scratch: four waves per
// SIMD by registers.  What the bytes are: pattern 4096 floats 16384 B, wrapped coordinates 3 * 256 floats 3072 B, weights 1024 B,
// a round's list (2 theta as double, amplitude, first and last grid point) 256 * 20 = 5120 B, 8 words of slots and partial sums:
// 25632 B; the rest is alignment.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

namespace {

// what the host derives from arreau_xrd_params in float64, once per launch (rule 1)
struct xrd_plan {
    double wavelength, g0, g1, step;  // the grid: g_p = g0 + p step, g_{n-1} = g1
    double sigma, six_sigma, norm;    // degrees; norm = 1 / (sigma sqrt(2 pi))
    double dlo2, dhi2, dhi;           // the cut on d*^2 and d*_max
    double b_iso;
    int n_points, max_index;
};

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_xrd_kernel(
    const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets, const float* __restrict__ weights,
    int B, int N, xrd_plan P, arreau_xrd_result out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int first, n;
    float Lm[9];
    int wbad = 0;
    bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [&] {
        for (int a = tid; a < n; a += CRYSTAL_THREADS) wbad |= !isfinite(weights[(size_t)first + a]);
    });
    bad |= __syncthreads_or(wbad) != 0;

    __shared__ float s_pat[ARREAU_XRD_MAX_POINTS];
    __shared__ float s_x[3 * CRYSTAL_LDS_ATOMS], s_w[CRYSTAL_LDS_ATOMS];
    __shared__ double s_tt[CRYSTAL_THREADS];
    __shared__ float s_amp[CRYSTAL_THREADS];
    __shared__ int s_lo[CRYSTAL_THREADS], s_hi[CRYSTAL_THREADS];
    __shared__ int s_slots[CRYSTAL_WAVES];
    __shared__ float s_sum[CRYSTAL_WAVES];

    const float qnan = __int_as_float(0x7fc00000);
    float* const row = out.pattern + (size_t)b * P.n_points;
    // a flagged crystal (workgroup-uniform): nothing is computed, the reals are NaN, the count 0
    auto blank = [&](int flags) {
        for (int p = tid; p < P.n_points; p += CRYSTAL_THREADS) row[p] = qnan;
        if (tid == 0) {
            out.n_reflections[b] = 0; out.volume[b] = qnan; out.weight_sum[b] = qnan; out.flags[b] = flags;
        }
    };
    if (bad) {
        blank(ARREAU_XRD_NONFINITE);
        return;
    }
    // ---- rule 2: the cell in float64 from the float32 entries, the reciprocal rows b_k = (a_i x a_j) / det
    const float volume = crystal_volume(Lm);
    double A[9], R[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) A[q] = (double)Lm[q];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* u = A + 3 * ((k + 1) % 3);
        const double* v = A + 3 * ((k + 2) % 3);
        R[3 * k] = u[1] * v[2] - u[2] * v[1]; R[3 * k + 1] = u[2] * v[0] - u[0] * v[2]; R[3 * k + 2] = u[0] * v[1] - u[1] * v[0];
    }
    const double det = (A[0] * R[0] + A[1] * R[1]) + A[2] * R[2], V = fabs(det);
    if (!(volume > 0.f) || !isfinite(volume) || !(V > 0.) || !isfinite(V)) {
        blank(ARREAU_XRD_CELL);
        return;
    }
    if (n == 0) {
        blank(ARREAU_XRD_EMPTY);
        return;
    }
    // ---- rule 3: the box, H_k = floor(d*_max |a_k|) from the direct cell's lengths
    double Hd[3];
    bool wide = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Hd[k] = floor(P.dhi * sqrt((A[3 * k] * A[3 * k] + A[3 * k + 1] * A[3 * k + 1]) + A[3 * k + 2] * A[3 * k + 2]));
        wide |= !(Hd[k] <= (double)P.max_index);
    }
    if (wide) {
        blank(ARREAU_XRD_RANGE);
        return;
    }
    const int H1 = (int)Hd[0], H2 = (int)Hd[1], H3 = (int)Hd[2];  // <= max_index <= 127
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] /= det;

    // ---- the atoms: wrapped fractional coordinates and amplitudes, in LDS when the crystal fits
    const bool staged = n <= CRYSTAL_LDS_ATOMS;
    if (staged) {
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) s_x[a] = crystal_wrap(frac[3 * (size_t)first + a]);
        for (int a = tid; a < n; a += CRYSTAL_THREADS) s_w[a] = weights[(size_t)first + a];
    }
    for (int p = tid; p < P.n_points; p += CRYSTAL_THREADS) s_pat[p] = 0.f;  // (its own points: no barrier needed for these)
    float wsum = 0.f;
    for (int a = tid; a < n; a += CRYSTAL_THREADS) wsum = __fadd_rn(wsum, weights[(size_t)first + a]);
    wsum = crystal_wave_sum(wsum);
    if (lane == 0) s_sum[wave] = wsum;
    __syncthreads();

    const unsigned W2 = 2u * H2 + 1u, W3 = 2u * H3 + 1u, M = W2 * W3;
    const unsigned long long span = (unsigned long long)(H1 + 1) * M;  // <= 128 * 255^2
    const double inv_sigma = 1.0 / P.sigma, inv_step = 1.0 / P.step, inv_v2 = 1.0 / (V * V), last = (double)(P.n_points - 1);
    const double deg = 57.29577951308232087680;  // 180 / pi
    int kept = 0;
    crystal_walk_chunks(span, M, (unsigned)tid, (unsigned)CRYSTAL_THREADS, [&](bool valid, unsigned uh, unsigned m) {
        const unsigned uk = m / W3;
        const int h = (int)uh, k = (int)uk - H2, l = (int)(m - uk * W3) - H3;
        // ---- rule 4: the half space, d*^2 and the cut, float64
        bool keep = valid && (h > 0 || k > 0 || (k == 0 && l > 0));  // (h >= 0 in the box)
        double d2 = 0.;
        if (keep) {
            const double gx = ((double)h * R[0] + (double)k * R[3]) + (double)l * R[6];
            const double gy = ((double)h * R[1] + (double)k * R[4]) + (double)l * R[7];
            const double gz = ((double)h * R[2] + (double)k * R[5]) + (double)l * R[8];
            d2 = (gx * gx + gy * gy) + gz * gz;
            keep = d2 >= P.dlo2 && d2 <= P.dhi2;
        }
        double tt = 0.;
        float amp = 0.f;
        int lo = 0, hi = -1;
        if (keep) {
            // ---- rule 5: the structure factor, float32 in atom order, the phase in revolutions
            const float hf = (float)h, kf = (float)k, lf = (float)l;
            float re = 0.f, im = 0.f;
            for (int a = 0; a < n; ++a) {
                float x, y, z, w;
                if (staged) {
                    x = s_x[3 * a]; y = s_x[3 * a + 1]; z = s_x[3 * a + 2]; w = s_w[a];
                } else {
                    const size_t g = (size_t)first + a;
                    x = crystal_wrap(frac[3 * g]); y = crystal_wrap(frac[3 * g + 1]); z = crystal_wrap(frac[3 * g + 2]); w = weights[g];
                }
                const float t = __fadd_rn(__fadd_rn(__fmul_rn(hf, x), __fmul_rn(kf, y)), __fmul_rn(lf, z));
                const float r = __fsub_rn(t, rintf(t));
                float s, c;
                sincospif(__fmul_rn(2.0f, r), &s, &c);
                re = __fadd_rn(re, __fmul_rn(w, c));
                im = __fadd_rn(im, __fmul_rn(w, s));
            }
            // ---- rule 6: the angle and the intensity, float64
            const double sth = 0.5 * P.wavelength * sqrt(d2), s2 = sth * sth, c2t = 1.0 - 2.0 * s2;
            const double lp = (1.0 + c2t * c2t) / (s2 * sqrt(1.0 - s2));
            const double f2 = (double)re * (double)re + (double)im * (double)im;
            const double dw = P.b_iso != 0. ? exp(-0.5 * P.b_iso * d2) : 1.0;  // exp(-B s^2)^2, s = d* / 2
            tt = 2.0 * deg * asin(sth);
            amp = (float)((2.0 * f2 * dw * lp * inv_v2) * P.norm);
            // the grid points that may lie inside the window, one to spare on either side; rule 7 tests each
            const double flo = floor((tt - P.six_sigma - P.g0) * inv_step), fhi = ceil((tt + P.six_sigma - P.g0) * inv_step);
            lo = (int)fmin(fmax(flo, 0.), last);
            hi = (int)fmin(fmax(fhi, 0.), last);
        }
        int total;
        const int rank = crystal_compact(keep, lane, wave, s_slots, total);
        if (keep) {
            s_tt[rank] = tt; s_amp[rank] = amp; s_lo[rank] = lo; s_hi[rank] = hi;
        }
        __syncthreads();  // (also: every thread has read s_slots before the next round writes them)
        // ---- rule 7: the round's reflections in ascending box index; this thread's points are p = tid (mod 256)
        for (int e = 0; e < total; ++e) {
            const int elo = s_lo[e], ehi = s_hi[e];
            const double te = s_tt[e];
            const float ae = s_amp[e];
            for (int p = elo + ((tid - elo) & (CRYSTAL_THREADS - 1)); p <= ehi; p += CRYSTAL_THREADS) {
                const double dd = (p == P.n_points - 1 ? P.g1 : P.g0 + (double)p * P.step) - te;
                if (fabs(dd) <= P.six_sigma) {
                    const float z = (float)(dd * inv_sigma);
                    s_pat[p] = __fadd_rn(s_pat[p], __fmul_rn(ae, expf(__fmul_rn(-0.5f, __fmul_rn(z, z)))));
                }
            }
        }
        kept += total;
    });

    for (int p = tid; p < P.n_points; p += CRYSTAL_THREADS) row[p] = s_pat[p];  // (its own points)
    if (tid == 0) {
        float sum = 0.f;
        for (int w = 0; w < CRYSTAL_WAVES; ++w) sum = __fadd_rn(sum, s_sum[w]);
        out.n_reflections[b] = 2 * kept;
        out.volume[b] = volume;
        out.weight_sum[b] = sum;
        out.flags[b] = 0;
    }
}

}  // namespace

extern "C" int arreau_crystal_xrd(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, const float* d_weights,
                                  int32_t B, int32_t N, const arreau_xrd_params* params, arreau_xrd_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_xrd: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_xrd: bad size");
    const arreau_xrd_params& p = *params;
    ARREAU_REQUIRE(std::isfinite(p.wavelength) && p.wavelength > 0., "arreau_crystal_xrd: wavelength must be finite and > 0");
    ARREAU_REQUIRE(p.two_theta_min >= 0. && p.two_theta_min < p.two_theta_max && p.two_theta_max <= ARREAU_XRD_MAX_TWO_THETA,
                   "arreau_crystal_xrd: 0 <= two_theta_min < two_theta_max <= 160 is required");
    ARREAU_REQUIRE(p.n_points >= 2 && p.n_points <= ARREAU_XRD_MAX_POINTS, "arreau_crystal_xrd: n_points must lie in 2..4096");
    ARREAU_REQUIRE(std::isfinite(p.fwhm) && p.fwhm > 0., "arreau_crystal_xrd: fwhm must be finite and > 0");
    ARREAU_REQUIRE(std::isfinite(p.b_iso) && p.b_iso >= 0., "arreau_crystal_xrd: b_iso must be finite and >= 0");
    ARREAU_REQUIRE(p.max_index >= 1 && p.max_index <= ARREAU_XRD_MAX_INDEX, "arreau_crystal_xrd: max_index must lie in 1..127");
    xrd_plan plan;
    plan.sigma = p.fwhm / (2.0 * std::sqrt(2.0 * std::log(2.0)));
    plan.six_sigma = 6.0 * plan.sigma;
    ARREAU_REQUIRE(plan.six_sigma <= ARREAU_XRD_MAX_WINDOW && plan.sigma > 0., "arreau_crystal_xrd: 6 sigma must lie in (0, 10] degrees");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_weights) || N == 0), "arreau_crystal_xrd: null pointer");
    ARREAU_REQUIRE(out->pattern && out->n_reflections && out->volume && out->weight_sum && out->flags, "arreau_crystal_xrd: null result array");
    const double rad = 3.14159265358979323846 / 180.0;
    const double lo = std::fmax(p.two_theta_min - plan.six_sigma, 0.0), hi = p.two_theta_max + plan.six_sigma;  // hi <= 170
    const double dlo = 2.0 * std::sin(0.5 * lo * rad) / p.wavelength;
    plan.dhi = 2.0 * std::sin(0.5 * hi * rad) / p.wavelength;
    ARREAU_REQUIRE(std::isfinite(plan.dhi) && plan.dhi * plan.dhi > 0. && std::isfinite(plan.dhi * plan.dhi),
                   "arreau_crystal_xrd: the wavelength puts the range's d* outside float64");
    plan.dlo2 = dlo * dlo; plan.dhi2 = plan.dhi * plan.dhi;
    plan.wavelength = p.wavelength; plan.b_iso = p.b_iso;
    plan.g0 = p.two_theta_min; plan.g1 = p.two_theta_max;
    plan.step = (p.two_theta_max - p.two_theta_min) / (double)(p.n_points - 1);
    ARREAU_REQUIRE(plan.step > 0. && std::isfinite(1.0 / plan.step), "arreau_crystal_xrd: the grid's step underflows");
    plan.norm = 1.0 / (plan.sigma * std::sqrt(2.0 * 3.14159265358979323846));
    plan.n_points = p.n_points; plan.max_index = p.max_index;
    ARREAU_LAUNCH(crystal_xrd_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_lattice, d_crystal_offsets,
                  d_weights, (int)B, (int)N, plan, *out);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
