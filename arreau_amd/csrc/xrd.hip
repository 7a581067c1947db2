// Powder X-ray diffraction patterns of a batch of crystals (arreau_crystal_xrd; the rules are written out in include/arreau_hip.h):
// per crystal the structure-factor sum over the reciprocal-lattice points of one half space inside the 2 theta range, each
// reflection's Lorentz-polarisation-weighted intensity, and the pattern -- the reflections as Gaussians on a fixed 2 theta grid.
// The first per-crystal kernel that walks reciprocal space: the flat range it deals to its threads (crystal_walk_chunks) is the
// box index e = (h W_2 + (k + H_2)) W_3 + (l + H_3), not an image index.  One launch, one workgroup of four waves per crystal, a
// thread per reflection of a round of 256 box entries, no atomics; needs no arreau_model.  The walk itself (the cell and its box, a
// box entry's reflection, the Gaussian term, the rounds) lives in xrd_dev.h, which xrd_guide.hip includes too.
//
// Per reflection d*^2, the 2 theta cut, theta = asin, the Lorentz-polarisation factor and the Debye-Waller factor are float64 from
// the float32 cell taken as exact (one asin and one sqrt per KEPT reflection, nothing per atom); the atom sum is float32 in atom
// order, the phase reduced in revolutions (t - rint(t)) before sincospif; the Gaussians are float32 of a float64 difference g - 2
// theta_hkl.  A round's kept reflections are compacted in thread order (crystal_compact) and added one after another; thread t
// owns the grid points p = t (mod 256) throughout, so every point receives its terms in ascending box index whatever the launch
// or the batch, and the pattern needs no barrier of its own.
//
// LDS per workgroup: 25888 B as the compiler reports it (group_segment_fixed_size), with 121 VGPRs and no scratch: four waves per
// SIMD by registers.  What the bytes are: pattern 4096 floats 16384 B, wrapped coordinates 3 * 256 floats 3072 B, weights 1024 B,
// a round's list (2 theta as double, amplitude, first and last grid point) 256 * 20 = 5120 B, 8 words of slots and partial sums:
// 25632 B; the rest is alignment.
#include "internal.h"
#include "xrd_dev.h"
#include <cmath>

namespace {

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
    // ---- rules 2 and 3: the cell, its reciprocal rows and the box (xrd_dev.h)
    xrd_cell cell;
    const int cell_flag = xrd_cell_measure(Lm, n, P, cell);
    if (cell_flag) {
        blank(cell_flag);
        return;
    }
    const float volume = cell.volume;

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

    // ---- rules 4-7: the walk (xrd_dev.h)
    const int kept = xrd_pattern_walk(P, cell, n, xrd_atoms{s_x, s_w, frac, weights, (size_t)first, staged}, s_pat,
                                      xrd_round_lds{s_tt, s_amp, s_lo, s_hi, s_slots});

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

int arreau_xrd_plan_of(const arreau_xrd_params* params, const char* who, xrd_plan* out) {
    const std::string name(who);
    ARREAU_REQUIRE(params != nullptr, name + ": null params or result");
    const arreau_xrd_params& p = *params;
    ARREAU_REQUIRE(std::isfinite(p.wavelength) && p.wavelength > 0., name + ": wavelength must be finite and > 0");
    ARREAU_REQUIRE(p.two_theta_min >= 0. && p.two_theta_min < p.two_theta_max && p.two_theta_max <= ARREAU_XRD_MAX_TWO_THETA,
                   name + ": 0 <= two_theta_min < two_theta_max <= 160 is required");
    ARREAU_REQUIRE(p.n_points >= 2 && p.n_points <= ARREAU_XRD_MAX_POINTS, name + ": n_points must lie in 2..4096");
    ARREAU_REQUIRE(std::isfinite(p.fwhm) && p.fwhm > 0., name + ": fwhm must be finite and > 0");
    ARREAU_REQUIRE(std::isfinite(p.b_iso) && p.b_iso >= 0., name + ": b_iso must be finite and >= 0");
    ARREAU_REQUIRE(p.max_index >= 1 && p.max_index <= ARREAU_XRD_MAX_INDEX, name + ": max_index must lie in 1..127");
    xrd_plan plan;
    plan.sigma = p.fwhm / (2.0 * std::sqrt(2.0 * std::log(2.0)));
    plan.six_sigma = 6.0 * plan.sigma;
    ARREAU_REQUIRE(plan.six_sigma <= ARREAU_XRD_MAX_WINDOW && plan.sigma > 0., name + ": 6 sigma must lie in (0, 10] degrees");
    const double rad = 3.14159265358979323846 / 180.0;
    const double lo = std::fmax(p.two_theta_min - plan.six_sigma, 0.0), hi = p.two_theta_max + plan.six_sigma;  // hi <= 170
    const double dlo = 2.0 * std::sin(0.5 * lo * rad) / p.wavelength;
    plan.dhi = 2.0 * std::sin(0.5 * hi * rad) / p.wavelength;
    ARREAU_REQUIRE(std::isfinite(plan.dhi) && plan.dhi * plan.dhi > 0. && std::isfinite(plan.dhi * plan.dhi),
                   name + ": the wavelength puts the range's d* outside float64");
    plan.dlo2 = dlo * dlo; plan.dhi2 = plan.dhi * plan.dhi;
    plan.wavelength = p.wavelength; plan.b_iso = p.b_iso;
    plan.g0 = p.two_theta_min; plan.g1 = p.two_theta_max;
    plan.step = (p.two_theta_max - p.two_theta_min) / (double)(p.n_points - 1);
    ARREAU_REQUIRE(plan.step > 0. && std::isfinite(1.0 / plan.step), name + ": the grid's step underflows");
    plan.norm = 1.0 / (plan.sigma * std::sqrt(2.0 * 3.14159265358979323846));
    plan.n_points = p.n_points; plan.max_index = p.max_index;
    *out = plan;
    return ARREAU_OK;
}

extern "C" int arreau_crystal_xrd(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, const float* d_weights,
                                  int32_t B, int32_t N, const arreau_xrd_params* params, arreau_xrd_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_xrd: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_xrd: bad size");
    xrd_plan plan;
    int rc;
    if ((rc = arreau_xrd_plan_of(params, "arreau_crystal_xrd", &plan))) return rc;
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_weights) || N == 0), "arreau_crystal_xrd: null pointer");
    ARREAU_REQUIRE(out->pattern && out->n_reflections && out->volume && out->weight_sum && out->flags, "arreau_crystal_xrd: null result array");
    ARREAU_LAUNCH(crystal_xrd_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_lattice, d_crystal_offsets,
                  d_weights, (int)B, (int)N, plan, *out);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
