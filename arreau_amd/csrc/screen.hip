// Structural screen of a batch of crystals (arreau_crystal_screen; the rules are written out in include/arreau_hip.h): the
// shortest interatomic contact over every periodic image within a search radius, the cell volume, the mask state.  An exact
// search of its own: the sampling step's neighbour list looks at 27 images, stops at k inside a radius and skips overlapping
// pairs.  One launch, one workgroup of four waves per crystal, no atomics; needs no arreau_model.
#include "internal.h"
#include "graph_dev.h"
#include "crystal_dev.h"
#include <cmath>

namespace {

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_screen_kernel(
    const float* __restrict__ frac, const int32_t* __restrict__ types, const float* __restrict__ lattice,
    const int32_t* __restrict__ offsets, int B, int N, float min_volume, float md2 /* min_distance^2 */, float r2 /* search_radius^2 */,
    float radius, int mask_type, int max_shells, float* __restrict__ o_dist, int32_t* __restrict__ o_pair,
    int32_t* __restrict__ o_close, float* __restrict__ o_volume, float* __restrict__ o_density, int32_t* __restrict__ o_flags) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int first, n;
    float Lm[9];
    int masked = 0;
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [&] {  // NONFINITE, and MASKED ahead of its barrier
        if (types != nullptr && mask_type >= 0)
            for (int a = tid; a < n; a += CRYSTAL_THREADS) masked |= types[(size_t)first + a] == mask_type;
    });
    masked = __syncthreads_or(masked);

    __shared__ float spos[3 * CRYSTAL_LDS_ATOMS];
    __shared__ unsigned s_d2[CRYSTAL_WAVES];
    __shared__ unsigned long long s_ij[CRYSTAL_WAVES];
    __shared__ unsigned s_m[CRYSTAL_WAVES];
    __shared__ int s_close[CRYSTAL_WAVES];

    const float qnan = __int_as_float(0x7fc00000);
    if (bad) {  // (workgroup-uniform) nothing else is computed
        if (tid == 0) {
            o_dist[b] = qnan; o_volume[b] = qnan; o_density[b] = qnan;
            o_close[b] = 0; o_flags[b] = ARREAU_SCREEN_NONFINITE;
        }
        if (tid < 5) o_pair[5 * (size_t)b + tid] = -1;
        return;
    }

    // ---- the cell: volume, plane spacings, images per axis (every thread computes the same values)
    crystal_cell cell;
    const bool cell_bad = crystal_cell_measure(Lm, radius, max_shells, cell) || !(cell.volume >= min_volume);
    const float volume = cell.volume, density = __fdiv_rn((float)n, volume);
    int flags = masked ? ARREAU_SCREEN_MASKED : 0;
    if (cell_bad) {  // (workgroup-uniform) the search is skipped
        if (tid == 0) {
            o_dist[b] = qnan; o_volume[b] = volume; o_density[b] = density;
            o_close[b] = 0; o_flags[b] = flags | ARREAU_SCREEN_CELL;
        }
        if (tid < 5) o_pair[5 * (size_t)b + tid] = -1;
        return;
    }
    crystal_cell_images(cell);

    const crystal_positions position = crystal_stage_positions(spos, frac, Lm, first, n);

    // ---- the search.  Receiver i (uniform), then the flattened (j >= i, image m) range dealt to the 256 threads: every thread
    // meets its contacts in ascending (i, j, m), so a strict "<" on the bits of d2 keeps the first of equal minima.
    unsigned best_d2 = 0xffffffffu, best_m = 0;  // bits of d2 (d2 >= +0: the bits order like the values; NaN cannot arise from
    unsigned long long best_ij = ~0ull;          // finite inputs, inf keeps its place above every finite value)
    int close = 0;
    for (int i = 0; i < n; ++i) {
        const float pix = position(i, 0), piy = position(i, 1), piz = position(i, 2);
        auto contact = [&](unsigned dj, unsigned m) {
            if (dj == 0 && m <= cell.centre) return;  // an atom with itself: only the images after (0, 0, 0)
            const int j = i + (int)dj;
            // crystal_contact_at's operations, kept in the loop: through the helper they are packed in pairs, and 1024 random
            // crystals of 64 atoms take 153.1 us against 152.2 us (medians, MI355X; 256 x 20 is 0.3 us faster through it)
            const unsigned m12 = m / cell.W3;
            const float n3 = (float)((int)(m - m12 * cell.W3) - cell.N3), n2 = (float)((int)(m12 % cell.W2) - cell.N2), n1 = (float)((int)(m12 / cell.W2) - cell.N1);
            const float sx = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[0]), __fmul_rn(n2, Lm[3])), __fmul_rn(n3, Lm[6]));
            const float sy = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[1]), __fmul_rn(n2, Lm[4])), __fmul_rn(n3, Lm[7]));
            const float sz = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[2]), __fmul_rn(n2, Lm[5])), __fmul_rn(n3, Lm[8]));
            const float dx = __fsub_rn(__fadd_rn(position(j, 0), sx), pix);
            const float dy = __fsub_rn(__fadd_rn(position(j, 1), sy), piy);
            const float dz = __fsub_rn(__fadd_rn(position(j, 2), sz), piz);
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            close += d2 < md2 ? 1 : 0;
            const unsigned bits = __float_as_uint(d2);
            if (bits < best_d2) {
                best_d2 = bits;
                best_ij = ((unsigned long long)i << 24) | (unsigned long long)j;
                best_m = m;
            }
        };
        crystal_walk((unsigned long long)(n - i) * cell.M, cell.M, (unsigned)tid, CRYSTAL_THREADS, contact);
    }

    // ---- deterministic reduction: the wave minimum of the ordered key (bits of d2; i, j; m), one exact double each
    // (arreau_wave_min_f64, graph_dev.h), then the four waves through LDS.  A lane without a contact holds the largest key.
    constexpr double NONE = 1.0e300;
    const double wd2 = arreau_wave_min_f64((double)best_d2);
    const double wij = arreau_wave_min_f64((double)best_d2 == wd2 && best_ij != ~0ull ? (double)best_ij : NONE);  // i, j < 2^24: exact
    const double wm = arreau_wave_min_f64((double)best_d2 == wd2 && (double)best_ij == wij ? (double)best_m : NONE);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) close += __shfl_xor(close, off);  // (an integer sum: any order gives the same value)
    if (lane == 0) {
        s_d2[wave] = (unsigned)wd2;
        s_ij[wave] = wij == NONE ? ~0ull : (unsigned long long)wij;
        s_m[wave] = wm == NONE ? 0xffffffffu : (unsigned)wm;
        s_close[wave] = close;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned d2b = s_d2[0], mm = s_m[0];
        unsigned long long ij = s_ij[0];
        int total = s_close[0];
        for (int w = 1; w < CRYSTAL_WAVES; ++w) {
            total += s_close[w];
            const bool less = s_d2[w] < d2b || (s_d2[w] == d2b && (s_ij[w] < ij || (s_ij[w] == ij && s_m[w] < mm)));
            if (less) { d2b = s_d2[w]; ij = s_ij[w]; mm = s_m[w]; }
        }
        int32_t* pr = o_pair + 5 * (size_t)b;
        if (total > 0) flags |= ARREAU_SCREEN_CLOSE;
        if (ij == ~0ull) {  // no contact at all (an empty crystal)
            o_dist[b] = __int_as_float(0x7f800000);
            pr[0] = pr[1] = pr[2] = pr[3] = pr[4] = -1;
            flags |= ARREAU_SCREEN_BEYOND;
        } else {
            const float d2 = __uint_as_float(d2b);
            o_dist[b] = sqrtf(d2);  // correctly rounded, like the neighbour list's distance
            pr[0] = (int)(ij >> 24); pr[1] = (int)(ij & 0xffffffull);
            crystal_image(cell, mm, pr + 2);
            if (!(d2 <= r2)) flags |= ARREAU_SCREEN_BEYOND;
        }
        o_volume[b] = volume; o_density[b] = density;
        o_close[b] = total; o_flags[b] = flags;
    }
}

}  // namespace

extern "C" int arreau_crystal_screen(const float* d_frac, const int32_t* d_types, const float* d_lattice,
                                     const int32_t* d_crystal_offsets, int32_t B, int32_t N, const arreau_screen_criteria* crit,
                                     arreau_screen_result* out, void* stream) {
    ARREAU_REQUIRE(crit != nullptr && out != nullptr, "arreau_crystal_screen: null criteria or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_screen: bad size");
    ARREAU_REQUIRE(std::isfinite(crit->min_distance) && crit->min_distance >= 0.f && std::isfinite(crit->min_volume) && crit->min_volume >= 0.f,
                   "arreau_crystal_screen: min_distance and min_volume must be finite and >= 0");
    ARREAU_REQUIRE(std::isfinite(crit->search_radius) && crit->search_radius > 0.f && crit->search_radius >= crit->min_distance,
                   "arreau_crystal_screen: search_radius must be finite, > 0 and at least min_distance");
    ARREAU_REQUIRE(crit->max_shells >= 1 && crit->max_shells <= ARREAU_SCREEN_MAX_SHELLS,
                   "arreau_crystal_screen: max_shells must lie in 1..8");
    ARREAU_REQUIRE(crit->mask_type >= -1, "arreau_crystal_screen: mask_type must be -1 (none) or a class index");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && (d_frac || N == 0), "arreau_crystal_screen: null pointer");
    ARREAU_REQUIRE(out->min_distance && out->pair && out->n_close && out->volume && out->number_density && out->flags,
                   "arreau_crystal_screen: null result array");
    const float md2 = (float)((double)crit->min_distance * (double)crit->min_distance);
    const float r2 = (float)((double)crit->search_radius * (double)crit->search_radius);
    ARREAU_LAUNCH(crystal_screen_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_types, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, crit->min_volume, md2, r2, crit->search_radius, (int)crit->mask_type,
                  (int)crit->max_shells, out->min_distance, out->pair, out->n_close, out->volume, out->number_density, out->flags);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
