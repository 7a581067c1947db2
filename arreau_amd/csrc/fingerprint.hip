// Duplicate detection (arreau_crystal_fingerprint, arreau_fingerprint_match; the rules are written out in include/arreau_hip.h):
// a reduced formula and a pair-distribution fingerprint per crystal, then for every crystal the earliest comparable crystal within
// a tolerance.  Contacts are enumerated as screen.hip enumerates them: the cell and the image walk are crystal_dev.h's in both, the
// contact's arithmetic is crystal_contact_at here and the same operations kept in screen.hip's loop.  No atomics; no order of
// summation depends on where a crystal sits in the batch.  Needs no arreau_model.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

#define FP_LIST 1024                                     // contacts the LDS list holds; it is drained when a further round of
#define FP_DRAIN (FP_LIST - CRYSTAL_THREADS)             // CRYSTAL_THREADS candidates might not fit
#define FP_CELLS (ARREAU_FP_COMPONENTS / CRYSTAL_WAVES)  // (component, bin) cells a thread owns: components wave, wave + 4, ...
#define MATCH_TILE 16                                    // the match kernel's tile: 16 rows of X by 16 rows of Y
#define MATCH_PAD (ARREAU_FP_BINS + 1)

namespace {

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_fingerprint_kernel(
    const float* __restrict__ frac, const int32_t* __restrict__ types, const float* __restrict__ lattice,
    const int32_t* __restrict__ offsets, int B, int N, float r_cut, float rc2 /* r_cut^2 */, float delta, float coef /* log2(e) / (2 sigma^2) */,
    float gnorm /* 1 / (sigma sqrt(2 pi)) */, int n_bins, int max_shells, float* __restrict__ o_fp, int32_t* __restrict__ o_species,
    int32_t* __restrict__ o_counts, int32_t* __restrict__ o_flags) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float spos[3 * CRYSTAL_LDS_ATOMS];
    __shared__ unsigned char srank[CRYSTAL_LDS_ATOMS];
    __shared__ int s_species[ARREAU_FP_MAX_SPECIES], s_count[ARREAU_FP_MAX_SPECIES], s_K;
    __shared__ float s_R[FP_LIST];
    __shared__ unsigned char s_c[FP_LIST];  // component in the low six bits, 64: both atoms of one species (c = 2)
    __shared__ int s_wcnt[2][CRYSTAL_WAVES];
    __shared__ float s_part[CRYSTAL_WAVES];

    float* row = o_fp + (size_t)b * ARREAU_FP_ROW;
    auto flagged = [&](int flags) {  // (workgroup-uniform) a zero row, no formula
#pragma unroll
        for (int q = 0; q < FP_CELLS; ++q) row[(wave + CRYSTAL_WAVES * q) * ARREAU_FP_BINS + lane] = 0.0f;
        if (tid < ARREAU_FP_MAX_SPECIES) {
            o_species[ARREAU_FP_MAX_SPECIES * (size_t)b + tid] = -1;
            o_counts[ARREAU_FP_MAX_SPECIES * (size_t)b + tid] = 0;
        }
        if (tid == 0) o_flags[b] = flags;
    };

    if (bad) return flagged(ARREAU_FP_NONFINITE);

    // ---- the formula: thread 0 inserts the species into a sorted list of at most eight (K = 9: a ninth was met)
    if (tid == 0) {
        int K = 0;
        for (int a = 0; a < n; ++a) {
            const int t = types[(size_t)first + a];
            int q = 0;
            while (q < K && s_species[q] < t) ++q;
            if (q < K && s_species[q] == t) { ++s_count[q]; continue; }
            if (K == ARREAU_FP_MAX_SPECIES) { K = ARREAU_FP_MAX_SPECIES + 1; break; }
            for (int r = K; r > q; --r) { s_species[r] = s_species[r - 1]; s_count[r] = s_count[r - 1]; }
            s_species[q] = t; s_count[q] = 1; ++K;
        }
        s_K = K;
    }
    __syncthreads();
    const int K = s_K;

    // ---- the cell, as in the screen with search_radius = r_cut (every thread computes the same values)
    crystal_cell cell;
    const bool cell_bad = crystal_cell_measure(Lm, r_cut, max_shells, cell) || !(cell.volume > 0.0f);
    const int flags = (n == 0 ? ARREAU_FP_EMPTY : 0) | (K > ARREAU_FP_MAX_SPECIES ? ARREAU_FP_MANY_SPECIES : 0) | (cell_bad ? ARREAU_FP_CELL : 0);
    if (flags) return flagged(flags);
    crystal_cell_images(cell);

    // ---- positions and species ranks: staged in LDS when the crystal fits, else formed from global memory where they are used
    auto rank_of = [&](int t) -> int {
        int r = 0;
        for (int q = 0; q < K; ++q) r = s_species[q] == t ? q : r;
        return r;
    };
    if (n <= CRYSTAL_LDS_ATOMS)
        for (int a = tid; a < n; a += CRYSTAL_THREADS) srank[a] = (unsigned char)rank_of(types[(size_t)first + a]);
    const crystal_positions position = crystal_stage_positions(spos, frac, Lm, first, n);  // (its barrier covers the ranks)
    auto species_rank = [&](int atom) -> int { return position.staged ? (int)srank[atom] : rank_of(types[(size_t)first + atom]); };

    // ---- the gather.  A thread owns bin `lane` of the components wave, wave + 4, ...; contacts inside r_cut are compacted into
    // the LDS list in enumeration order (i, j, m) and every cell adds the list's entries in that order.
    float acc[FP_CELLS];
#pragma unroll
    for (int q = 0; q < FP_CELLS; ++q) acc[q] = 0.0f;
    const float Rk = ((float)lane + 0.5f) * delta;
    int cnt = 0;  // (uniform) entries in the list
    auto drain = [&]() {
        __syncthreads();  // the list is complete
        for (int e = 0; e < cnt; ++e) {
            const int c = __builtin_amdgcn_readfirstlane((int)s_c[e]);
            if ((c & (CRYSTAL_WAVES - 1)) != wave) continue;  // (uniform) another wave's component
            const float x = Rk - s_R[e];
            const float g = __builtin_amdgcn_exp2f(-(x * x) * coef);  // one v_exp_f32
            const float v = (c & 64) ? g + g : g;
            const int cq = (c & 63) >> 2;
#pragma unroll
            for (int q = 0; q < FP_CELLS; ++q)
                if (cq == q) acc[q] += v;
        }
        __syncthreads();  // before the list is written again
        cnt = 0;
    };
    int parity = 0;
    for (int i = 0; i < n; ++i) {
        const float pix = position(i, 0), piy = position(i, 1), piz = position(i, 2);
        const int ri = species_rank(i);
        crystal_walk_chunks((unsigned long long)(n - i) * cell.M, cell.M, (unsigned)tid, CRYSTAL_THREADS, [&](bool valid, unsigned dj, unsigned m) {
            bool hit = false;
            float R = 0.0f;
            int comp = 0;
            if (valid && !(dj == 0 && m <= cell.centre)) {  // an atom with itself: only the images after (0, 0, 0)
                const int j = i + (int)dj;
                const float d2 = crystal_contact_at(cell, Lm, position, j, m, pix, piy, piz).d2;
                if (d2 < rc2) {
                    hit = true;
                    R = sqrtf(d2);
                    const int rj = species_rank(j), A = min(ri, rj), Bq = max(ri, rj);
                    comp = (Bq * (Bq + 1) / 2 + A) | (A == Bq ? 64 : 0);
                }
            }
            // the hits of this round, in thread order: the wave's ballot, then a prefix over the four waves
            // (the other parity's counts are not written before every thread has passed the helper's barrier again)
            int total;
            const int at = cnt + crystal_compact(hit, lane, wave, s_wcnt[parity], total);  // < FP_LIST: cnt <= FP_DRAIN here
            if (hit) {
                s_R[at] = R;
                s_c[at] = (unsigned char)comp;
            }
            cnt += total;
            parity ^= 1;
            if (cnt > FP_DRAIN) drain();
        });
    }
    drain();

    // ---- F, its weighted norm (a fixed-order sum: the thread's cells, the wave's lanes, the four waves) and the stored row
    const float pref = cell.volume * gnorm / (4.0f * 3.14159265358979323846f);
    const float fn = (float)n;
    float Fv[FP_CELLS], sw[FP_CELLS], part = 0.0f;
#pragma unroll
    for (int q = 0; q < FP_CELLS; ++q) {
        const int c = wave + CRYSTAL_WAVES * q;
        int Bq = 0;
        while ((Bq + 1) * (Bq + 2) / 2 <= c) ++Bq;
        const int A = c - Bq * (Bq + 1) / 2;
        Fv[q] = 0.0f; sw[q] = 0.0f;
        if (Bq < K && lane < n_bins) {
            const float na = (float)s_count[A], nb = (float)s_count[Bq];
            const float w = na * nb / (fn * fn);
            Fv[q] = acc[q] * pref / (Rk * Rk * na * nb) - 1.0f;
            sw[q] = sqrtf(w);
            part += w * Fv[q] * Fv[q];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) s_part[wave] = part;
    __syncthreads();
    const float norm2 = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
    const float inv = norm2 > 0.0f ? 1.0f / sqrtf(norm2) : 0.0f;
#pragma unroll
    for (int q = 0; q < FP_CELLS; ++q) row[(wave + CRYSTAL_WAVES * q) * ARREAU_FP_BINS + lane] = sw[q] * Fv[q] * inv;
    if (tid < ARREAU_FP_MAX_SPECIES) {
        int g = 0;  // gcd of the counts
        for (int q = 0; q < K; ++q) {
            int u = s_count[q], v = g;
            while (v) { const int r = u % v; u = v; v = r; }
            g = u;
        }
        o_species[ARREAU_FP_MAX_SPECIES * (size_t)b + tid] = tid < K ? s_species[tid] : -1;
        o_counts[ARREAU_FP_MAX_SPECIES * (size_t)b + tid] = tid < K ? s_count[tid] / g : 0;
    }
    if (tid == 0) o_flags[b] = 0;
}

// One workgroup per tile of 16 rows of X; it walks the tiles of 16 rows of Y in ascending order, thread (tx, ty) holding the pair
// (x0 + tx, y0 + ty).  The formulas are compared first; a tile without a comparable pair loads nothing.  The dot product is plain
// fp32 FMAs over LDS-staged components, ascending index.  A thread meets its candidates in ascending index, the sixteen threads of
// a row are combined by (d, index) at the end: ties go to the smaller index without atomics.
__global__ __launch_bounds__(MATCH_TILE * MATCH_TILE) void fingerprint_match_kernel(
    const float* __restrict__ xf, const int32_t* __restrict__ xs, const int32_t* __restrict__ xc, const int32_t* __restrict__ xflags, int Bx,
    const float* __restrict__ yf, const int32_t* __restrict__ ys, const int32_t* __restrict__ yc, const int32_t* __restrict__ yflags, int By,
    int self, float tolerance, int32_t* __restrict__ o_dup, float* __restrict__ o_dist, int32_t* __restrict__ o_near, float* __restrict__ o_neard) {
    constexpr int T = MATCH_TILE, S = ARREAU_FP_MAX_SPECIES, FORM = 2 * S + 1;
    __shared__ float sx[T][MATCH_PAD], sy[T][MATCH_PAD];
    __shared__ int fx[T][FORM], fy[T][FORM];  // species, counts, flags (-1: no such row)
    __shared__ float r_d[T][T], r_dupd[T][T];
    __shared__ int r_a[T][T], r_dup[T][T], s_k[2][T * T / 64];
    const int tid = threadIdx.x, tx = tid & (T - 1), ty = tid / T;
    const int x0 = blockIdx.x * T, x = x0 + tx;
    auto load_formula = [&](int (*f)[FORM], const int32_t* s, const int32_t* c, const int32_t* fl, int r0, int rows) {
        for (int e = tid; e < T * FORM; e += T * T) {
            const int r = e / FORM, q = e % FORM, g = r0 + r;
            f[r][q] = g >= rows ? -1 : (q < S ? s[S * (size_t)g + q] : (q < 2 * S ? c[S * (size_t)g + q - S] : fl[g]));
        }
    };
    load_formula(fx, xs, xc, xflags, x0, Bx);
    __syncthreads();
    int Kx = 0;  // species of x (the counts are positive where a species is)
    for (int q = 0; q < S; ++q) Kx += fx[tx][S + q] > 0;
    const float inf = __int_as_float(0x7f800000);
    float best_d = inf, dup_d = inf;
    int best_a = -1, dup = -1;
    const int y_tiles = self ? (int)blockIdx.x + 1 : (By + T - 1) / T;
    for (int t = 0; t < y_tiles; ++t) {
        const int y0 = t * T, a = y0 + ty;
        load_formula(fy, ys, yc, yflags, y0, By);
        __syncthreads();
        bool comparable = x < Bx && a < By && (!self || a < x) && fx[tx][2 * S] == 0 && fy[ty][2 * S] == 0 && Kx > 0;
        for (int q = 0; q < 2 * S; ++q) comparable = comparable && fx[tx][q] == fy[ty][q];
        // the most species a comparable pair of this tile has: the wave's maximum, then the four waves through LDS (the
        // counts alternate between two slots, so one barrier a tile is enough; every read of fy precedes it)
        int Kmax = comparable ? Kx : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) Kmax = max(Kmax, __shfl_xor(Kmax, off));
        if ((tid & 63) == 0) s_k[t & 1][tid >> 6] = Kmax;
        __syncthreads();
        Kmax = max(max(s_k[t & 1][0], s_k[t & 1][1]), max(s_k[t & 1][2], s_k[t & 1][3]));
        if (Kmax == 0) continue;  // (uniform) no comparable pair: nothing is loaded
        const int nc = Kmax * (Kmax + 1) / 2;  // components beyond a crystal's own are zero
        float dot = 0.0f;
        for (int c = 0; c < nc; ++c) {
            __syncthreads();
            for (int e = tid; e < T * ARREAU_FP_BINS; e += T * T) {
                const int r = e / ARREAU_FP_BINS, k = e % ARREAU_FP_BINS;
                sx[r][k] = x0 + r < Bx ? xf[(size_t)(x0 + r) * ARREAU_FP_ROW + c * ARREAU_FP_BINS + k] : 0.0f;
                sy[r][k] = y0 + r < By ? yf[(size_t)(y0 + r) * ARREAU_FP_ROW + c * ARREAU_FP_BINS + k] : 0.0f;
            }
            __syncthreads();
#pragma unroll 16
            for (int k = 0; k < ARREAU_FP_BINS; ++k) dot = fmaf(sx[tx][k], sy[ty][k], dot);
        }
        if (comparable) {
            const float d = 0.5f * (1.0f - dot);
            if (d < best_d) { best_d = d; best_a = a; }
            if (dup < 0 && d <= tolerance) { dup = a; dup_d = d; }
        }
    }
    r_d[tx][ty] = best_d; r_a[tx][ty] = best_a; r_dup[tx][ty] = dup; r_dupd[tx][ty] = dup_d;
    __syncthreads();
    if (tid < T && x0 + tid < Bx) {
        float bd = inf, dd = inf;
        int ba = -1, da = -1;
        for (int q = 0; q < T; ++q) {
            const int a = r_a[tid][q], u = r_dup[tid][q];
            if (a >= 0 && (ba < 0 || r_d[tid][q] < bd || (r_d[tid][q] == bd && a < ba))) { bd = r_d[tid][q]; ba = a; }
            if (u >= 0 && (da < 0 || u < da)) { da = u; dd = r_dupd[tid][q]; }
        }
        o_dup[x0 + tid] = da; o_dist[x0 + tid] = dd; o_near[x0 + tid] = ba; o_neard[x0 + tid] = bd;
    }
}

bool complete(const arreau_fingerprint_result* r) { return r->fingerprint && r->species && r->counts && r->flags; }

}  // namespace

extern "C" int arreau_crystal_fingerprint(const float* d_frac, const int32_t* d_types, const float* d_lattice,
                                          const int32_t* d_crystal_offsets, int32_t B, int32_t N, const arreau_fingerprint_params* params,
                                          arreau_fingerprint_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_fingerprint: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_fingerprint: bad size");
    ARREAU_REQUIRE(params->n_bins >= 1 && params->n_bins <= ARREAU_FP_BINS, "arreau_crystal_fingerprint: n_bins must lie in 1..64");
    ARREAU_REQUIRE(std::isfinite(params->r_max) && params->r_max > 0.f, "arreau_crystal_fingerprint: r_max must be finite and > 0");
    ARREAU_REQUIRE(std::isfinite(params->sigma) && params->sigma > 0.f, "arreau_crystal_fingerprint: sigma must be finite and > 0");
    ARREAU_REQUIRE(params->max_shells >= 1 && params->max_shells <= ARREAU_SCREEN_MAX_SHELLS,
                   "arreau_crystal_fingerprint: max_shells must lie in 1..8");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_types) || N == 0), "arreau_crystal_fingerprint: null pointer");
    ARREAU_REQUIRE(complete(out), "arreau_crystal_fingerprint: null result array");
    const double sigma = (double)params->sigma;
    const float r_cut = (float)((double)params->r_max + 5.0 * sigma);
    const float rc2 = (float)((double)r_cut * (double)r_cut);
    const float delta = params->r_max / (float)params->n_bins;
    const float coef = (float)(1.4426950408889634 / (2.0 * sigma * sigma));
    const float gnorm = (float)(1.0 / (sigma * 2.5066282746310002));
    ARREAU_LAUNCH(crystal_fingerprint_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_types, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, r_cut, rc2, delta, coef, gnorm, (int)params->n_bins, (int)params->max_shells,
                  out->fingerprint, out->species, out->counts, out->flags);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

extern "C" int arreau_fingerprint_match(const arreau_fingerprint_result* x, int32_t Bx, const arreau_fingerprint_result* y, int32_t By,
                                        float tolerance, arreau_match_result* out, void* stream) {
    ARREAU_REQUIRE(x != nullptr && out != nullptr, "arreau_fingerprint_match: null set or result");
    ARREAU_REQUIRE(Bx >= 0 && (y == nullptr || By >= 0), "arreau_fingerprint_match: bad size");
    ARREAU_REQUIRE(tolerance >= 0.f && tolerance <= 1.f, "arreau_fingerprint_match: tolerance must lie in [0, 1]");
    if (Bx == 0) return ARREAU_OK;
    ARREAU_REQUIRE(complete(x) && (y == nullptr || By == 0 || complete(y)), "arreau_fingerprint_match: null set array");
    ARREAU_REQUIRE(out->duplicate_of && out->distance && out->nearest && out->nearest_distance,
                   "arreau_fingerprint_match: null result array");
    const bool self = y == nullptr;
    const arreau_fingerprint_result* s = self ? x : y;
    ARREAU_LAUNCH(fingerprint_match_kernel, dim3((unsigned)((Bx + MATCH_TILE - 1) / MATCH_TILE)), dim3(MATCH_TILE * MATCH_TILE), 0,
                  (hipStream_t)stream, x->fingerprint, x->species, x->counts, x->flags, (int)Bx, s->fingerprint, s->species, s->counts,
                  s->flags, self ? (int)Bx : (int)By, self ? 1 : 0, tolerance, out->duplicate_of, out->distance, out->nearest,
                  out->nearest_distance);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
