// Structure match of pairs of crystals (arreau_structure_match; the rules are written out in include/arreau_hip.h): is crystal x of
// one batch crystal y of another, under which change of basis W and translation, with which atom-to-atom map and how far off in A.
// One launch, one workgroup of four waves per pair, no atomics; needs no arreau_model.
//   phase 1  the 3^9 codes in contiguous ranges of 77 per thread: count the lattice mappings (lengths within ltol, angles within
//            angle_tol of x's), one prefix scan over the workgroup, then the threads that found some evaluate their range again
//            and write the first max_mappings codes in code order (LDS);
//   phase 2  the candidates (W, q), q the atoms of y of x's rarest species, in (code, q) order, four at a time, one per wave: the
//            lanes run over the atoms i of x and take the nearest atom j of y of i's species under the mean metric (27 images per
//            pair); the map goes to LDS (crystals of up to 256 atoms) or to out.scratch (larger ones), the differences are summed
//            in atom order by lane reads; after a barrier the wave checks that the map is one-to-one, refines the translation and
//            forms the rms again from the stored partners; lane 0 keeps the wave's best (rms, code, q);
//   phase 3  the best of the four waves; wave 0 evaluates that candidate once more (the same float32 operations, the same bits)
//            and writes partner, translation, rms, max_dist, rms_norm.
// The kernel is a template on the assignment mode (rule 6b).  The assigning instance keeps every same-species dist^2 of part A as
// the candidate's cost matrix (LDS up to ARREAU_SM_ASSIGN_LDS_ATOMS atoms, d_cost above) and, where the nearest-partner map is not
// one-to-one, the wave that owns the candidate solves the linear assignment by shortest augmenting paths, columns on lanes in
// blocks of 64, in exact 64-bit integer arithmetic on the costs rounded to multiples of 2^-24 A^2; phase 3 repeats it.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

namespace {

struct sm_side {
    const float* frac;
    const int32_t* types;
    const float* lattice;
    const int32_t* offsets;
    int B, N;
};

struct sm_out {
    float *rms, *rms_norm, *max_dist;
    int32_t* mapping;
    float* translation;
    int32_t *partner, *n_mappings, *n_candidates, *n_permutations, *matched, *flags, *scratch;
    int stride;
};

// lengths sqrt(G_ii) and angles (angle i between the other two vectors: acos of the clamped quotient, the symmetrization's rule 5)
// of a metric 00, 11, 22, 01, 02, 12
__device__ __forceinline__ void metric_lengths(const float* g, float* len) {
#pragma unroll
    for (int i = 0; i < 3; ++i) len[i] = sqrtf(g[i]);
}

__device__ __forceinline__ float metric_angle(const float* g, const float* len, int i) {
    const int pj[3] = {1, 0, 0}, pk[3] = {2, 2, 1}, pe[3] = {5, 4, 3};
    const float c = __fdiv_rn(g[pe[i]], __fmul_rn(len[pj[i]], len[pk[i]]));
    return acosf(fminf(fmaxf(c, -1.f), 1.f));
}

// rule 2: does the code map y's lattice onto x's within ltol (relative, lengths) and angle_tol (radians)?
__device__ bool mapping_candidate(int code, const float* Ly, const float* lenx, const float* angx, float ltol, float angle_tol) {
    int W[9];
    const int det = decode_rotation(code, W);
    if (det != 1 && det != -1) return false;
    float g[6], len[3];
    image_metric(W, Ly, g);
    metric_lengths(g, len);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && fabsf(__fsub_rn(len[i], lenx[i])) <= __fmul_rn(ltol, lenx[i]);  // (a NaN fails)
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && fabsf(__fsub_rn(metric_angle(g, len, i), angx[i])) <= angle_tol;
    return ok;
}

// e G e^T of a metric 00, 11, 22, 01, 02, 12: g_r = (G_r0 e_0 + G_r1 e_1) + G_r2 e_2, then (e_0 g_0 + e_1 g_1) + e_2 g_2; a rounded
// result below 0 becomes 0
__device__ __forceinline__ float metric_d2(float e0, float e1, float e2, const float* G) {
    const float g0 = __fadd_rn(__fadd_rn(__fmul_rn(G[0], e0), __fmul_rn(G[3], e1)), __fmul_rn(G[4], e2));
    const float g1 = __fadd_rn(__fadd_rn(__fmul_rn(G[3], e0), __fmul_rn(G[1], e1)), __fmul_rn(G[5], e2));
    const float g2 = __fadd_rn(__fadd_rn(__fmul_rn(G[4], e0), __fmul_rn(G[5], e1)), __fmul_rn(G[2], e2));
    return fmaxf(dot3_rn(e0, e1, e2, g0, g1, g2), 0.f);
}

// rule 4: each component minus its nearest integer, then the smallest e G e^T over the 27 images s in {-1, 0, 1}^3, s_0 slowest, the
// first on ties; e becomes the difference of that image
__device__ __forceinline__ float nearest_image_d2(float* e, const float* G) {
    const float r0 = __fsub_rn(e[0], rintf(e[0])), r1 = __fsub_rn(e[1], rintf(e[1])), r2 = __fsub_rn(e[2], rintf(e[2]));
    float best = __int_as_float(0x7f800000);
    for (int s0 = -1; s0 <= 1; ++s0)
        for (int s1 = -1; s1 <= 1; ++s1)
#pragma unroll
            for (int s2 = -1; s2 <= 1; ++s2) {
                const float f0 = __fadd_rn(r0, (float)s0), f1 = __fadd_rn(r1, (float)s1), f2 = __fadd_rn(r2, (float)s2);
                const float d2 = metric_d2(f0, f1, f2, G);
                if (d2 < best) { best = d2; e[0] = f0; e[1] = f1; e[2] = f2; }
            }
    return best;
}

constexpr int SM_ROW_V = 0, SM_ROW_D = 2, SM_ROW_Y = 4, SM_ROW_PRED = 5;  // the solver's state rows (v and d: low word, high word)
constexpr int SM_EXCLUDED = -2147483647 - 1;                              // pred of a column of another species
static_assert(ARREAU_SM_ASSIGN_STATE_ROWS == 6, "v (2), d (2), y, pred");

template <bool ASSIGN>
__global__ __launch_bounds__(CRYSTAL_THREADS) void structure_match_kernel(sm_side X, sm_side Y, const int32_t* __restrict__ pairs, int P,
                                                                          float ltol, float angle_tol, float stol, int max_mappings, sm_out o,
                                                                          float* d_cost) {
    const int p = blockIdx.x;
    if (p >= P) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    __shared__ float sw[3 * CRYSTAL_LDS_ATOMS], sv[3 * CRYSTAL_LDS_ATOMS];
    __shared__ int stx[CRYSTAL_LDS_ATOMS], sty[CRYSTAL_LDS_ATOMS];
    __shared__ int s_codes[ARREAU_SM_MAX_MAPPINGS_CAP];
    __shared__ int s_pm[CRYSTAL_WAVES * CRYSTAL_LDS_ATOMS];
    __shared__ int s_cnt[CRYSTAL_WAVES];
    __shared__ unsigned s_ka[CRYSTAL_WAVES], s_kb[CRYSTAL_WAVES];
    __shared__ float s_best[CRYSTAL_WAVES];
    __shared__ int s_bcode[CRYSTAL_WAVES], s_bq[CRYSTAL_WAVES], s_surv[CRYSTAL_WAVES];
    constexpr int A = ARREAU_SM_ASSIGN_LDS_ATOMS, ROWS = ARREAU_SM_ASSIGN_STATE_ROWS;
    __shared__ float s_cost[ASSIGN ? CRYSTAL_WAVES * A * (A + 1) : 1];  // (rows of A + 1: the lanes of part A write one column at a time)
    __shared__ int s_state[ASSIGN ? CRYSTAL_WAVES * ROWS * CRYSTAL_LDS_ATOMS : 1];

    const float inf = __int_as_float(0x7f800000);
    int32_t* o_partner = o.partner + (size_t)p * o.stride;
    auto no_result = [&](int flags, int n_mappings, int n_candidates) {
        if (tid == 0) {
            o.rms[p] = inf; o.rms_norm[p] = inf; o.max_dist[p] = inf; o.mapping[p] = -1;
            o.translation[3 * (size_t)p] = 0.f; o.translation[3 * (size_t)p + 1] = 0.f; o.translation[3 * (size_t)p + 2] = 0.f;
            o.n_mappings[p] = n_mappings; o.n_candidates[p] = n_candidates; o.n_permutations[p] = 0; o.matched[p] = 0; o.flags[p] = flags;
        }
        for (int k = tid; k < o.stride; k += CRYSTAL_THREADS) o_partner[k] = -1;
    };

    // ---- rule 1: BAD_PAIR before anything is read through the indices, NONFINITE alone, else CELL | EMPTY | DIFFERENT
    const int bx = pairs[2 * (size_t)p], by = pairs[2 * (size_t)p + 1];
    if (bx < 0 || bx >= X.B || by < 0 || by >= Y.B) {  // (uniform)
        no_result(ARREAU_SM_BAD_PAIR, 0, 0);
        return;
    }
    int firstx, firsty, nx, ny;
    float Lx[9], Ly[9];
    const bool badx = crystal_prologue(X.frac, X.lattice, X.offsets, bx, X.N, firstx, nx, Lx, [] {});
    const bool bady = crystal_prologue(Y.frac, Y.lattice, Y.offsets, by, Y.N, firsty, ny, Ly, [] {});
    if (nx > o.stride) {  // (uniform) a row of partner, and of scratch, cannot hold the map
        no_result(ARREAU_SM_BAD_PAIR, 0, 0);
        return;
    }
    if (badx || bady) {
        no_result(ARREAU_SM_NONFINITE, 0, 0);
        return;
    }
    const int n = nx;
    const bool staged = nx == ny && n <= CRYSTAL_LDS_ATOMS;
    if (staged) {
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) {
            sw[a] = crystal_wrap(X.frac[3 * (size_t)firstx + a]);
            sv[a] = crystal_wrap(Y.frac[3 * (size_t)firsty + a]);
        }
        for (int a = tid; a < n; a += CRYSTAL_THREADS) {
            stx[a] = X.types[(size_t)firstx + a];
            sty[a] = Y.types[(size_t)firsty + a];
        }
    }
    __syncthreads();
    auto wpos = [&](int atom, int d) -> float { return staged ? sw[3 * atom + d] : crystal_wrap(X.frac[3 * ((size_t)firstx + atom) + d]); };
    auto vpos = [&](int atom, int d) -> float { return staged ? sv[3 * atom + d] : crystal_wrap(Y.frac[3 * ((size_t)firsty + atom) + d]); };
    auto spx = [&](int atom) -> int { return staged ? stx[atom] : X.types[(size_t)firstx + atom]; };
    auto spy = [&](int atom) -> int { return staged ? sty[atom] : Y.types[(size_t)firsty + atom]; };

    int flags = 0;
    {
        const float volx = crystal_volume(Lx), voly = crystal_volume(Ly);
        if (!(volx > 0.f) || !isfinite(volx) || !(voly > 0.f) || !isfinite(voly)) flags |= ARREAU_SM_CELL;
        if (nx == 0 || ny == 0) flags |= ARREAU_SM_EMPTY;
        int differs = nx != ny;
        if (!differs)  // equal counts: the multisets agree when every species of x has as many atoms in y
            for (int i = tid; i < n; i += CRYSTAL_THREADS) {
                const int ti = spx(i);
                int cx = 0, cy = 0;
                for (int j = 0; j < n; ++j) {
                    cx += spx(j) == ti;
                    cy += spy(j) == ti;
                }
                differs |= cx != cy;
            }
        if (__syncthreads_or(differs)) flags |= ARREAU_SM_DIFFERENT;
    }
    if (flags) {
        no_result(flags, 0, 0);
        return;
    }

    // ---- rule 2 (phase 1): the lattice mappings, the first max_mappings compacted in code order
    float Gx[6], lenx[3], angx[3];
    {
        const int identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        image_metric(identity, Lx, Gx);
        metric_lengths(Gx, lenx);
#pragma unroll
        for (int i = 0; i < 3; ++i) angx[i] = metric_angle(Gx, lenx, i);
    }
    constexpr int PER = (SYM_CODES + CRYSTAL_THREADS - 1) / CRYSTAL_THREADS;
    const int code0 = tid * PER, code1 = min(code0 + PER, SYM_CODES);
    int mine = 0;
    for (int c = code0; c < code1; ++c) mine += mapping_candidate(c, Ly, lenx, angx, ltol, angle_tol) ? 1 : 0;
    int incl = mine;  // inclusive prefix over the wave's lanes, then over the waves through LDS
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_cnt[wave] = incl;
    __syncthreads();
    int n_mappings = 0, before = 0;
#pragma unroll
    for (int w = 0; w < CRYSTAL_WAVES; ++w) {
        before += w < wave ? s_cnt[w] : 0;
        n_mappings += s_cnt[w];
    }
    if (n_mappings == 0) {  // (uniform)
        no_result(ARREAU_SM_NO_MAPPING, 0, 0);
        return;
    }
    const int used = min(n_mappings, max_mappings);
    if (mine > 0) {
        int pos = before + incl - mine;
        for (int c = code0; c < code1 && pos < used; ++c)
            if (mapping_candidate(c, Ly, lenx, angx, ltol, angle_tol)) s_codes[pos++] = c;
    }

    // ---- rule 5: the rarest species of x (the same atoms of y: the multisets agree) and its first atom p0
    int p0;
    const int rare = crystal_rarest_species(n, lane, wave, spx, s_ka, s_kb, p0);
    int n_rare = 0;
    for (int j = 0; j < n; ++j) n_rare += spy(j) == rare;
    const float wp0[3] = {wpos(p0, 0), wpos(p0, 1), wpos(p0, 2)};
    __syncthreads();  // (s_codes: written above, read below by every thread)

    // ---- rules 3-6: one candidate (W, q) on this wave.  part A: the partners and the sum of the differences; part B, after a
    // barrier: the map one-to-one?  then the refined translation and the distances once more.
    int* pm = n <= CRYSTAL_LDS_ATOMS ? s_pm + wave * CRYSTAL_LDS_ATOMS : o.scratch + ((size_t)p * CRYSTAL_WAVES + wave) * o.stride;
    float V[9], Gm[6], t[3], sum[3];  // the state of the wave's candidate between part A and part B
    // rule 6b: the wave's cost matrix cm (row stride cs) and solver state st (row stride ss), each in LDS or in d_cost
    float* cm = nullptr;
    int* st = nullptr;
    int cs = 0, ss = 0;
    if constexpr (ASSIGN) {
        float* home = d_cost ? d_cost + ((size_t)p * CRYSTAL_WAVES + wave) * ((size_t)o.stride + ROWS) * o.stride : nullptr;
        if (n <= A) { cm = s_cost + wave * A * (A + 1); cs = A + 1; } else { cm = home; cs = o.stride; }
        if (n <= CRYSTAL_LDS_ATOMS) { st = s_state + wave * ROWS * CRYSTAL_LDS_ATOMS; ss = CRYSTAL_LDS_ATOMS; }
        else { st = reinterpret_cast<int*>(home + (size_t)o.stride * o.stride); ss = o.stride; }
    }
    auto mapped = [&](int j, float* y) {  // rule 3: v' = wrap(W^-1 v)
        const float v0 = vpos(j, 0), v1 = vpos(j, 1), v2 = vpos(j, 2);
#pragma unroll
        for (int r = 0; r < 3; ++r) y[r] = crystal_wrap(rot_row(V, r, v0, v1, v2));
    };
    auto lane_sum = [&](float e0, float e1, float e2, int upto, float& a0, float& a1, float& a2) {  // in atom order: lane k's value, k ascending
        for (int k = 0; k < upto; ++k) {
            a0 = __fadd_rn(a0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e0), k)));
            a1 = __fadd_rn(a1, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e1), k)));
            a2 = __fadd_rn(a2, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e2), k)));
        }
    };
    auto part_a = [&](int code, int q) {
        int Wi[9];
        const int det = decode_rotation(code, Wi);
        inverse_rotation(Wi, det, V);
        float Gy[6];
        image_metric(Wi, Ly, Gy);
#pragma unroll
        for (int e = 0; e < 6; ++e) Gm[e] = __fmul_rn(0.5f, __fadd_rn(Gx[e], Gy[e]));  // rule 4: the mean metric
        float vq[3];
        mapped(q, vq);
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = crystal_wrap(__fsub_rn(wp0[r], vq[r]));
        sum[0] = sum[1] = sum[2] = 0.f;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
            if (i < n) {
                const float x0 = wpos(i, 0), x1 = wpos(i, 1), x2 = wpos(i, 2);
                const int ti = spx(i);
                float best2 = inf;
                int best = -1;
                for (int j = 0; j < n; ++j) {  // ascending j and a strict comparison: ties go to the smallest j
                    if (spy(j) != ti) continue;
                    float y[3], e[3];
                    mapped(j, y);
                    e[0] = __fsub_rn(__fadd_rn(y[0], t[0]), x0); e[1] = __fsub_rn(__fadd_rn(y[1], t[1]), x1); e[2] = __fsub_rn(__fadd_rn(y[2], t[2]), x2);
                    const float d2 = nearest_image_d2(e, Gm);
                    if constexpr (ASSIGN) cm[(size_t)i * cs + j] = d2;
                    if (d2 < best2) { best2 = d2; best = j; b0 = e[0]; b1 = e[1]; b2 = e[2]; }
                }
                pm[i] = best;
            }
            lane_sum(b0, b1, b2, min(64, n - i0), sum[0], sum[1], sum[2]);
        }
    };
    // rule 6b: the one-to-one, species-preserving map of the smallest sum of the wave's cost matrix, into pm.  Shortest augmenting
    // paths (Jonker-Volgenant) from part A's start: column duals 0, a row keeps its nearest partner when it is the smallest row
    // that claims the column (its dual is that minimum, implicitly); the other rows are augmented in ascending order.  Columns
    // live on lanes (j = lane, lane + 64, ...), each lane owns the state of its columns; costs are round(d^2 x 2^24) as 64-bit
    // integers, so every sum and difference is exact.  Called by the whole wave.
    auto ld64 = [&](int row, int j) -> long long {
        return (long long)(((unsigned long long)(unsigned)st[(size_t)(row + 1) * ss + j] << 32) | (unsigned)st[(size_t)row * ss + j]);
    };
    auto st64 = [&](int row, int j, long long v) {
        st[(size_t)row * ss + j] = (int)(unsigned)(unsigned long long)v;
        st[(size_t)(row + 1) * ss + j] = (int)(v >> 32);
    };
    auto cost = [&](int i, int j) -> long long { return __float2ll_rn(__fmul_rn(cm[(size_t)i * cs + j], 16777216.f)); };
    auto solve = [&]() {
        int* y = st + (size_t)SM_ROW_Y * ss;
        int* pred = st + (size_t)SM_ROW_PRED * ss;
        for (int j = lane; j < n; j += 64) { y[j] = -1; st64(SM_ROW_V, j, 0); }
        crystal_wave_sync();
        for (int i = lane; i < n; i += 64) {
            const int pi = pm[i];
            bool first = pi >= 0;
            for (int k = 0; k < i; ++k) first = first && pm[k] != pi;
            if (first) y[pi] = i;
        }
        crystal_wave_sync();
        for (int i = lane; i < n; i += 64) {
            const int pi = pm[i];
            if (pi >= 0 && y[pi] != i) pm[i] = -1;
        }
        crystal_wave_sync();
        for (int f = 0; f < n; ++f) {
            if (pm[f] >= 0) continue;  // (uniform)
            const int tf = spx(f);
            for (int j = lane; j < n; j += 64) {
                const bool same = spy(j) == tf;  // another species is excluded, not made expensive
                pred[j] = same ? f : SM_EXCLUDED;
                if (same) st64(SM_ROW_D, j, cost(f, j) - ld64(SM_ROW_V, j));
            }
            int j1 = -1;
            long long mind = 0;
            for (int step = 0; step < n; ++step) {  // (every step scans one column)
                long long bd = 0x7fffffffffffffffLL;
                int bj = 0x7fffffff;
                for (int j = lane; j < n; j += 64) {  // ascending j and a strict comparison: ties go to the smallest j
                    if (pred[j] < 0) continue;
                    const long long d = ld64(SM_ROW_D, j);
                    if (d < bd) { bd = d; bj = j; }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const long long od = __shfl_xor(bd, off);
                    const int oj = __shfl_xor(bj, off);
                    if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
                }
                if (bj >= n) break;  // (not reached: the species multisets agree, a free column of the species exists)
                mind = bd;
                if (lane == (bj & 63)) pred[bj] = ~pred[bj];  // scanned
                const int i = y[bj];
                if (i < 0) { j1 = bj; break; }
                const long long h = cost(i, bj) - ld64(SM_ROW_V, bj) - mind;
                for (int j = lane; j < n; j += 64) {
                    if (pred[j] < 0) continue;
                    const long long nd = cost(i, j) - ld64(SM_ROW_V, j) - h;
                    if (nd < ld64(SM_ROW_D, j)) { st64(SM_ROW_D, j, nd); pred[j] = i; }
                }
            }
            if (j1 >= 0) {
                for (int j = lane; j < n; j += 64)
                    if (pred[j] < 0 && pred[j] != SM_EXCLUDED) st64(SM_ROW_V, j, ld64(SM_ROW_V, j) + ld64(SM_ROW_D, j) - mind);
                crystal_wave_sync();
                int j = j1;
                for (int hop = 0; hop < n; ++hop) {  // the path back to f: every row on it moves to the column it was reached from
                    const int i = ~pred[j];
                    if (i < 0 || i >= n) break;  // (not reached)
                    const int before = pm[i];
                    if (lane == 0) { y[j] = i; pm[i] = j; }
                    if (i == f || before < 0) break;
                    j = before;
                }
            }
            crystal_wave_sync();
        }
    };
    // part B: returns whether the map is a permutation (or was made one-to-one by the assignment step: `solved`); then rms2 = (sum
    // of d^2) / n and max2 = max d^2 with the refined translation
    auto part_b = [&](float& rms2, float& max2, float* refined, bool& solved) -> bool {
        int twice = 0;
        for (int i = lane; i < n; i += 64) {
            const int pi = pm[i];
            if (pi < 0) { twice = 1; continue; }
            for (int k = 0; k < i; ++k) twice |= pm[k] == pi;
        }
        solved = false;
        if (__any(twice)) {
            if constexpr (!ASSIGN) return false;
            crystal_wave_sync();  // (every lane has read the map before the solver writes it)
            solve();
            int hole = 0;
            for (int i = lane; i < n; i += 64) hole |= pm[i] < 0;
            if (__any(hole)) return false;  // (not reached)
            solved = true;
            sum[0] = sum[1] = sum[2] = 0.f;  // the differences of the chosen partners under the unrefined t: part A's operations
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                float e[3] = {0.f, 0.f, 0.f};
                if (i < n) {
                    float y[3];
                    mapped(pm[i], y);
                    e[0] = __fsub_rn(__fadd_rn(y[0], t[0]), wpos(i, 0)); e[1] = __fsub_rn(__fadd_rn(y[1], t[1]), wpos(i, 1));
                    e[2] = __fsub_rn(__fadd_rn(y[2], t[2]), wpos(i, 2));
                    nearest_image_d2(e, Gm);
                }
                lane_sum(e[0], e[1], e[2], min(64, n - i0), sum[0], sum[1], sum[2]);
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) refined[r] = __fsub_rn(t[r], __fdiv_rn(sum[r], (float)n));
        float total = 0.f, dummy1 = 0.f, dummy2 = 0.f;
        max2 = 0.f;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            float d2 = 0.f;
            if (i < n) {
                float y[3], e[3];
                mapped(pm[i], y);
                e[0] = __fsub_rn(__fadd_rn(y[0], refined[0]), wpos(i, 0)); e[1] = __fsub_rn(__fadd_rn(y[1], refined[1]), wpos(i, 1));
                e[2] = __fsub_rn(__fadd_rn(y[2], refined[2]), wpos(i, 2));
                d2 = nearest_image_d2(e, Gm);
            }
            lane_sum(d2, 0.f, 0.f, min(64, n - i0), total, dummy1, dummy2);
            max2 = fmaxf(max2, d2);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) max2 = fmaxf(max2, __shfl_xor(max2, off));
        rms2 = __fdiv_rn(total, (float)n);
        return true;
    };
    // the k-th atom of y of the rarest species, ascending
    auto kth_rare = [&](int k) -> int {
        for (int j = 0; j < n; ++j)
            if (spy(j) == rare && k-- == 0) return j;
        return -1;
    };

    // ---- phase 2: every candidate, four at a time (a uniform trip count: the barriers are met by every wave)
    const long long n_candidates = (long long)used * n_rare;
    float best_rms = inf;
    int best_code = -1, best_q = -1, survivors = 0;
    for (long long base = 0; base < n_candidates; base += CRYSTAL_WAVES) {
        const long long c = base + wave;
        const bool have = c < n_candidates;
        int code = -1, q = -1;
        if (have) {
            code = s_codes[(int)(c / n_rare)];
            q = kth_rare((int)(c % n_rare));
            part_a(code, q);
        }
        __syncthreads();  // (the partner map: written by the lanes of part A, read across lanes in part B)
        if (have) {
            float rms2, max2, refined[3];
            bool solved;
            if (part_b(rms2, max2, refined, solved)) {
                survivors += solved ? 0 : 1;  // n_permutations: the candidates whose nearest-partner map was one-to-one
                const float rms = sqrtf(rms2);
                if (rms < best_rms) { best_rms = rms; best_code = code; best_q = q; }  // (ascending (code, q) on a wave: ties keep the first)
            }
        }
        __syncthreads();  // (the map is written again in the next round)
    }

    // ---- rule 7 (phase 3): the best of the waves, ties to the smaller code, then the smaller q
    if (lane == 0) { s_best[wave] = best_rms; s_bcode[wave] = best_code; s_bq[wave] = best_q; s_surv[wave] = survivors; }
    __syncthreads();
    best_rms = inf; best_code = -1; best_q = -1; survivors = 0;
#pragma unroll
    for (int w = 0; w < CRYSTAL_WAVES; ++w) {
        survivors += s_surv[w];
        if (s_bcode[w] < 0) continue;
        const float r = s_best[w];
        if (best_code < 0 || r < best_rms || (r == best_rms && (s_bcode[w] < best_code || (s_bcode[w] == best_code && s_bq[w] < best_q)))) {
            best_rms = r; best_code = s_bcode[w]; best_q = s_bq[w];
        }
    }
    const int more = n_mappings > max_mappings ? ARREAU_SM_OVERFLOW : 0;
    if (best_code < 0) {  // (uniform) mappings, and no candidate whose nearest-partner map is a permutation
        no_result(more | ARREAU_SM_NO_PERMUTATION, n_mappings, (int)n_candidates);
        return;
    }
    if (wave == 0) part_a(best_code, best_q);
    __syncthreads();
    if (wave == 0) {
        float rms2, max2, refined[3];
        bool solved;
        part_b(rms2, max2, refined, solved);  // (a permutation, or solved again: as in phase 2)
        for (int i = lane; i < o.stride; i += 64) o_partner[i] = i < n ? pm[i] : -1;
        if (lane == 0) {
            const float rms = sqrtf(rms2);
            // det G_m, expanded along the first row; l = cbrt(sqrt(det) / n)
            const float m0 = __fsub_rn(__fmul_rn(Gm[1], Gm[2]), __fmul_rn(Gm[5], Gm[5]));
            const float m1 = __fsub_rn(__fmul_rn(Gm[3], Gm[2]), __fmul_rn(Gm[5], Gm[4]));
            const float m2 = __fsub_rn(__fmul_rn(Gm[3], Gm[5]), __fmul_rn(Gm[1], Gm[4]));
            const float detg = __fadd_rn(__fsub_rn(__fmul_rn(Gm[0], m0), __fmul_rn(Gm[3], m1)), __fmul_rn(Gm[4], m2));
            const float ell = cbrtf(__fdiv_rn(sqrtf(detg), (float)n));
            const float norm = __fdiv_rn(rms, ell);
            o.rms[p] = rms; o.rms_norm[p] = norm; o.max_dist[p] = sqrtf(max2); o.mapping[p] = best_code;
            o.translation[3 * (size_t)p] = refined[0]; o.translation[3 * (size_t)p + 1] = refined[1]; o.translation[3 * (size_t)p + 2] = refined[2];
            o.n_mappings[p] = n_mappings; o.n_candidates[p] = (int)n_candidates; o.n_permutations[p] = survivors;
            o.matched[p] = norm <= stol ? 1 : 0;  // (a NaN does not match)
            o.flags[p] = more | (solved ? ARREAU_SM_ASSIGNED : 0);
        }
    }
}

// the argument checks and the launch of both entry points; `who` names the caller in the error text
int launch_structure_match(const char* who, const float* x_frac, const int32_t* x_types, const float* x_lattice, const int32_t* x_offsets, int32_t Bx,
                           int32_t Nx, const float* y_frac, const int32_t* y_types, const float* y_lattice, const int32_t* y_offsets, int32_t By,
                           int32_t Ny, const int32_t* d_pairs, int32_t P, const arreau_structure_match_params* params,
                           arreau_structure_match_result* out, int32_t assignment, float* d_cost, void* stream) {
#define SM_REQUIRE(cond, text) ARREAU_REQUIRE(cond, std::string(who) + text)
    SM_REQUIRE(params != nullptr && out != nullptr, ": null params or result");
    SM_REQUIRE(Bx >= 0 && Nx >= 0 && By >= 0 && Ny >= 0 && P >= 0, ": bad size");
    SM_REQUIRE(std::isfinite(params->ltol) && params->ltol > 0.f, ": ltol must be finite and > 0");
    SM_REQUIRE(std::isfinite(params->angle_tol) && params->angle_tol > 0.f, ": angle_tol must be finite and > 0");
    SM_REQUIRE(std::isfinite(params->stol) && params->stol > 0.f, ": stol must be finite and > 0");
    SM_REQUIRE(params->max_mappings >= 1 && params->max_mappings <= ARREAU_SM_MAX_MAPPINGS_CAP, ": max_mappings must lie in 1..4096");
    SM_REQUIRE(assignment == ARREAU_SM_ASSIGN_NEAREST || assignment == ARREAU_SM_ASSIGN_OPTIMAL, ": assignment must be 0 (nearest) or 1 (optimal)");
    if (P == 0) return ARREAU_OK;
    SM_REQUIRE(d_pairs != nullptr, ": null pair list");
    SM_REQUIRE((x_lattice && x_offsets) || Bx == 0, ": null pointer (x)");
    SM_REQUIRE((y_lattice && y_offsets) || By == 0, ": null pointer (y)");
    SM_REQUIRE(((x_frac && x_types) || Nx == 0) && ((y_frac && y_types) || Ny == 0), ": null per-atom pointer");
    SM_REQUIRE(out->rms && out->rms_norm && out->max_dist && out->mapping && out->translation && out->n_mappings && out->n_candidates &&
                   out->n_permutations && out->matched && out->flags,
               ": null result array");
    SM_REQUIRE(out->partner_stride >= 0 && (out->partner || out->partner_stride == 0), ": null partner array or bad stride");
    SM_REQUIRE(out->scratch || out->partner_stride <= CRYSTAL_LDS_ATOMS, ": a partner_stride above 256 needs the scratch array");
    SM_REQUIRE(assignment == ARREAU_SM_ASSIGN_NEAREST || d_cost || out->partner_stride <= ARREAU_SM_ASSIGN_LDS_ATOMS,
               ": the optimal assignment with a partner_stride above ARREAU_SM_ASSIGN_LDS_ATOMS needs d_cost");
#undef SM_REQUIRE
    sm_side X{x_frac, x_types, x_lattice, x_offsets, (int)Bx, (int)Nx}, Y{y_frac, y_types, y_lattice, y_offsets, (int)By, (int)Ny};
    sm_out o{out->rms, out->rms_norm, out->max_dist, out->mapping, out->translation, out->partner, out->n_mappings, out->n_candidates,
             out->n_permutations, out->matched, out->flags, out->scratch, (int)out->partner_stride};
    if (assignment == ARREAU_SM_ASSIGN_OPTIMAL)
        ARREAU_LAUNCH(structure_match_kernel<true>, dim3((unsigned)P), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, X, Y, d_pairs, (int)P,
                      params->ltol, params->angle_tol, params->stol, (int)params->max_mappings, o, d_cost);
    else
        ARREAU_LAUNCH(structure_match_kernel<false>, dim3((unsigned)P), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, X, Y, d_pairs, (int)P,
                      params->ltol, params->angle_tol, params->stol, (int)params->max_mappings, o, (float*)nullptr);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

}  // namespace

extern "C" int arreau_structure_match(const float* x_frac, const int32_t* x_types, const float* x_lattice, const int32_t* x_offsets, int32_t Bx,
                                      int32_t Nx, const float* y_frac, const int32_t* y_types, const float* y_lattice, const int32_t* y_offsets,
                                      int32_t By, int32_t Ny, const int32_t* d_pairs, int32_t P, const arreau_structure_match_params* params,
                                      arreau_structure_match_result* out, void* stream) {
    return launch_structure_match("arreau_structure_match", x_frac, x_types, x_lattice, x_offsets, Bx, Nx, y_frac, y_types, y_lattice, y_offsets,
                                  By, Ny, d_pairs, P, params, out, ARREAU_SM_ASSIGN_NEAREST, nullptr, stream);
}

extern "C" int arreau_structure_match_assigned(const float* x_frac, const int32_t* x_types, const float* x_lattice, const int32_t* x_offsets,
                                               int32_t Bx, int32_t Nx, const float* y_frac, const int32_t* y_types, const float* y_lattice,
                                               const int32_t* y_offsets, int32_t By, int32_t Ny, const int32_t* d_pairs, int32_t P,
                                               const arreau_structure_match_params* params, arreau_structure_match_result* out, int32_t assignment,
                                               float* d_cost, void* stream) {
    return launch_structure_match("arreau_structure_match_assigned", x_frac, x_types, x_lattice, x_offsets, Bx, Nx, y_frac, y_types, y_lattice,
                                  y_offsets, By, Ny, d_pairs, P, params, out, assignment, d_cost, stream);
}
