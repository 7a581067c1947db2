// Cell reduction of a batch of crystals (arreau_crystal_reduce; the rules are written out in include/arreau_hip.h): the pure
// translations a crystal has, the primitive cell they imply, a Delaunay-reduced (Selling) basis of that cell with its shortest
// vectors, and one atom per translation class expressed in it.  One launch, one workgroup of four waves per crystal, no atomics;
// needs no arreau_model.
//   phase 1  the candidate translations (the atoms q of the rarest species, in rounds of up to 256) dealt to the waves as in
//            symfind.hip for W = I; the residual takes the minimum over the 27 neighbouring images; the accepted ones are
//            compacted in q order; their closure is tested pair by pair;
//   phase 2  the vector set (a, b, c and the translations' shortest images, as integer numerators over m) is ranked by length,
//            the pairs (i, j) of the sorted list are dealt to the threads, each looks for its first k that passes the volume test,
//            a minimum over the workgroup gives the first triple in lexicographic order;
//   phase 3  thread 0 runs the Selling steps on integers (every vector is formed again from its numerators: nothing accumulates)
//            and takes the three shortest independent vectors;
//   phase 4  the atoms in rounds of 256: an atom is kept when none of its translated images lands on an atom before it.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

#define RED_ROUND CRYSTAL_THREADS
#define RED_MAX_VEC (3 + ARREAU_RED_MAX_TRANSLATIONS)

namespace {

struct red_out {
    int32_t *multiplicity, *n_translations;
    float *lattice_out, *transform;
    int32_t *n_out, *flags, *selling_steps;
    float* frac_out;
    int32_t *types_out, *keep;
};

// rule 2's distance: each component minus its nearest integer, then the shortest of the 27 images e + s, s in {-1, 0, 1}^3
__device__ __forceinline__ float min_image_d2(float d0, float d1, float d2, const float* Lm) {
    d0 = __fsub_rn(d0, rintf(d0)); d1 = __fsub_rn(d1, rintf(d1)); d2 = __fsub_rn(d2, rintf(d2));
    float best = __int_as_float(0x7f800000);
    for (int s0 = -1; s0 <= 1; ++s0)
        for (int s1 = -1; s1 <= 1; ++s1)
#pragma unroll
            for (int s2 = -1; s2 <= 1; ++s2)
                best = fminf(best, crystal_frac_d2(__fadd_rn(d0, (float)s0), __fadd_rn(d1, (float)s1), __fadd_rn(d2, (float)s2), Lm));
    return best;
}

// the Cartesian vector of integer numerators over m: coefficients num_k / m, then (c_0 L_0d + c_1 L_1d) + c_2 L_2d
__device__ __forceinline__ void num_cart(const int* num, float mf, const float* Lm, float* v) {
    const float c0 = __fdiv_rn((float)num[0], mf), c1 = __fdiv_rn((float)num[1], mf), c2 = __fdiv_rn((float)num[2], mf);
#pragma unroll
    for (int d = 0; d < 3; ++d) v[d] = rows_rn(Lm, d, c0, c1, c2);
}

__device__ __forceinline__ float det3_rn(const float* a, const float* b, const float* c) {
    float x[3];
    cross_rn(b, c, x);
    return dot3_rn(a[0], a[1], a[2], x[0], x[1], x[2]);
}

__device__ __forceinline__ long long idet3(const int* a, const int* b, const int* c) {
    return (long long)a[0] * ((long long)b[1] * c[2] - (long long)b[2] * c[1]) - (long long)a[1] * ((long long)b[0] * c[2] - (long long)b[2] * c[0]) +
           (long long)a[2] * ((long long)b[0] * c[1] - (long long)b[1] * c[0]);
}

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_reduce_kernel(
    const float* __restrict__ frac, const int32_t* __restrict__ types, const float* __restrict__ lattice,
    const int32_t* __restrict__ offsets, int B, int N, float symprec, red_out o) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float sw[3 * CRYSTAL_LDS_ATOMS];
    __shared__ int sty[CRYSTAL_LDS_ATOMS];
    __shared__ int s_q[RED_ROUND];
    __shared__ float s_res[RED_ROUND];
    __shared__ int s_cnt[CRYSTAL_WAVES];
    __shared__ unsigned s_ka[CRYSTAL_WAVES], s_kb[CRYSTAL_WAVES];
    __shared__ int s_tq[ARREAU_RED_MAX_TRANSLATIONS];  // the atom q of every accepted translation, ascending
    __shared__ int s_num[3 * RED_MAX_VEC];             // the vector set: integer numerators over m in the input basis
    __shared__ float s_vec[3 * RED_MAX_VEC], s_len2[RED_MAX_VEC];
    __shared__ int s_sorted[RED_MAX_VEC];
    __shared__ int s_c[7 * 3];   // phase 3: the four Selling vectors, then the seven candidates, in the primitive basis
    __shared__ float s_l7[7];
    __shared__ int s_red[9], s_steps;  // the reduced basis: numerators over m in the input basis

    // a crystal nothing is done to: the inputs' bits, identity transform, multiplicity 1 (every output slot is written)
    auto copy_through = [&](int flags, int n_translations) {
        const int32_t* fin = reinterpret_cast<const int32_t*>(frac);
        int32_t* fout = reinterpret_cast<int32_t*>(o.frac_out);
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) fout[3 * (size_t)first + a] = fin[3 * (size_t)first + a];
        for (int a = tid; a < n; a += CRYSTAL_THREADS) {
            o.types_out[(size_t)first + a] = types[(size_t)first + a];
            o.keep[(size_t)first + a] = a;
        }
        if (tid < 9) {
            reinterpret_cast<int32_t*>(o.lattice_out)[9 * (size_t)b + tid] = reinterpret_cast<const int32_t*>(lattice)[9 * (size_t)b + tid];
            o.transform[9 * (size_t)b + tid] = tid % 4 == 0 ? 1.f : 0.f;
        }
        if (tid == 0) {
            o.multiplicity[b] = 1; o.n_translations[b] = n_translations; o.n_out[b] = n;
            o.flags[b] = flags; o.selling_steps[b] = 0;
        }
    };

    // ---- rule 1: NONFINITE, CELL, EMPTY (workgroup-uniform)
    if (bad) {
        copy_through(ARREAU_RED_NONFINITE, 0);
        return;
    }
    const float volume = crystal_volume(Lm);
    const int early = ((!(volume > 0.f) || !isfinite(volume)) ? ARREAU_RED_CELL : 0) | (n == 0 ? ARREAU_RED_EMPTY : 0);
    if (early) {
        copy_through(early, 0);
        return;
    }

    // ---- positions and species: staged in LDS when the crystal fits, else read where they are used (the same values)
    const bool staged = n <= CRYSTAL_LDS_ATOMS;
    if (staged) {
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) sw[a] = crystal_wrap(frac[3 * (size_t)first + a]);
        for (int a = tid; a < n; a += CRYSTAL_THREADS) sty[a] = types[(size_t)first + a];
    }
    __syncthreads();
    auto wpos = [&](int atom, int d) -> float { return staged ? sw[3 * atom + d] : crystal_wrap(frac[3 * ((size_t)first + atom) + d]); };
    auto species = [&](int atom) -> int { return staged ? sty[atom] : types[(size_t)first + atom]; };

    // ---- rule 2 (phase 1): the candidate translations t = wrap(w_q - w_p0), q over the rarest species, ascending
    int p0;
    const int rare = crystal_rarest_species(n, lane, wave, species, s_ka, s_kb, p0);
    const float wp0[3] = {wpos(p0, 0), wpos(p0, 1), wpos(p0, 2)};
    auto translation = [&](int q, int d) -> float { return crystal_wrap(__fsub_rn(wpos(q, d), wp0[d])); };
    // the atom of the species of i nearest to y (ties to the lower index) and its squared distance
    auto partner = [&](int ti, float y0, float y1, float y2, float& best) -> int {
        int at = -1;
        best = __int_as_float(0x7f800000);
        for (int j = 0; j < n; ++j) {
            if (species(j) != ti) continue;
            const float d2 = min_image_d2(__fsub_rn(y0, wpos(j, 0)), __fsub_rn(y1, wpos(j, 1)), __fsub_rn(y2, wpos(j, 2)), Lm);
            if (d2 < best || at < 0) { best = d2; at = j; }
        }
        return at;
    };
    const int n_rounds = (n + RED_ROUND - 1) / RED_ROUND;
    int total = 0, nq = 0;
    for (int round = 0; round < n_rounds; ++round) {
        const int a = round * RED_ROUND + tid;
        const bool is = a < n && species(a) == rare;
        const int at = crystal_compact(is, lane, wave, s_cnt, nq);
        if (is) s_q[at] = a;
        __syncthreads();
        for (int k = wave; k < nq; k += CRYSTAL_WAVES) {
            const int q = s_q[k];
            const float t0 = translation(q, 0), t1 = translation(q, 1), t2 = translation(q, 2);
            float worst2 = 0.f;
            bool alive = true;
            for (int i0 = 0; i0 < n && alive; i0 += 64) {
                const int i = i0 + lane;
                float m2 = 0.f;  // (a lane without an atom does not raise the maximum)
                if (i < n) partner(species(i), __fadd_rn(wpos(i, 0), t0), __fadd_rn(wpos(i, 1), t1), __fadd_rn(wpos(i, 2), t2), m2);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) m2 = fmaxf(m2, __shfl_xor(m2, off));
                worst2 = fmaxf(worst2, m2);
                alive = sqrtf(worst2) <= symprec;
            }
            if (lane == 0) s_res[k] = alive ? 1.f : -1.f;
        }
        __syncthreads();
        const bool acc = tid < nq && s_res[tid] >= 0.f;
        int accepted;
        const int slot = total + crystal_compact(acc, lane, wave, s_cnt, accepted);
        if (acc && slot < ARREAU_RED_MAX_TRANSLATIONS) s_tq[slot] = s_q[tid];
        total += accepted;
        __syncthreads();  // s_q, s_res and s_cnt are written again in the next round
    }
    // (q = p0 comes first and has t = 0, residual 0: total >= 1 and translation 0 is the identity)
    const int m = total;
    if (m > ARREAU_RED_MAX_TRANSLATIONS || n % m != 0) {  // (uniform)
        copy_through(ARREAU_RED_AMBIGUOUS, total);
        return;
    }
    // closure: every sum t_a + t_b lies within symprec of an accepted t_c
    int open = 0;
    for (int p = tid; p < m * m; p += CRYSTAL_THREADS) {
        const int qa = s_tq[p / m], qb = s_tq[p % m];
        const float u0 = __fadd_rn(translation(qa, 0), translation(qb, 0)), u1 = __fadd_rn(translation(qa, 1), translation(qb, 1)),
                    u2 = __fadd_rn(translation(qa, 2), translation(qb, 2));
        bool found = false;
        for (int c = 0; c < m && !found; ++c) {
            const int qc = s_tq[c];
            found = sqrtf(min_image_d2(__fsub_rn(u0, translation(qc, 0)), __fsub_rn(u1, translation(qc, 1)), __fsub_rn(u2, translation(qc, 2)), Lm)) <= symprec;
        }
        open |= !found;
    }
    if (__syncthreads_or(open)) {
        copy_through(ARREAU_RED_AMBIGUOUS, total);
        return;
    }

    // ---- rule 3 (phase 2): the vector set, ranked by length; the first triple of the primitive volume
    const float mf = (float)m;
    const int K = 3 + (m - 1);
    if (tid < K) {
        int num[3];
        float v[3];
        if (tid < 3) {
            num[0] = tid == 0 ? m : 0; num[1] = tid == 1 ? m : 0; num[2] = tid == 2 ? m : 0;
            num_cart(num, mf, Lm, v);
        } else {
            const int q = s_tq[tid - 2];
            int base[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float t = translation(q, d);
                base[d] = (int)rintf(__fmul_rn(mf, __fsub_rn(t, rintf(t))));  // m t is an integer vector in a group of order m
            }
            float best = __int_as_float(0x7f800000);
            for (int s0 = -1; s0 <= 1; ++s0)
                for (int s1 = -1; s1 <= 1; ++s1)
                    for (int s2 = -1; s2 <= 1; ++s2) {
                        const int cand[3] = {base[0] + s0 * m, base[1] + s1 * m, base[2] + s2 * m};
                        float cv[3];
                        num_cart(cand, mf, Lm, cv);
                        const float l2 = dot3_rn(cv[0], cv[1], cv[2], cv[0], cv[1], cv[2]);
                        if (l2 < best) {  // ties: the first image in lexicographic order
                            best = l2;
#pragma unroll
                            for (int d = 0; d < 3; ++d) { num[d] = cand[d]; v[d] = cv[d]; }
                        }
                    }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) { s_num[3 * tid + d] = num[d]; s_vec[3 * tid + d] = v[d]; }
        s_len2[tid] = dot3_rn(v[0], v[1], v[2], v[0], v[1], v[2]);
    }
    __syncthreads();
    if (tid < K) {
        int rank = 0;
        const float mine = s_len2[tid];
        for (int u = 0; u < K; ++u) rank += (s_len2[u] < mine || (s_len2[u] == mine && u < tid)) ? 1 : 0;
        s_sorted[rank] = tid;
    }
    __syncthreads();
    const float target = __fdiv_rn(volume, mf), slack = __fdiv_rn(volume, __fmul_rn(4.f, mf));
    unsigned key = 0xffffffffu;  // (i K + j) K + k of the thread's first passing triple
    for (int p = tid; p < K * K; p += CRYSTAL_THREADS) {
        const int i = p / K, j = p % K;
        if (i >= j) continue;
        const float *vi = s_vec + 3 * s_sorted[i], *vj = s_vec + 3 * s_sorted[j];
        for (int k = j + 1; k < K; ++k) {
            const float det = det3_rn(vi, vj, s_vec + 3 * s_sorted[k]);
            if (fabsf(__fsub_rn(fabsf(det), target)) <= slack) {
                key = min(key, (unsigned)((i * K + j) * K + k));
                break;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) key = min(key, (unsigned)__shfl_xor(key, off));
    if (lane == 0) s_ka[wave] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < CRYSTAL_WAVES; ++w) key = min(key, s_ka[w]);
    if (key == 0xffffffffu) {  // (uniform)
        copy_through(ARREAU_RED_AMBIGUOUS, total);
        return;
    }

    // ---- rule 4 (phase 3): Selling steps and the three shortest independent vectors, on thread 0
    if (tid == 0) {
        int prim[9];  // the primitive basis: numerators over m in the input basis, right-handed
        const int tri[3] = {s_sorted[(int)(key / (unsigned)(K * K))], s_sorted[(int)(key / (unsigned)K) % K], s_sorted[(int)(key % (unsigned)K)]};
        const float det = det3_rn(s_vec + 3 * tri[0], s_vec + 3 * tri[1], s_vec + 3 * tri[2]);
        for (int r = 0; r < 3; ++r)
            for (int d = 0; d < 3; ++d) prim[3 * r + d] = det < 0.f ? -s_num[3 * tri[r] + d] : s_num[3 * tri[r] + d];
        // a vector with coefficients c in the primitive basis: numerators c . prim, then num_cart
        auto cart_of = [&](const int* c, float* v) {
            const int num[3] = {c[0] * prim[0] + c[1] * prim[3] + c[2] * prim[6], c[0] * prim[1] + c[1] * prim[4] + c[2] * prim[7],
                                c[0] * prim[2] + c[1] * prim[5] + c[2] * prim[8]};
            num_cart(num, mf, Lm, v);
        };
        for (int r = 0; r < 4; ++r)
            for (int d = 0; d < 3; ++d) s_c[3 * r + d] = r < 3 ? (r == d ? 1 : 0) : -1;
        float longest2 = 0.f;
        for (int r = 0; r < 3; ++r) {
            float v[3];
            cart_of(s_c + 3 * r, v);
            longest2 = fmaxf(longest2, dot3_rn(v[0], v[1], v[2], v[0], v[1], v[2]));
        }
        const float tol = __fmul_rn(1e-5f, longest2);
        const int PI[6] = {0, 0, 0, 1, 1, 2}, PJ[6] = {1, 2, 3, 2, 3, 3}, PK[6] = {2, 1, 1, 0, 0, 0}, PL[6] = {3, 3, 2, 3, 2, 1};
        int steps = 0;
        while (steps < ARREAU_RED_MAX_STEPS) {
            float v[12];
            for (int r = 0; r < 4; ++r) cart_of(s_c + 3 * r, v + 3 * r);
            int e = 0;
            for (; e < 6; ++e)
                if (dot3_rn(v[3 * PI[e]], v[3 * PI[e] + 1], v[3 * PI[e] + 2], v[3 * PJ[e]], v[3 * PJ[e] + 1], v[3 * PJ[e] + 2]) > tol) break;
            if (e == 6) break;
            for (int d = 0; d < 3; ++d) {  // v_k += v_i, v_l += v_i, v_i = -v_i: the sum stays zero, v_i . v_j changes sign
                const int ci = s_c[3 * PI[e] + d];
                s_c[3 * PK[e] + d] += ci; s_c[3 * PL[e] + d] += ci; s_c[3 * PI[e] + d] = -ci;
            }
            ++steps;
        }
        for (int d = 0; d < 3; ++d) {  // candidates 4, 5, 6: a + b, b + c, c + a
            const int ca = s_c[d], cb = s_c[3 + d], cc = s_c[6 + d];
            s_c[12 + d] = ca + cb; s_c[15 + d] = cb + cc; s_c[18 + d] = cc + ca;
        }
        for (int r = 0; r < 7; ++r) {
            float v[3];
            cart_of(s_c + 3 * r, v);
            s_l7[r] = dot3_rn(v[0], v[1], v[2], v[0], v[1], v[2]);
        }
        int order[7];
        for (int r = 0; r < 7; ++r) {
            int rank = 0;
            for (int u = 0; u < 7; ++u) rank += (s_l7[u] < s_l7[r] || (s_l7[u] == s_l7[r] && u < r)) ? 1 : 0;
            order[rank] = r;
        }
        // the three shortest that are independent, decided on the integers (the seven span the lattice: a third one exists)
        int pick[3] = {order[0], -1, -1};
        for (int x = 1; x < 7; ++x) {
            const int* c0 = s_c + 3 * pick[0];
            const int* cx = s_c + 3 * order[x];
            if (pick[1] < 0) {
                const bool parallel = c0[1] * cx[2] - c0[2] * cx[1] == 0 && c0[2] * cx[0] - c0[0] * cx[2] == 0 && c0[0] * cx[1] - c0[1] * cx[0] == 0;
                if (!parallel) pick[1] = order[x];
            } else if (pick[2] < 0 && idet3(c0, s_c + 3 * pick[1], cx) != 0) {
                pick[2] = order[x];
            }
        }
        if (pick[1] < 0) pick[1] = pick[0];  // (unreachable for a basis; det 0 below then flags the crystal)
        if (pick[2] < 0) pick[2] = pick[0];
        const int sign = idet3(s_c + 3 * pick[0], s_c + 3 * pick[1], s_c + 3 * pick[2]) < 0 ? -1 : 1;
        for (int r = 0; r < 3; ++r) {
            const int* c = s_c + 3 * pick[r];
            for (int d = 0; d < 3; ++d) s_red[3 * r + d] = sign * (c[0] * prim[d] + c[1] * prim[3 + d] + c[2] * prim[6 + d]);
        }
        s_steps = steps;
    }
    __syncthreads();
    int R[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = s_red[q];
    const int steps = s_steps;
    // T = R / m expresses the reduced basis in the input basis, det T = 1 / m: det R = m^2, and T^-1 = adj(R) / m is an integer matrix Q
    const long long detR = idet3(R, R + 3, R + 6);
    int Q[9];
    Q[0] = R[4] * R[8] - R[5] * R[7]; Q[1] = R[2] * R[7] - R[1] * R[8]; Q[2] = R[1] * R[5] - R[2] * R[4];
    Q[3] = R[5] * R[6] - R[3] * R[8]; Q[4] = R[0] * R[8] - R[2] * R[6]; Q[5] = R[2] * R[3] - R[0] * R[5];
    Q[6] = R[3] * R[7] - R[4] * R[6]; Q[7] = R[1] * R[6] - R[0] * R[7]; Q[8] = R[0] * R[4] - R[1] * R[3];
    bool whole = detR == (long long)m * m;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        whole = whole && Q[q] % m == 0;
        Q[q] /= m;
    }
    if (!whole) {  // (uniform) the snapped translations do not span a lattice of index m
        copy_through(ARREAU_RED_AMBIGUOUS, total);
        return;
    }

    // ---- rule 5 (phase 4): one atom per translation class, the lowest index; x_red = w Q (row vector), wrapped
    const int n_out = n / m;
    int kept = 0;
    for (int round = 0; round < n_rounds; ++round) {
        const int a = round * RED_ROUND + tid;
        bool rep = a < n;
        if (rep) {
            const int ta = species(a);
            const float x0 = wpos(a, 0), x1 = wpos(a, 1), x2 = wpos(a, 2);
            for (int k = 1; k < m && rep; ++k) {
                const int q = s_tq[k];
                float d2;
                rep = partner(ta, __fadd_rn(x0, translation(q, 0)), __fadd_rn(x1, translation(q, 1)), __fadd_rn(x2, translation(q, 2)), d2) >= a;
            }
        }
        int found;
        const int slot = kept + crystal_compact(rep, lane, wave, s_cnt, found);
        if (rep && slot < n) {
            const float x0 = wpos(a, 0), x1 = wpos(a, 1), x2 = wpos(a, 2);
            float* fo = o.frac_out + 3 * ((size_t)first + slot);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                fo[c] = crystal_wrap(__fadd_rn(__fadd_rn(__fmul_rn(x0, (float)Q[c]), __fmul_rn(x1, (float)Q[3 + c])), __fmul_rn(x2, (float)Q[6 + c])));
            o.types_out[(size_t)first + slot] = species(a);
            o.keep[(size_t)first + slot] = a;
        }
        kept += found;
        __syncthreads();  // s_cnt is written again in the next round
    }
    if (kept != n_out) {  // (uniform) the classes are not all of size m; the slots written above are written again
        __threadfence_block();
        __syncthreads();
        copy_through(ARREAU_RED_AMBIGUOUS, total);
        return;
    }
    for (int a = n_out + tid; a < n; a += CRYSTAL_THREADS) {
        o.frac_out[3 * ((size_t)first + a)] = 0.f; o.frac_out[3 * ((size_t)first + a) + 1] = 0.f; o.frac_out[3 * ((size_t)first + a) + 2] = 0.f;
        o.types_out[(size_t)first + a] = -1;
        o.keep[(size_t)first + a] = -1;
    }
    if (tid < 3) {
        const float c0 = __fdiv_rn((float)R[3 * tid], mf), c1 = __fdiv_rn((float)R[3 * tid + 1], mf), c2 = __fdiv_rn((float)R[3 * tid + 2], mf);
        float* T = o.transform + 9 * (size_t)b + 3 * tid;
        T[0] = c0; T[1] = c1; T[2] = c2;
#pragma unroll
        for (int d = 0; d < 3; ++d) o.lattice_out[9 * (size_t)b + 3 * tid + d] = rows_rn(Lm, d, c0, c1, c2);
    }
    if (tid == 0) {
        o.multiplicity[b] = m; o.n_translations[b] = total; o.n_out[b] = n_out;
        o.flags[b] = steps >= ARREAU_RED_MAX_STEPS ? ARREAU_RED_NOT_CONVERGED : 0;
        o.selling_steps[b] = steps;
    }
}

}  // namespace

extern "C" int arreau_crystal_reduce(const float* d_frac, const int32_t* d_types, const float* d_lattice, const int32_t* d_crystal_offsets,
                                     int32_t B, int32_t N, const arreau_reduce_params* params, arreau_reduce_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_reduce: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_reduce: bad size");
    ARREAU_REQUIRE(std::isfinite(params->symprec) && params->symprec > 0.f, "arreau_crystal_reduce: symprec must be finite and > 0");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_types) || N == 0), "arreau_crystal_reduce: null pointer");
    ARREAU_REQUIRE(out->multiplicity && out->n_translations && out->lattice_out && out->transform && out->n_out && out->flags &&
                       out->selling_steps && ((out->frac_out && out->types_out && out->keep) || N == 0),
                   "arreau_crystal_reduce: null result array");
    red_out o{out->multiplicity, out->n_translations, out->lattice_out, out->transform, out->n_out, out->flags, out->selling_steps,
              out->frac_out, out->types_out, out->keep};
    ARREAU_LAUNCH(crystal_reduce_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_types, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, params->symprec, o);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
