// Symmetry search of a batch of crystals (arreau_crystal_symmetry; the rules are written out in include/arreau_hip.h): the
// operations x' = W x + t a crystal has in the cell it is given, W an integer matrix with entries in {-1, 0, 1}, and the point
// group of their rotations.  One launch, one workgroup of four waves per crystal, no atomics; needs no arreau_model.
//   phase 1  the 3^9 rotation codes in contiguous ranges of 77 per thread: count the lattice isometries, one prefix scan over
//            the workgroup, then the threads that found some evaluate their range again and write the codes in code order;
//   phase 2  per surviving W, the candidate translations (the atoms q of the rarest species, in rounds of up to 256) dealt to
//            the waves; the lanes run over the atoms i, each takes the minimum over the partners j, a wave reduction takes the
//            maximum; the residuals of a round land in LDS and the accepted ones are compacted in (code, q) order by ballots;
//   phase 3  the counts per rotation type, one 6-bit field each, are compared with the 32 rows of symfind_table.h.
#include "internal.h"
#include "crystal_dev.h"
#include "symfind_table.h"
#include <cmath>

#define SYM_ROUND CRYSTAL_THREADS  // candidate translations per round: one compaction pass of the workgroup
#define SYM_IDENTITY 16484
#define SYM_MAX_LATTICE 48

namespace {

struct sym_out {
    int32_t *n_lattice, *n_ops, *n_translations, *ops_rotation;
    float *ops_translation, *ops_residual, *residual;
    int32_t *point_group, *flags;
};

// rule 2: is the code a lattice isometry within symprec?  G = (G_01, G_02, G_12), len = |a_i|
__device__ bool lattice_candidate(int code, const float* Lm, const float* G, const float* len, float symprec) {
    int W[9];
    const int det = decode_rotation(code, W);
    if (det != 1 && det != -1) return false;
    float img[9];  // img[3 j + d]: component d of a'_j = (W_0j a_0 + W_1j a_1) + W_2j a_2
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int d = 0; d < 3; ++d)
            img[3 * j + d] = __fadd_rn(__fadd_rn(__fmul_rn((float)W[j], Lm[d]), __fmul_rn((float)W[3 + j], Lm[3 + d])),
                                       __fmul_rn((float)W[6 + j], Lm[6 + d]));
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float g = dot3_rn(img[3 * i], img[3 * i + 1], img[3 * i + 2], img[3 * i], img[3 * i + 1], img[3 * i + 2]);
        ok = ok && fabsf(__fsub_rn(sqrtf(g), len[i])) <= symprec;  // (a NaN fails)
    }
    const int pi[3] = {0, 0, 1}, pj[3] = {1, 2, 2};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int i = pi[e], j = pj[e];
        const float g = dot3_rn(img[3 * i], img[3 * i + 1], img[3 * i + 2], img[3 * j], img[3 * j + 1], img[3 * j + 2]);
        const float tol = __fmul_rn(symprec, __fmul_rn(0.5f, __fadd_rn(len[i], len[j])));
        ok = ok && fabsf(__fsub_rn(g, G[e])) <= tol;
    }
    return ok;
}

// the index into the count vector (1, 2, 3, 4, 6, -1, m, -3, -4, -6) of a rotation of finite order, from det and trace; -1: none
__device__ __forceinline__ int rotation_type(int det, int trace) {
    if (det == 1) return trace == 3 ? 0 : (trace >= -1 && trace <= 2 ? trace + 2 : -1);
    return trace >= -3 && trace <= 1 ? (trace == -3 ? 5 : 7 - trace) : -1;
}

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_symmetry_kernel(
    const float* __restrict__ frac, const int32_t* __restrict__ types, const float* __restrict__ lattice,
    const int32_t* __restrict__ offsets, int B, int N, float symprec, int max_ops, sym_out o) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float sw[3 * CRYSTAL_LDS_ATOMS];
    __shared__ int sty[CRYSTAL_LDS_ATOMS];
    __shared__ int s_codes[SYM_MAX_LATTICE];
    __shared__ int s_q[SYM_ROUND];
    __shared__ float s_res[SYM_ROUND];
    __shared__ int s_cnt[CRYSTAL_WAVES];
    __shared__ unsigned s_ka[CRYSTAL_WAVES], s_kb[CRYSTAL_WAVES];
    __shared__ float s_max[CRYSTAL_WAVES];

    int32_t* o_rot = o.ops_rotation + (size_t)b * max_ops;
    float* o_trans = o.ops_translation + 3 * (size_t)b * max_ops;
    float* o_res = o.ops_residual + (size_t)b * max_ops;
    const float qnan = __int_as_float(0x7fc00000);
    auto clear_ops = [&](int from) {  // the slots no operation was stored in
        for (int k = from + tid; k < max_ops; k += CRYSTAL_THREADS) {
            o_rot[k] = -1; o_res[k] = 0.f;
            o_trans[3 * (size_t)k] = 0.f; o_trans[3 * (size_t)k + 1] = 0.f; o_trans[3 * (size_t)k + 2] = 0.f;
        }
    };
    auto no_result = [&](int flags, int n_lattice) {
        if (tid == 0) {
            o.n_lattice[b] = n_lattice; o.n_ops[b] = 0; o.n_translations[b] = 0;
            o.residual[b] = qnan; o.point_group[b] = -1; o.flags[b] = flags;
        }
        clear_ops(0);
    };

    // ---- rule 1: NONFINITE, CELL, EMPTY (workgroup-uniform; nothing else is computed)
    if (bad) {
        no_result(ARREAU_SYM_NONFINITE, 0);
        return;
    }
    const float volume = crystal_volume(Lm);
    const int early = ((!(volume > 0.f) || !isfinite(volume)) ? ARREAU_SYM_CELL : 0) | (n == 0 ? ARREAU_SYM_EMPTY : 0);
    if (early) {
        no_result(early, 0);
        return;
    }

    // ---- rule 2 (phase 1): the lattice candidates, compacted in code order
    float len[3], G[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) len[i] = sqrtf(dot3_rn(Lm[3 * i], Lm[3 * i + 1], Lm[3 * i + 2], Lm[3 * i], Lm[3 * i + 1], Lm[3 * i + 2]));
    G[0] = dot3_rn(Lm[0], Lm[1], Lm[2], Lm[3], Lm[4], Lm[5]);
    G[1] = dot3_rn(Lm[0], Lm[1], Lm[2], Lm[6], Lm[7], Lm[8]);
    G[2] = dot3_rn(Lm[3], Lm[4], Lm[5], Lm[6], Lm[7], Lm[8]);
    constexpr int PER = (SYM_CODES + CRYSTAL_THREADS - 1) / CRYSTAL_THREADS;
    const int code0 = tid * PER, code1 = min(code0 + PER, SYM_CODES);
    int mine = 0;
    for (int c = code0; c < code1; ++c) mine += lattice_candidate(c, Lm, G, len, symprec) ? 1 : 0;
    int incl = mine;  // inclusive prefix over the wave's lanes, then over the waves through LDS
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_cnt[wave] = incl;
    __syncthreads();
    int n_lattice = 0, before = 0;
#pragma unroll
    for (int w = 0; w < CRYSTAL_WAVES; ++w) {
        before += w < wave ? s_cnt[w] : 0;
        n_lattice += s_cnt[w];
    }
    if (n_lattice > SYM_MAX_LATTICE) {  // (uniform) symprec is too loose for this cell
        no_result(ARREAU_SYM_AMBIGUOUS, n_lattice);
        return;
    }
    if (mine > 0) {  // at most 48 threads: the same evaluation again, now with a place to write to
        int pos = before + incl - mine;
        for (int c = code0; c < code1; ++c)
            if (lattice_candidate(c, Lm, G, len, symprec)) s_codes[pos++] = c;
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

    // ---- rule 3: the rarest species (fewest atoms, then the smallest id) and its first atom p0
    int p0;
    const int rare = crystal_rarest_species(n, lane, wave, species, s_ka, s_kb, p0);
    const float wp0[3] = {wpos(p0, 0), wpos(p0, 1), wpos(p0, 2)};

    // ---- rules 3-5 (phase 2): every (W, q), W in code order, q ascending
    const int n_rounds = (n + SYM_ROUND - 1) / SYM_ROUND;
    int total = 0, n_translations = 0, distinct = 0, nq = 0, odd_type = 0;
    unsigned long long hist = 0;  // ten 6-bit counters, type k at bit 6 k (a lattice has at most 48 isometries)
    float worst = 0.f;
    for (int wi = 0; wi < n_lattice; ++wi) {
        const int code = s_codes[wi];
        int Wi[9];
        const int det = decode_rotation(code, Wi);
        float W[9];
#pragma unroll
        for (int p = 0; p < 9; ++p) W[p] = (float)Wi[p];
        const float Wp0[3] = {rot_row(W, 0, wp0[0], wp0[1], wp0[2]), rot_row(W, 1, wp0[0], wp0[1], wp0[2]), rot_row(W, 2, wp0[0], wp0[1], wp0[2])};
        auto translation = [&](int q, int d) -> float { return crystal_wrap(__fsub_rn(wpos(q, d), Wp0[d])); };
        const int total_before = total;
        for (int round = 0; round < n_rounds; ++round) {
            if (n_rounds > 1 || wi == 0) {  // (uniform) the rarest species' atoms of this round, ascending: one list serves every W
                const int a = round * SYM_ROUND + tid;
                const bool is = a < n && species(a) == rare;
                const int at = crystal_compact(is, lane, wave, s_cnt, nq);
                if (is) s_q[at] = a;
                __syncthreads();
            }
            // the round's pairs dealt to the waves: residual = max over i of min over j of the same species
            for (int k = wave; k < nq; k += CRYSTAL_WAVES) {
                const int q = s_q[k];
                const float t0 = translation(q, 0), t1 = translation(q, 1), t2 = translation(q, 2);
                float worst2 = 0.f;
                bool alive = true;
                for (int i0 = 0; i0 < n && alive; i0 += 64) {
                    const int i = i0 + lane;
                    float m2 = 0.f;  // (a lane without an atom does not raise the maximum)
                    if (i < n) {
                        const float x0 = wpos(i, 0), x1 = wpos(i, 1), x2 = wpos(i, 2);
                        const float y0 = __fadd_rn(rot_row(W, 0, x0, x1, x2), t0), y1 = __fadd_rn(rot_row(W, 1, x0, x1, x2), t1),
                                    y2 = __fadd_rn(rot_row(W, 2, x0, x1, x2), t2);
                        const int ti = species(i);
                        m2 = __int_as_float(0x7f800000);
                        // the residual is the minimum over j: the loop is finished even after a partner within symprec
                        for (int j = 0; j < n; ++j) {
                            if (species(j) != ti) continue;
                            float d0 = __fsub_rn(y0, wpos(j, 0)), d1 = __fsub_rn(y1, wpos(j, 1)), d2 = __fsub_rn(y2, wpos(j, 2));
                            d0 = __fsub_rn(d0, rintf(d0)); d1 = __fsub_rn(d1, rintf(d1)); d2 = __fsub_rn(d2, rintf(d2));
                            const float cx = __fadd_rn(__fadd_rn(__fmul_rn(d0, Lm[0]), __fmul_rn(d1, Lm[3])), __fmul_rn(d2, Lm[6]));
                            const float cy = __fadd_rn(__fadd_rn(__fmul_rn(d0, Lm[1]), __fmul_rn(d1, Lm[4])), __fmul_rn(d2, Lm[7]));
                            const float cz = __fadd_rn(__fadd_rn(__fmul_rn(d0, Lm[2]), __fmul_rn(d1, Lm[5])), __fmul_rn(d2, Lm[8]));
                            m2 = fminf(m2, dot3_rn(cx, cy, cz, cx, cy, cz));
                        }
                    }
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) m2 = fmaxf(m2, __shfl_xor(m2, off));
                    worst2 = fmaxf(worst2, m2);
                    alive = sqrtf(worst2) <= symprec;  // an atom without a partner within symprec: the operation is abandoned
                }
                if (lane == 0) s_res[k] = alive ? sqrtf(worst2) : -1.f;
            }
            __syncthreads();
            // the accepted operations of the round, compacted in q order (nq <= SYM_ROUND: one pass)
            const bool acc = tid < nq && s_res[tid] >= 0.f;
            const float res = acc ? s_res[tid] : 0.f;
            float rmax = res;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, off));
            if (lane == 0) s_max[wave] = rmax;
            int accepted;
            const long long slot = (long long)total + crystal_compact(acc, lane, wave, s_cnt, accepted);
#pragma unroll
            for (int w = 0; w < CRYSTAL_WAVES; ++w) worst = fmaxf(worst, s_max[w]);
            if (acc && slot < max_ops) {
                const int q = s_q[tid];
                o_rot[slot] = code; o_res[slot] = res;
                o_trans[3 * slot] = translation(q, 0); o_trans[3 * slot + 1] = translation(q, 1); o_trans[3 * slot + 2] = translation(q, 2);
            }
            total += accepted;
            __syncthreads();  // s_q, s_res, s_cnt and s_max are written again in the next round
        }
        const int found = total - total_before;
        if (found > 0) {
            const int type = rotation_type(det, Wi[0] + Wi[4] + Wi[8]);
            ++distinct;
            if (type < 0) odd_type = 1;
            else hist += 1ull << (6 * type);
        }
        if (code == SYM_IDENTITY) n_translations = found;
    }

    // ---- rule 6 (phase 3): one wave looks the ten counts up among the 32 rows
    if (wave == 0) {
        unsigned long long row = 0;
        if (lane < 32) {
#pragma unroll
            for (int k = 0; k < 10; ++k) row |= (unsigned long long)SYM_POINT_GROUP_COUNTS[lane][k] << (6 * k);
        }
        const unsigned long long hit = __ballot(lane < 32 && row == hist);
        if (lane == 0) {
            int pg = hit && !odd_type ? __ffsll((long long)hit) - 1 : -1;
            if ((long long)total != (long long)distinct * n_translations) pg = -1;  // a tolerance can accept a set that is not closed
            o.n_lattice[b] = n_lattice; o.n_ops[b] = total; o.n_translations[b] = n_translations;
            o.residual[b] = worst; o.point_group[b] = pg;
            o.flags[b] = (total > max_ops ? ARREAU_SYM_OVERFLOW : 0) | (pg < 0 ? ARREAU_SYM_NOT_A_GROUP : 0);
        }
    }
    clear_ops(total < max_ops ? total : max_ops);
}

}  // namespace

extern "C" int arreau_crystal_symmetry(const float* d_frac, const int32_t* d_types, const float* d_lattice,
                                       const int32_t* d_crystal_offsets, int32_t B, int32_t N, const arreau_symmetry_params* params,
                                       arreau_symmetry_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_symmetry: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_symmetry: bad size");
    ARREAU_REQUIRE(std::isfinite(params->symprec) && params->symprec > 0.f, "arreau_crystal_symmetry: symprec must be finite and > 0");
    ARREAU_REQUIRE(params->max_ops >= 1 && params->max_ops <= ARREAU_SYM_MAX_OPS_CAP, "arreau_crystal_symmetry: max_ops must lie in 1..4096");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_types) || N == 0), "arreau_crystal_symmetry: null pointer");
    ARREAU_REQUIRE(out->n_lattice && out->n_ops && out->n_translations && out->ops_rotation && out->ops_translation && out->ops_residual &&
                       out->residual && out->point_group && out->flags,
                   "arreau_crystal_symmetry: null result array");
    sym_out o{out->n_lattice, out->n_ops, out->n_translations, out->ops_rotation, out->ops_translation, out->ops_residual,
              out->residual, out->point_group, out->flags};
    ARREAU_LAUNCH(crystal_symmetry_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_types, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, params->symprec, (int)params->max_ops, o);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
