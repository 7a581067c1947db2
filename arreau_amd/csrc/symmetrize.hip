// Symmetrization of a batch of crystals (arreau_crystal_symmetrize; the rules are written out in include/arreau_hip.h): with the
// operations the symmetry search stored for a crystal, the atoms they map onto each other, their least-squares translations, the
// positions averaged over the group, the metric averaged over its rotations and the orbits.  One launch, one workgroup of four
// waves per crystal, no float atomics; needs no arreau_model.
//   metric   the distinct rotations dealt to the threads, their W^T G W summed in code order by six threads through LDS;
//   pass A   the operations dealt to the waves, the lanes run over the atoms i and take the nearest atom j of i's species: the
//            partner goes to out.partner (global memory: any crystal size, any number of operations, and an output of its own),
//            the differences are summed in atom order by lane reads, which gives the refined translation;
//   checks   every partner map one-to-one, the distinct partners of every atom counted (integer atomics on orbit_size);
//   pass B   one thread per atom, the operations in order: the difference is formed again from the stored partner (the same float32
//            operations, the same bits) and W^-1 (mean - delta) accumulated; displacements reduced in a fixed order.
// A crystal flagged at any point is copied through.
#include "internal.h"
#include "crystal_dev.h"
#include "prep_dev.h"
#include <cmath>

namespace {

struct symz_in {
    const int32_t *n_ops, *ops_rotation, *flags;
    const float* ops_translation;
};

struct symz_out {
    float *frac_out, *lattice, *lengths, *angles;
    int32_t *orbit, *orbit_size, *site_order, *n_orbits;
    float *max_displacement, *rms_displacement, *ops_translation, *ops_shift;
    int32_t *partner, *flags;
};

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_symmetrize_kernel(
    const float* __restrict__ frac, const int32_t* __restrict__ types, const float* __restrict__ lattice,
    const int32_t* __restrict__ offsets, int B, int N, int max_ops, symz_in f, symz_out o) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float sw[3 * CRYSTAL_LDS_ATOMS];
    __shared__ int sty[CRYSTAL_LDS_ATOMS];
    __shared__ float s_term[6 * CRYSTAL_THREADS];
    __shared__ int s_distinct[CRYSTAL_THREADS];
    __shared__ float s_metric[6];
    __shared__ int s_ndistinct;
    __shared__ float s_red[2 * CRYSTAL_WAVES];
    __shared__ int s_cnt[CRYSTAL_WAVES];

    const int32_t* rot = f.ops_rotation + (size_t)b * max_ops;
    const float* trans = f.ops_translation + 3 * (size_t)b * max_ops;
    float* o_trans = o.ops_translation + 3 * (size_t)b * max_ops;
    float* o_shift = o.ops_shift + 3 * (size_t)b * max_ops;
    auto partner = [&](int m, int atom) -> int32_t& { return o.partner[(size_t)m * N + (size_t)first + atom]; };

    // ---- rule 1: NONFINITE alone, else CELL | EMPTY, else NO_GROUP (all workgroup-uniform)
    int flags = 0, nops = 0;
    if (bad) flags = ARREAU_SYMZ_NONFINITE;
    else {
        const float volume = crystal_volume(Lm);
        flags = ((!(volume > 0.f) || !isfinite(volume)) ? ARREAU_SYMZ_CELL : 0) | (n == 0 ? ARREAU_SYMZ_EMPTY : 0);
    }
    if (!flags) {
        nops = f.n_ops[b];
        const int searched = f.flags[b];
        if ((searched & (ARREAU_SYM_AMBIGUOUS | ARREAU_SYM_OVERFLOW | ARREAU_SYM_NOT_A_GROUP)) || nops < 1 || nops > max_ops)
            flags = ARREAU_SYMZ_NO_GROUP;
    }

    // ---- the crystal's own metric (00, 11, 22, 01, 02, 12): what a flagged crystal's cell is rebuilt from
    float G[6];
    {
        const int identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        image_metric(identity, Lm, G);
    }

    // ---- rule 5: the mean of W^T G W over the distinct rotations (the operations come sorted by code), summed in code order
    if (!flags) {
        float acc = 0.f;
        int count = 0, badcode = 0;
        for (int base = 0; base < nops; base += CRYSTAL_THREADS) {
            const int m = base + tid;
            int distinct = 0;
            if (m < nops) {
                const int code = rot[m];
                int W[9];
                if (code < 0 || code >= SYM_CODES) badcode = 1;
                else {
                    const int det = decode_rotation(code, W);
                    if (det != 1 && det != -1) badcode = 1;
                    else if (m == 0 || rot[m - 1] != code) {
                        distinct = 1;
                        image_metric(W, Lm, s_term + 6 * tid);
                    }
                }
            }
            s_distinct[tid] = distinct;
            __syncthreads();
            if (tid < 6) {
                const int upto = min(CRYSTAL_THREADS, nops - base);
                for (int k = 0; k < upto; ++k)
                    if (s_distinct[k]) {
                        acc = __fadd_rn(acc, s_term[6 * k + tid]);
                        ++count;
                    }
            }
            __syncthreads();
        }
        if (tid < 6) s_metric[tid] = acc;
        if (tid == 0) s_ndistinct = count;
        if (__syncthreads_or(badcode)) flags = ARREAU_SYMZ_NO_GROUP;  // (not what the search writes: the stored rows are not trusted)
    }

    // ---- positions and species: staged in LDS when the crystal fits, else read where they are used (the same values)
    const bool staged = n <= CRYSTAL_LDS_ATOMS;
    if (staged && !bad) {
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) sw[a] = crystal_wrap(frac[3 * (size_t)first + a]);
        for (int a = tid; a < n; a += CRYSTAL_THREADS) sty[a] = types[(size_t)first + a];
    }
    for (int a = tid; a < n; a += CRYSTAL_THREADS) o.orbit_size[(size_t)first + a] = 0;
    __syncthreads();
    auto wpos = [&](int atom, int d) -> float { return staged ? sw[3 * atom + d] : crystal_wrap(frac[3 * ((size_t)first + atom) + d]); };
    auto species = [&](int atom) -> int { return staged ? sty[atom] : types[(size_t)first + atom]; };

    if (!flags) {
        // ---- rules 2, 3 (pass A): partners, differences, refined translations
        for (int m = wave; m < nops; m += CRYSTAL_WAVES) {
            int Wi[9];
            decode_rotation(rot[m], Wi);
            float W[9];
#pragma unroll
            for (int p = 0; p < 9; ++p) W[p] = (float)Wi[p];
            const float t0 = trans[3 * (size_t)m], t1 = trans[3 * (size_t)m + 1], t2 = trans[3 * (size_t)m + 2];
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                float e0 = 0.f, e1 = 0.f, e2 = 0.f;
                if (i < n) {
                    const float x0 = wpos(i, 0), x1 = wpos(i, 1), x2 = wpos(i, 2);
                    const float y0 = __fadd_rn(rot_row(W, 0, x0, x1, x2), t0), y1 = __fadd_rn(rot_row(W, 1, x0, x1, x2), t1),
                                y2 = __fadd_rn(rot_row(W, 2, x0, x1, x2), t2);
                    const int ti = species(i);
                    float best2 = __int_as_float(0x7f800000);
                    int best = -1;
                    for (int j = 0; j < n; ++j) {  // ascending j and a strict comparison: ties go to the smallest j
                        if (species(j) != ti) continue;
                        float d0 = __fsub_rn(y0, wpos(j, 0)), d1 = __fsub_rn(y1, wpos(j, 1)), d2 = __fsub_rn(y2, wpos(j, 2));
                        d0 = __fsub_rn(d0, rintf(d0)); d1 = __fsub_rn(d1, rintf(d1)); d2 = __fsub_rn(d2, rintf(d2));
                        const float len2 = crystal_frac_d2(d0, d1, d2, Lm);
                        if (len2 < best2) { best2 = len2; best = j; e0 = d0; e1 = d1; e2 = d2; }
                    }
                    partner(m, i) = best;
                }
                const int upto = min(64, n - i0);  // the sum over the atoms in atom order: lane k's difference, k ascending
                for (int k = 0; k < upto; ++k) {
                    s0 = __fadd_rn(s0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e0), k)));
                    s1 = __fadd_rn(s1, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e1), k)));
                    s2 = __fadd_rn(s2, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e2), k)));
                }
            }
            if (lane < 3) {
                const float mean = __fdiv_rn(lane == 0 ? s0 : (lane == 1 ? s1 : s2), (float)n);
                o_shift[3 * (size_t)m + lane] = -mean;
                o_trans[3 * (size_t)m + lane] = __fsub_rn(lane == 0 ? t0 : (lane == 1 ? t1 : t2), mean);
            }
        }
        __syncthreads();  // (partner, ops_shift: written above, read below by other threads of the workgroup)

        // ---- rules 1, 6 (checks): every map one-to-one; the distinct partners of every atom
        int notperm = 0;
        const long long pairs = (long long)nops * n;
        for (long long idx = tid; idx < pairs; idx += CRYSTAL_THREADS) {
            const int m = (int)(idx / n), i = (int)(idx - (long long)m * n);
            const int p = partner(m, i);
            if (p < 0) { notperm = 1; continue; }
            int twice = 0;
            for (int k = 0; k < i; ++k) twice |= partner(m, k) == p;
            notperm |= twice;
        }
        for (long long idx = tid; idx < (long long)n * n; idx += CRYSTAL_THREADS) {  // is j among the partners of i?  (n^2 n_ops reads)
            const int i = (int)(idx / n), j = (int)(idx - (long long)i * n);
            int hit = 0;
            for (int m = 0; m < nops; ++m) hit |= partner(m, i) == j;
            if (hit) atomicAdd(&o.orbit_size[(size_t)first + i], 1);
        }
        __syncthreads();
        for (int a = tid; a < n; a += CRYSTAL_THREADS) {
            const int size = __hip_atomic_load(&o.orbit_size[(size_t)first + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (past this CU's L1, as the atomics above went)
            notperm |= size < 1 || nops % size != 0;
        }
        if (__syncthreads_or(notperm)) flags = ARREAU_SYMZ_NOT_A_PERMUTATION;
    }

    float max2 = 0.f, sum2 = 0.f;
    int leaders = 0;
    if (!flags) {
        // ---- rules 4, 6, 7 (pass B): one thread per atom, the operations in order
        for (int i = tid; i < n; i += CRYSTAL_THREADS) {
            const float x0 = wpos(i, 0), x1 = wpos(i, 1), x2 = wpos(i, 2);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            int lowest = n;
            for (int m = 0; m < nops; ++m) {
                int Wi[9];
                const int det = decode_rotation(rot[m], Wi);
                float W[9], V[9];
#pragma unroll
                for (int p = 0; p < 9; ++p) W[p] = (float)Wi[p];
                inverse_rotation(Wi, det, V);
                const int j = partner(m, i);
                lowest = min(lowest, j);
                float d0 = __fsub_rn(__fadd_rn(rot_row(W, 0, x0, x1, x2), trans[3 * (size_t)m]), wpos(j, 0));
                float d1 = __fsub_rn(__fadd_rn(rot_row(W, 1, x0, x1, x2), trans[3 * (size_t)m + 1]), wpos(j, 1));
                float d2 = __fsub_rn(__fadd_rn(rot_row(W, 2, x0, x1, x2), trans[3 * (size_t)m + 2]), wpos(j, 2));
                d0 = __fsub_rn(-o_shift[3 * (size_t)m], __fsub_rn(d0, rintf(d0)));  // mean delta - delta
                d1 = __fsub_rn(-o_shift[3 * (size_t)m + 1], __fsub_rn(d1, rintf(d1)));
                d2 = __fsub_rn(-o_shift[3 * (size_t)m + 2], __fsub_rn(d2, rintf(d2)));
                a0 = __fadd_rn(a0, rot_row(V, 0, d0, d1, d2));
                a1 = __fadd_rn(a1, rot_row(V, 1, d0, d1, d2));
                a2 = __fadd_rn(a2, rot_row(V, 2, d0, d1, d2));
            }
            const float u0 = __fdiv_rn(a0, (float)nops), u1 = __fdiv_rn(a1, (float)nops), u2 = __fdiv_rn(a2, (float)nops);
            float* out = o.frac_out + 3 * ((size_t)first + i);
            out[0] = crystal_wrap(__fadd_rn(x0, u0)); out[1] = crystal_wrap(__fadd_rn(x1, u1)); out[2] = crystal_wrap(__fadd_rn(x2, u2));
            o.orbit[(size_t)first + i] = lowest;
            o.site_order[(size_t)first + i] = nops / __hip_atomic_load(&o.orbit_size[(size_t)first + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            leaders += lowest == i;
            const float moved2 = crystal_frac_d2(u0, u1, u2, Lm);
            max2 = fmaxf(max2, moved2);
            sum2 = __fadd_rn(sum2, moved2);
        }
        // the unused slots
        for (int k = 3 * nops + tid; k < 3 * max_ops; k += CRYSTAL_THREADS) { o_trans[k] = 0.f; o_shift[k] = 0.f; }
        for (long long idx = (long long)nops * n + tid; idx < (long long)max_ops * n; idx += CRYSTAL_THREADS)
            partner((int)(idx / n), (int)(idx % n)) = -1;
    } else {
        // ---- a flagged crystal is copied through: wrapped positions, every atom its own orbit, no operation
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) o.frac_out[3 * (size_t)first + a] = crystal_wrap(frac[3 * (size_t)first + a]);
        for (int a = tid; a < n; a += CRYSTAL_THREADS) {
            o.orbit[(size_t)first + a] = a; o.orbit_size[(size_t)first + a] = 1; o.site_order[(size_t)first + a] = 1;
        }
        for (int k = tid; k < 3 * max_ops; k += CRYSTAL_THREADS) { o_trans[k] = 0.f; o_shift[k] = 0.f; }
        for (long long idx = tid; idx < (long long)max_ops * n; idx += CRYSTAL_THREADS) partner((int)(idx / n), (int)(idx % n)) = -1;
        leaders = 0;
    }

    // ---- the workgroup's maximum, sum (lanes by xor shuffles, then the waves in order: a fixed order) and orbit count
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        max2 = fmaxf(max2, __shfl_xor(max2, off));
        sum2 = __fadd_rn(sum2, __shfl_xor(sum2, off));
        leaders += __shfl_xor(leaders, off);
    }
    if (lane == 0) { s_red[wave] = max2; s_red[CRYSTAL_WAVES + wave] = sum2; s_cnt[wave] = leaders; }
    __syncthreads();
    if (tid == 0) {
        max2 = 0.f; sum2 = 0.f; leaders = 0;
#pragma unroll
        for (int w = 0; w < CRYSTAL_WAVES; ++w) {
            max2 = fmaxf(max2, s_red[w]);
            sum2 = __fadd_rn(sum2, s_red[CRYSTAL_WAVES + w]);
            leaders += s_cnt[w];
        }
        o.n_orbits[b] = flags ? n : leaders;
        o.max_displacement[b] = sqrtf(max2);
        o.rms_displacement[b] = n > 0 ? sqrtf(__fdiv_rn(sum2, (float)n)) : 0.f;
        o.flags[b] = flags;
        // ---- rule 5: lengths and angles of the metric, the cell in the sampler's orientation
        if (!flags) {
            const float nd = (float)s_ndistinct;
#pragma unroll
            for (int e = 0; e < 6; ++e) G[e] = __fdiv_rn(s_metric[e], nd);
        }
        float len[3], ang[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) len[i] = sqrtf(G[i]);
        const int pj[3] = {1, 0, 0}, pk[3] = {2, 2, 1}, pe[3] = {5, 4, 3};  // angle i lies between the other two vectors
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float c = __fdiv_rn(G[pe[i]], __fmul_rn(len[pj[i]], len[pk[i]]));
            ang[i] = acosf(fminf(fmaxf(c, -1.f), 1.f));
        }
        float cell[9];
        arreau_prep_cell(len, ang, cell);
#pragma unroll
        for (int i = 0; i < 3; ++i) { o.lengths[3 * (size_t)b + i] = len[i]; o.angles[3 * (size_t)b + i] = ang[i]; }
#pragma unroll
        for (int q = 0; q < 9; ++q) o.lattice[9 * (size_t)b + q] = cell[q];
    }
}

}  // namespace

extern "C" int arreau_crystal_symmetrize(const float* d_frac, const int32_t* d_types, const float* d_lattice,
                                         const int32_t* d_crystal_offsets, int32_t B, int32_t N, const arreau_symmetry_result* found,
                                         int32_t max_ops, arreau_symmetrize_result* out, void* stream) {
    ARREAU_REQUIRE(found != nullptr && out != nullptr, "arreau_crystal_symmetrize: null search result or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_symmetrize: bad size");
    ARREAU_REQUIRE(max_ops >= 1 && max_ops <= ARREAU_SYM_MAX_OPS_CAP, "arreau_crystal_symmetrize: max_ops must lie in 1..4096");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_types) || N == 0), "arreau_crystal_symmetrize: null pointer");
    ARREAU_REQUIRE(found->n_ops && found->ops_rotation && found->ops_translation && found->flags,
                   "arreau_crystal_symmetrize: null array in the search result");
    ARREAU_REQUIRE(out->lattice && out->lengths && out->angles && out->n_orbits && out->max_displacement && out->rms_displacement &&
                       out->ops_translation && out->ops_shift && out->flags,
                   "arreau_crystal_symmetrize: null result array");
    ARREAU_REQUIRE((out->frac_out && out->orbit && out->orbit_size && out->site_order && out->partner) || N == 0,
                   "arreau_crystal_symmetrize: null per-atom result array");
    symz_in f{found->n_ops, found->ops_rotation, found->flags, found->ops_translation};
    symz_out o{out->frac_out, out->lattice, out->lengths, out->angles, out->orbit, out->orbit_size, out->site_order, out->n_orbits,
               out->max_displacement, out->rms_displacement, out->ops_translation, out->ops_shift, out->partner, out->flags};
    ARREAU_LAUNCH(crystal_symmetrize_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_types, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, (int)max_ops, f, o);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
