// Coordination environments of a batch of crystals (arreau_crystal_coordination; the rules are written out in include/arreau_hip.h):
// per atom its nearest distance over every periodic image, the neighbours within (1 + tol) times that distance and a cutoff, their
// number, the first max_neighbors of them in (j, m) order and how many the other end agrees on; per crystal the sums and extremes.
// The screen's exact image search (screen.hip), run per atom over all j.  One launch, one workgroup of four waves per crystal, one
// wave per atom, no atomics; needs no arreau_model.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

namespace {

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_coordination_kernel(
    const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets, int B, int N,
    float f2 /* (1 + tol)^2 */, float r2 /* cutoff^2 */, float cutoff, int max_nb, int max_shells, arreau_coordination_result out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (wave-uniform: the atoms a wave owns are scalars)
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float spos[3 * CRYSTAL_LDS_ATOMS];
    __shared__ unsigned s_min[CRYSTAL_LDS_ATOMS];
    __shared__ int s_bonds[CRYSTAL_WAVES], s_mutual[CRYSTAL_WAVES], s_lo[CRYSTAL_WAVES], s_hi[CRYSTAL_WAVES], s_flags[CRYSTAL_WAVES];

    const float qnan = __int_as_float(0x7fc00000);
    int4* const nb_rows = reinterpret_cast<int4*>(out.neighbors);  // one (j, n1, n2, n3) per slot
    // NONFINITE / CELL (workgroup-uniform): nothing is computed, the reals are NaN, the lists -1, the counts 0
    auto blank = [&](int flags) {
        for (int a = tid; a < n; a += CRYSTAL_THREADS) {
            const size_t A = (size_t)first + a;
            out.cn[A] = 0; out.mutual[A] = 0;
            out.nearest[A] = qnan; out.farthest[A] = qnan; out.nearest_d2[A] = qnan;
        }
        const size_t slots = (size_t)n * max_nb;
        for (size_t q = tid; q < slots; q += CRYSTAL_THREADS) nb_rows[(size_t)first * max_nb + q] = make_int4(-1, -1, -1, -1);
        if (tid == 0) {
            out.n_bonds[b] = 0; out.n_mutual[b] = 0; out.min_cn[b] = -1; out.max_cn[b] = -1;
            out.mean_cn[b] = qnan; out.flags[b] = flags;
        }
    };
    if (bad) {
        blank(ARREAU_COORD_NONFINITE);
        return;
    }
    crystal_cell cell;
    if (crystal_cell_measure(Lm, cutoff, max_shells, cell)) {
        blank(ARREAU_COORD_CELL);
        return;
    }
    crystal_cell_images(cell);

    const crystal_positions position = crystal_stage_positions(spos, frac, Lm, first, n);
    const bool staged = position.staged;
    const unsigned long long span = (unsigned long long)n * cell.M;  // receiver i meets e = j * M + m, 0 <= e < span
    // This kernel keeps its own copy of crystal_dev.h's walk and contact: it is at the limit of its scalar registers, and through
    // crystal_walk / crystal_walk_chunks 59 of them go through vector lanes instead of 13.  Medians, MI355X, 1024 random crystals of
    // 64 atoms: the parent's 546 us became 567 us through the walk helpers, 577 us through them and crystal_contact_at.
    const bool narrow = crystal_walk_narrow(span, 64);  // (uniform) the usual case: 32-bit index arithmetic

    // ---- phase A: d2min(i), the minimum of the bits of d2 (d2 >= +0: the bits order like the values; inf keeps its place above
    // every finite value) over every (j, m) but the atom itself.  One wave per atom; the wave minimum is a min of integers.
    for (int i = wave; i < n; i += CRYSTAL_WAVES) {
        const float pix = position(i, 0), piy = position(i, 1), piz = position(i, 2);
        unsigned best = 0x7f800000u;
        auto contact = [&](unsigned j, unsigned m) {
            if (j == (unsigned)i && m == cell.centre) return;  // the atom itself; every other image of i counts
            // crystal_contact_at's operations (see above)
            const unsigned m12 = m / cell.W3;
            const float n3 = (float)((int)(m - m12 * cell.W3) - cell.N3), n2 = (float)((int)(m12 % cell.W2) - cell.N2), n1 = (float)((int)(m12 / cell.W2) - cell.N1);
            const float sx = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[0]), __fmul_rn(n2, Lm[3])), __fmul_rn(n3, Lm[6]));
            const float sy = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[1]), __fmul_rn(n2, Lm[4])), __fmul_rn(n3, Lm[7]));
            const float sz = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[2]), __fmul_rn(n2, Lm[5])), __fmul_rn(n3, Lm[8]));
            const float dx = __fsub_rn(__fadd_rn(position((int)j, 0), sx), pix);
            const float dy = __fsub_rn(__fadd_rn(position((int)j, 1), sy), piy);
            const float dz = __fsub_rn(__fadd_rn(position((int)j, 2), sz), piz);
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            best = min(best, __float_as_uint(d2));
        };
        if (narrow) {
            for (unsigned e = (unsigned)lane; e < (unsigned)span; e += 64u) {
                const unsigned j = e / cell.M;
                contact(j, e - j * cell.M);
            }
        } else {
            for (unsigned long long e = (unsigned long long)lane; e < span; e += 64ull) {
                const unsigned long long j = e / cell.M;
                contact((unsigned)j, (unsigned)(e - j * cell.M));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) best = min(best, (unsigned)__shfl_xor(best, off));
        best = __builtin_amdgcn_readfirstlane(best);
        if (lane == 0) {
            out.nearest_d2[(size_t)first + i] = __uint_as_float(best);
            if (staged) s_min[i] = best;
        }
    }
    __syncthreads();  // every d2min of the crystal is written (LDS, or nearest_d2 for a crystal that is not staged)
    auto threshold = [&](int atom) -> float {
        return __fmul_rn(f2, staged ? __uint_as_float(s_min[atom]) : out.nearest_d2[(size_t)first + atom]);
    };

    // ---- phase B: the neighbours.  One wave per atom, e in ascending chunks of 64; a ballot and the population count of the lanes
    // below give every hit its slot, so the stored ones are the first max_nb in ascending (j, m) whatever the launch.
    int w_bonds = 0, w_mutual = 0, w_lo = 0x7fffffff, w_hi = -1, w_flags = 0;
    for (int i = wave; i < n; i += CRYSTAL_WAVES) {
        const float pix = position(i, 0), piy = position(i, 1), piz = position(i, 2);
        const float thr2 = threshold(i);
        int4* const row = nb_rows + ((size_t)first + i) * max_nb;
        unsigned far = 0;  // bits of the largest neighbour d2
        int cn = 0, mutual = 0;
        auto chunk = [&](bool valid, unsigned j, unsigned m) {
            bool hit = false, agreed = false;
            int n1i = 0, n2i = 0, n3i = 0;
            if (valid && !(j == (unsigned)i && m == cell.centre)) {
                const unsigned m12 = m / cell.W3;
                n3i = (int)(m - m12 * cell.W3) - cell.N3; n2i = (int)(m12 % cell.W2) - cell.N2; n1i = (int)(m12 / cell.W2) - cell.N1;
                const float n3 = (float)n3i, n2 = (float)n2i, n1 = (float)n1i;
                const float sx = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[0]), __fmul_rn(n2, Lm[3])), __fmul_rn(n3, Lm[6]));
                const float sy = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[1]), __fmul_rn(n2, Lm[4])), __fmul_rn(n3, Lm[7]));
                const float sz = __fadd_rn(__fadd_rn(__fmul_rn(n1, Lm[2]), __fmul_rn(n2, Lm[5])), __fmul_rn(n3, Lm[8]));
                const float dx = __fsub_rn(__fadd_rn(position((int)j, 0), sx), pix);
                const float dy = __fsub_rn(__fadd_rn(position((int)j, 1), sy), piy);
                const float dz = __fsub_rn(__fadd_rn(position((int)j, 2), sz), piz);
                const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                hit = d2 <= thr2 && d2 <= r2;
                if (hit) {
                    agreed = d2 <= threshold((int)j);  // the d2 computed from i's side against j's own threshold
                    far = max(far, __float_as_uint(d2));
                }
            }
            const unsigned long long hits = __ballot(hit);  // (every lane of the wave is here: the chunk loop is uniform)
            const int slot = cn + __popcll(hits & ((1ull << lane) - 1ull));
            if (hit && slot < max_nb) row[slot] = make_int4((int)j, n1i, n2i, n3i);
            cn += __popcll(hits);
            mutual += __popcll(__ballot(agreed));
        };
        if (narrow) {
            for (unsigned base = 0; base < (unsigned)span; base += 64u) {
                const unsigned e = base + (unsigned)lane, j = e / cell.M;
                chunk(e < (unsigned)span, j, e - j * cell.M);
            }
        } else {
            for (unsigned long long base = 0; base < span; base += 64ull) {
                const unsigned long long e = base + (unsigned long long)lane, j = e / cell.M;
                chunk(e < span, (unsigned)j, (unsigned)(e - j * cell.M));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) far = max(far, (unsigned)__shfl_xor(far, off));
        far = __builtin_amdgcn_readfirstlane(far);
        if (lane >= min(cn, max_nb) && lane < max_nb) row[lane] = make_int4(-1, -1, -1, -1);  // (max_nb <= 64: one lane per slot)
        const unsigned d2min = __float_as_uint(out.nearest_d2[(size_t)first + i]);
        if (lane == 0) {
            const size_t A = (size_t)first + i;
            out.cn[A] = cn; out.mutual[A] = mutual;
            out.nearest[A] = sqrtf(__uint_as_float(d2min));  // correctly rounded, like the screen's distance
            out.farthest[A] = sqrtf(__uint_as_float(far));
        }
        w_bonds += cn; w_mutual += mutual;
        w_lo = min(w_lo, cn); w_hi = max(w_hi, cn);
        w_flags |= (d2min == 0u ? ARREAU_COORD_OVERLAP : 0) | (cn == 0 ? ARREAU_COORD_ISOLATED : 0) | (cn > max_nb ? ARREAU_COORD_OVERFLOW : 0);
    }

    // ---- per crystal: integer sums, minima and maxima of the four waves through LDS (any order gives the same value)
    if (lane == 0) {
        s_bonds[wave] = w_bonds; s_mutual[wave] = w_mutual; s_lo[wave] = w_lo; s_hi[wave] = w_hi; s_flags[wave] = w_flags;
    }
    __syncthreads();
    if (tid == 0) {
        int bonds = 0, mutual = 0, lo = 0x7fffffff, hi = -1, flags = n == 0 ? ARREAU_COORD_EMPTY : 0;
        for (int w = 0; w < CRYSTAL_WAVES; ++w) {
            bonds += s_bonds[w]; mutual += s_mutual[w];
            lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]);
            flags |= s_flags[w];
        }
        out.n_bonds[b] = bonds; out.n_mutual[b] = mutual;
        out.min_cn[b] = n == 0 ? -1 : lo; out.max_cn[b] = hi;
        out.mean_cn[b] = n == 0 ? qnan : __fdiv_rn((float)bonds, (float)n);  // (the blank NaN, not the sign 0 / 0 happens to give)
        out.flags[b] = flags;
    }
}

}  // namespace

extern "C" int arreau_crystal_coordination(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                                           const arreau_coordination_params* params, arreau_coordination_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_coordination: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_coordination: bad size");
    ARREAU_REQUIRE(std::isfinite(params->tol) && params->tol >= 0.f, "arreau_crystal_coordination: tol must be finite and >= 0");
    ARREAU_REQUIRE(std::isfinite(params->cutoff) && params->cutoff > 0.f, "arreau_crystal_coordination: cutoff must be finite and > 0");
    ARREAU_REQUIRE(params->max_neighbors >= 1 && params->max_neighbors <= ARREAU_COORD_MAX_NEIGHBORS,
                   "arreau_crystal_coordination: max_neighbors must lie in 1..64");
    ARREAU_REQUIRE(params->max_shells >= 1 && params->max_shells <= ARREAU_SCREEN_MAX_SHELLS,
                   "arreau_crystal_coordination: max_shells must lie in 1..8");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && (d_frac || N == 0), "arreau_crystal_coordination: null pointer");
    ARREAU_REQUIRE(out->n_bonds && out->n_mutual && out->min_cn && out->max_cn && out->mean_cn && out->flags,
                   "arreau_crystal_coordination: null per-crystal result array");
    ARREAU_REQUIRE(N == 0 || (out->cn && out->neighbors && out->nearest && out->farthest && out->mutual && out->nearest_d2),
                   "arreau_crystal_coordination: null per-atom result array");
    ARREAU_REQUIRE((reinterpret_cast<uintptr_t>(out->neighbors) & 15u) == 0, "arreau_crystal_coordination: neighbors must be 16-byte aligned");
    const double f = 1.0 + (double)params->tol;
    const float f2 = (float)(f * f);
    const float r2 = (float)((double)params->cutoff * (double)params->cutoff);
    ARREAU_LAUNCH(crystal_coordination_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, f2, r2, params->cutoff, (int)params->max_neighbors, (int)params->max_shells, *out);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
