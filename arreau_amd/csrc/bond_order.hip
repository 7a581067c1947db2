// Bond angles and Steinhardt order parameters of a batch of crystals (arreau_crystal_bond_order; the rules are written out in
// include/arreau_hip.h): per atom, from the neighbour list a coordination result stores, the unit bond vectors, the cosine of every
// pair of them, its bin in a 37-bin angle histogram and its Legendre polynomials P_2, P_4, P_6, P_8, whose sums give q_l by the
// addition theorem; per crystal the summed histogram and the mean q_l.  One launch after the coordination launch, one workgroup of
// four waves per crystal, one wave per atom, lane f owns bond f and walks the bonds before it; no global atomics, needs no
// arreau_model.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

namespace {

struct bond_edges {
    float e[ARREAU_BOND_ANGLE_BINS - 1];
};

// a_k = (float)((2k+1)/(k+1)), b_k = (float)(k/(k+1)), formed in double: P_{k+1} = a_k (c P_k) - b_k P_{k-1}, k = 1..7
__device__ __forceinline__ float legendre_a(int k) { return (float)((2.0 * k + 1.0) / (k + 1.0)); }
__device__ __forceinline__ float legendre_b(int k) { return (float)((double)k / (k + 1.0)); }

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_bond_order_kernel(
    const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets, int B, int N,
    const int32_t* __restrict__ cn_in, const int4* __restrict__ nb_rows, int max_nb, bond_edges edges, arreau_bond_order_result out) {
    constexpr int BINS = ARREAU_BOND_ANGLE_BINS, NL = ARREAU_BOND_ORDER_L;
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float spos[3 * CRYSTAL_LDS_ATOMS];
    __shared__ float s_u[CRYSTAL_WAVES][3][64];  // a wave's unit bond vectors, component by component
    __shared__ int s_hist[CRYSTAL_WAVES][BINS];  // a wave's angle counters: of its current atom, at the end of its atoms' sum
    __shared__ int s_flags[CRYSTAL_WAVES];

    const float qnan = __int_as_float(0x7fc00000);
    // NONFINITE / BAD_LIST (workgroup-uniform): nothing is computed, the reals are NaN, the counts 0
    auto blank = [&](int flags) {
        for (int a = tid; a < n; a += CRYSTAL_THREADS) {
            const size_t A = (size_t)first + a;
            out.n_used[A] = 0;
            out.cos_min[A] = qnan; out.cos_max[A] = qnan;
        }
        for (size_t q = tid; q < (size_t)NL * n; q += CRYSTAL_THREADS) {
            out.q[(size_t)first * NL + q] = qnan; out.q2[(size_t)first * NL + q] = qnan;
        }
        for (size_t q = tid; q < (size_t)BINS * n; q += CRYSTAL_THREADS) out.angles[(size_t)first * BINS + q] = 0;
        if (tid < BINS) out.angle_hist[(size_t)b * BINS + tid] = 0;
        if (tid < NL) out.mean_q[(size_t)b * NL + tid] = qnan;
        if (tid == 0) { out.n_angles[b] = 0; out.flags[b] = flags; }
    };
    if (bad) {
        blank(ARREAU_BOND_NONFINITE);
        return;
    }

    // ---- the list: every cn >= 0 and every j of the entries in use inside the crystal, before anything is indexed with one
    int bad_list = 0;
    for (size_t q = tid; q < (size_t)n * max_nb; q += CRYSTAL_THREADS) {
        const int a = (int)(q / max_nb), k = (int)(q - (size_t)a * max_nb);
        const int c = cn_in[(size_t)first + a];
        bad_list |= c < 0;
        if (k < min(c, max_nb)) {
            const int j = nb_rows[(size_t)first * max_nb + q].x;
            bad_list |= j < 0 || j >= n;
        }
    }
    if (__syncthreads_or(bad_list)) {
        blank(ARREAU_BOND_BAD_LIST);
        return;
    }

    // ---- positions: crystal_stage_positions' lines, kept here: through the helper 256 fcc supercells of 32 atoms at 64 bonds take
    // 206.6 us against 205.6 us, at 12 bonds 61.0 us against 60.7 us (medians, MI355X, twice each, the parent's spread 0.1 us)
    const bool staged = n <= CRYSTAL_LDS_ATOMS;
    if (staged)
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) spos[a] = crystal_cart(frac, Lm, (size_t)first + a / 3, a % 3);
    __syncthreads();
    auto position = [&](int atom, int d) -> float { return staged ? spos[3 * atom + d] : crystal_cart(frac, Lm, (size_t)first + atom, d); };

    // ---- one wave per atom; every wave runs every round (the barriers inside are the workgroup's), `active` says whether it
    // has an atom in it.  A wave's LDS regions are its own: written in part 1, read by its other lanes in part 2 (barrier
    // between), the counters read in part 3 (barrier between) and cleared by the lane that read them in the next part 1.
    int w_flags = 0, w_hist = 0;  // lane k < 37: the sum of this wave's atoms' counters of bin k
    for (int i0 = 0; i0 < n; i0 += CRYSTAL_WAVES) {
        const int i = i0 + wave;
        const bool active = i < n;  // (wave-uniform)
        const size_t A = (size_t)first + (active ? i : 0);
        int cn = 0, m = 0;
        bool degenerate = false;
        float ux = 0.f, uy = 0.f, uz = 0.f;
        // part 1: the bonds.  Lane e < m forms bond e; lanes beyond m read neither the list nor positions.
        if (active) {
            cn = __builtin_amdgcn_readfirstlane(cn_in[A]);
            m = min(cn, max_nb);
            if (lane < BINS) s_hist[wave][lane] = 0;
            bool zero = false;
            if (lane < m) {
                const int4 en = nb_rows[A * max_nb + lane];  // (j validated above)
                const float n1 = (float)en.y, n2 = (float)en.z, n3 = (float)en.w;
                const float dx = __fsub_rn(__fadd_rn(position(en.x, 0), rows_rn(Lm, 0, n1, n2, n3)), position(i, 0));
                const float dy = __fsub_rn(__fadd_rn(position(en.x, 1), rows_rn(Lm, 1, n1, n2, n3)), position(i, 1));
                const float dz = __fsub_rn(__fadd_rn(position(en.x, 2), rows_rn(Lm, 2, n1, n2, n3)), position(i, 2));
                const float d2 = dot3_rn(dx, dy, dz, dx, dy, dz);
                const float d = sqrtf(d2);  // correctly rounded, like the screen's distance
                zero = d2 == 0.f;
                ux = __fdiv_rn(dx, d); uy = __fdiv_rn(dy, d); uz = __fdiv_rn(dz, d);
                s_u[wave][0][lane] = ux; s_u[wave][1][lane] = uy; s_u[wave][2][lane] = uz;
            }
            degenerate = __ballot(zero) != 0ull;
        }
        __syncthreads();
        // part 2: the pairs.  Lane f walks e = 0 .. f-1 in ascending order: sums from +0, extremes by comparison, counters in LDS.
        float s[NL] = {0.f, 0.f, 0.f, 0.f};
        float lo = __int_as_float(0x7f800000), hi = __int_as_float(0xff800000);
        if (active && !degenerate && lane < m) {
            for (int e = 0; e < lane; ++e) {  // (e < lane < m: only slots written in part 1)
                float c = dot3_rn(s_u[wave][0][e], s_u[wave][1][e], s_u[wave][2][e], ux, uy, uz);
                c = c < -1.f ? -1.f : c;
                c = c > 1.f ? 1.f : c;
                float pm = 1.f, pk = c;  // P_{k-1}, P_k
#pragma unroll
                for (int k = 1; k < 2 * NL; ++k) {
                    const float t = __fmul_rn(legendre_a(k), __fmul_rn(c, pk));
                    const float next = __fsub_rn(t, __fmul_rn(legendre_b(k), pm));
                    pm = pk; pk = next;
                    if (k & 1) s[k >> 1] = __fadd_rn(s[k >> 1], pk);  // k + 1 = 2, 4, 6, 8
                }
                lo = c < lo ? c : lo;
                hi = c > hi ? c : hi;
                int bin = 0;
#pragma unroll
                for (int k = 0; k < BINS - 1; ++k) bin += c <= edges.e[k] ? 1 : 0;
                atomicAdd(&s_hist[wave][bin], 1);
            }
        }
        __syncthreads();
        // part 3: the atom's rows
        if (active) {
            float S[NL];
#pragma unroll
            for (int l = 0; l < NL; ++l) S[l] = crystal_wave_sum(s[l]);
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) {
                const float ol = __shfl_xor(lo, w), oh = __shfl_xor(hi, w);
                lo = ol < lo ? ol : lo;
                hi = oh > hi ? oh : hi;
            }
            const int count = lane < BINS ? s_hist[wave][lane] : 0;  // (0 for a degenerate atom: nothing was added)
            if (lane < BINS) out.angles[A * BINS + lane] = count;
            w_hist += count;
            if (lane == 0) {
                out.n_used[A] = m;
                const float mf = (float)m;
                const bool blank_q = degenerate || m == 0;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    float q2 = __fdiv_rn(__fadd_rn(mf, __fmul_rn(2.f, S[l])), __fmul_rn(mf, mf));
                    q2 = q2 < 0.f ? 0.f : q2;
                    out.q2[A * NL + l] = blank_q ? qnan : q2;
                    out.q[A * NL + l] = blank_q ? qnan : sqrtf(q2);
                }
                const bool no_pair = degenerate || m < 2;
                out.cos_min[A] = no_pair ? qnan : lo;
                out.cos_max[A] = no_pair ? qnan : hi;
            }
            w_flags |= (degenerate ? ARREAU_BOND_OVERLAP : 0) | (m == 0 ? ARREAU_BOND_ISOLATED : 0) | (cn > max_nb ? ARREAU_BOND_TRUNCATED : 0);
        }
    }

    // ---- per crystal: the counters of the four waves (integers: any order), the flags, and the mean q_l as a lane sum over the
    // atoms, lane = i mod 64, ascending i -- from the q rows the waves wrote (the barrier makes them visible to the workgroup)
    if (lane < BINS) s_hist[wave][lane] = w_hist;  // (its own lane's slot: read last by this lane)
    if (lane == 0) s_flags[wave] = w_flags;
    __syncthreads();
    if (wave == 0) {
        int total = 0, flags = n == 0 ? ARREAU_BOND_EMPTY : 0;
#pragma unroll
        for (int w = 0; w < CRYSTAL_WAVES; ++w) {
            total += lane < BINS ? s_hist[w][lane] : 0;
            flags |= s_flags[w];
        }
        if (lane < BINS) out.angle_hist[(size_t)b * BINS + lane] = total;
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) total += __shfl_xor(total, w);
        float sum[NL] = {0.f, 0.f, 0.f, 0.f};
        int used = 0;
        for (int a = lane; a < n; a += 64) {
            const size_t A = (size_t)first + a;
            float q[NL];
            bool fin = out.n_used[A] >= 1;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                q[l] = out.q[A * NL + l];
                fin = fin && isfinite(q[l]);
            }
            if (fin) {
                ++used;
#pragma unroll
                for (int l = 0; l < NL; ++l) sum[l] = __fadd_rn(sum[l], q[l]);
            }
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) used += __shfl_xor(used, w);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const float v = crystal_wave_sum(sum[l]);
            if (lane == 0) out.mean_q[(size_t)b * NL + l] = used == 0 ? qnan : __fdiv_rn(v, (float)used);
        }
        if (lane == 0) { out.n_angles[b] = total; out.flags[b] = flags; }
    }
}

}  // namespace

extern "C" int arreau_crystal_bond_order(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                                         const int32_t* d_cn, const int32_t* d_neighbors, const arreau_bond_order_params* params,
                                         arreau_bond_order_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_bond_order: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_bond_order: bad size");
    ARREAU_REQUIRE(params->max_neighbors >= 1 && params->max_neighbors <= ARREAU_COORD_MAX_NEIGHBORS,
                   "arreau_crystal_bond_order: max_neighbors must lie in 1..64");
    bond_edges edges;
    for (int k = 0; k < ARREAU_BOND_ANGLE_BINS - 1; ++k) {
        const float e = params->cos_edges[k], above = k == 0 ? 1.f : params->cos_edges[k - 1];
        ARREAU_REQUIRE(e < above && e > -1.f, "arreau_crystal_bond_order: cos_edges must descend strictly inside (-1, 1)");
        edges.e[k] = e;
    }
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && (d_frac || N == 0), "arreau_crystal_bond_order: null pointer");
    ARREAU_REQUIRE(N == 0 || (d_cn && d_neighbors), "arreau_crystal_bond_order: null neighbour list");
    ARREAU_REQUIRE((reinterpret_cast<uintptr_t>(d_neighbors) & 15u) == 0, "arreau_crystal_bond_order: neighbors must be 16-byte aligned");
    ARREAU_REQUIRE(out->mean_q && out->n_angles && out->angle_hist && out->flags, "arreau_crystal_bond_order: null per-crystal result array");
    ARREAU_REQUIRE(N == 0 || (out->n_used && out->q && out->q2 && out->cos_min && out->cos_max && out->angles),
                   "arreau_crystal_bond_order: null per-atom result array");
    ARREAU_LAUNCH(crystal_bond_order_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, d_cn, reinterpret_cast<const int4*>(d_neighbors), (int)params->max_neighbors, edges, *out);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
