// Kernels 2 + 3 of SURVEY.md: pair invariants -> polynomial features -> basis MLP -> window -> per-layer kernel
// projection, fused in registers, one wave per 64 (edge, orientation) rows.
//
// Replaces, per denoising step (sizes for B=256, n=20: 655 360 rows):
//   transforms/invariants.py:69-88 + geometry/invariants.py:10-31  (attr [E,O,6])
//   nn/embedding.py:10-14                                          (258-column polynomial tensor, 676 MB)
//   models/ponita.py:65,94 + utils/windowing.py:21-29              (kernel_basis [E,O,D], 671 MB)
//   nn/conv.py:110 for all L layers                                (kernel [E,O,C] x L)
// Nothing but the final per-layer kernels ([L][N*k*O][C] fp32) is written to HBM.
#include <stdlib.h>
#include <utility>

#include "internal.h"
#include "edge_rows.h"

// One wave owns 64 rows = 4 edge slots x 16 orientations of one receiver, as two 32-row column
// blocks cb = 0, 1 (row j of block cb: slot = slot0 + 2 cb + (j >> 4), orientation = j & 15; both lane
// halves carry the same row and differ in the k index they feed).  One wave per SIMD (the whole
// 512-register file): activations of both blocks stay in registers through the chain
//     monomials [96] -> h [C] -> basis [D] -> kernel_l [C] (l = 0..L-1).
// Output tiles are produced one at a time (out-tile-major), so only 2 accumulator tiles are live per
// GEMM and the three weight matrices become ONE linear stream of 16-byte fragments (w1 | w2 | wk_0..L-1,
// 1 KiB per wave-load, each fragment feeding 8 MFMAs).  The stream is prefetched PF groups ahead through
// a register ring, so L2 latency hides behind PF * 8 MFMAs (= 4096 cycles at PF = 8); no LDS, no barrier.
template <int C, int D, int NCB, int OCC>
__global__ __launch_bounds__(256, OCC) void edge_kernel(
    const float* __restrict__ nbr_dir,   // [N][k][3]
    const float* __restrict__ nbr_dist,  // [N][k]
    const int32_t* __restrict__ deg,     // [N]
    const int32_t* __restrict__ batch,   // [N] crystal of node
    const float* __restrict__ lattice,   // [B][9]
    const float* __restrict__ ori,       // [16][3]
    const float* __restrict__ stream,    // w1p | w2p | wkp[0..L-1], contiguous fragment stream
    const float* __restrict__ b1, const float* __restrict__ b2, float r_max, int N, int k, int L,
    float* __restrict__ kbuf)            // [L][N*k*16][C]
{
    constexpr int TC = C / 32, TD = D / 32, TM = ARREAU_MONO_PAD / 32;
    constexpr int G1 = TM * 4, G2 = TC * 4, G3 = TD * 4;          // k-groups per output tile
    constexpr int F1 = TC * G1, F2 = TD * G2, F3 = TC * G3;       // groups per matrix
    static_assert(F1 % ARREAU_PF == 0 && F2 % ARREAU_PF == 0 && F3 % ARREAU_PF == 0, "ring phase must repeat");
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, j = lane & 31;
    constexpr int SLOTS = 2 * NCB;  // edge slots per wave
    const int tiles_per_node = (k + SLOTS - 1) / SLOTS;
    const long long wt = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int node = (int)(wt / tiles_per_node);
    if (node >= N) return;
    const int slot0 = (int)(wt - (long long)node * tiles_per_node) * SLOTS;
    const int nd = min(deg[node], k);
    if (slot0 >= nd) return;  // wave-uniform: all four slots of this wave are empty
    const int o = j & 15;

    // start the weight stream before anything else
    const float* sp = stream + lane * 4;
    f32x4 ring[ARREAU_PF];
#pragma unroll
    for (int i = 0; i < ARREAU_PF; ++i) ring[i] = *reinterpret_cast<const f32x4*>(sp + (size_t)i * 256);

    const float* Lm = lattice + 9 * (size_t)batch[node];
    int slot[NCB];
    size_t row[NCB];
    EdgeRow er[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        slot[cb] = slot0 + 2 * cb + (j >> 4);
        // padding rows (k not a multiple of 4) read a valid slot.  A slot in [nd, k) computes on whatever the caller left in it,
        // NaN included, and its K rows are stored; the conv kernels behind this kernel drop them by a select on the degree (never
        // a multiply by zero), so the unused slots of a given graph do not change an output bit (include/arreau_hip.h).
        const int sc = min(slot[cb], k - 1);
        er[cb] = edge_row<false>(nbr_dir, nbr_dist, ori, Lm, (size_t)node * k + sc, o, r_max, slot[cb] < nd);
        row[cb] = ((size_t)node * k + sc) * 16 + o;
    }

    // ---- layer 1: h = GELU(W1f . mono + b1)   (83 distinct monomials, canonical order of model.hip) ----
    f32x16 acc1[TC][NCB];
    {
        static_assert(TM == 3, "three monomial tiles");
        f32x16 bm[TM][NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            bm[0][cb] = mono_tile<0>(er[cb].a, h, std::make_integer_sequence<int, 16>{});
            bm[1][cb] = mono_tile<1>(er[cb].a, h, std::make_integer_sequence<int, 16>{});
            bm[2][cb] = mono_tile<2>(er[cb].a, h, std::make_integer_sequence<int, 16>{});
        }
#pragma unroll
        for (int u = 0; u < TC; ++u) {
            f32x16 acc[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = arreau_bias_tile(b1, u, h);
            __builtin_amdgcn_sched_barrier(0);
            arreau_stream_tile<G1, TM, NCB>(acc, ring, sp, u * G1, bm);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc1[u][cb][r] = arreau_gelu(acc[cb][r]);
        }
    }

    // ---- layer 2: basis = GELU(W2 . h + b2) * window ---------------------------------------------------
    f32x16 acc2[TD][NCB];
    {
        const float* region = sp + (size_t)F1 * 256;
#pragma unroll
        for (int u = 0; u < TD; ++u) {
            f32x16 acc[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = arreau_bias_tile(b2, u, h);
            __builtin_amdgcn_sched_barrier(0);
            arreau_stream_tile<G2, TC, NCB>(acc, ring, region, u * G2, acc1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[u][cb][r] = arreau_gelu(acc[cb][r]) * er[cb].window;
        }
    }

    // ---- per layer: kernel_l = Wk_l . basis  (conv.py:110), written tile by tile -------------------------
    const size_t layer_stride = (size_t)N * k * 16 * C;
    for (int l = 0; l < L; ++l) {
        const float* region = sp + (size_t)(F1 + F2 + (size_t)l * F3) * 256;
#pragma unroll
        for (int u = 0; u < TC; ++u) {
            f32x16 acc[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            arreau_stream_tile<G3, TD, NCB>(acc, ring, region, u * G3, acc2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                if (slot[cb] < k) {
                    float* dst = kbuf + (size_t)l * layer_stride + row[cb] * C + 4 * h + 32 * u;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 v = {acc[cb][4 * q], acc[cb][4 * q + 1], acc[cb][4 * q + 2], acc[cb][4 * q + 3]};
                        *reinterpret_cast<f32x4*>(dst + 8 * q) = v;
                    }
                }
            }
        }
    }
}

template <int NCB, int OCC>
static void launch_variant(const arreau_model* m, const float* dir, const float* dist, const int32_t* deg,
                           const int32_t* batch, const float* lattice, int N, float* kbuf, hipStream_t s) {
    constexpr int SLOTS = 2 * NCB;
    const long long wave_tiles = (long long)N * ((m->k + SLOTS - 1) / SLOTS);
    ARREAU_LAUNCH((edge_kernel<128, 256, NCB, OCC>), dim3((unsigned)((wave_tiles + 3) / 4)), dim3(256), 0, s, dir,
                       dist, deg, batch, lattice, m->ori, m->w1p, m->b1, m->b2, m->cfg.radius, N, m->k, m->L, kbuf);
}

int arreau_launch_edge(const arreau_model* m, const ScorePlan& plan, const float* dir, const float* dist, const int32_t* deg,
                       const int32_t* batch, const float* lattice, int N, float* kbuf, hipStream_t s) {
    if (N == 0) return ARREAU_OK;
    if (!(m->C == 128 && m->D == 256)) {
        arreau_set_error("edge kernel: unsupported (hidden_dim, basis_dim)");
        return ARREAU_EINVAL;
    }
    // (the fp32-MFMA kernel, 32 rows per wave and 2 waves per SIMD, stays for A/B runs and as the numerical cross-check)
    if (plan.edge == ScorePlan::EDGE_F16X3) return arreau_launch_edge_f16x3(m, plan, dir, dist, deg, batch, lattice, N, kbuf, s);
    if (plan.edge == ScorePlan::EDGE_BF16X6) return arreau_launch_edge_bf16x6(m, dir, dist, deg, batch, lattice, N, kbuf, s);
    launch_variant<1, 2>(m, dir, dist, deg, batch, lattice, N, kbuf, s);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
