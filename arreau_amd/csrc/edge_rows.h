// Per-row geometry of the edge kernels (edge.hip, edge_bf16.hip, edge_f16.hip, edge_rows_kernel in train_net.hip):
// the attributes of one (edge slot, orientation) row, its cut-off window and the compile-time monomial table.
// Include after internal.h.
#pragma once
#include <utility>

// ---- compile-time monomial table: index f -> (degree, i, j, k), in the canonical order of fold_poly_weight (model.hip) --
struct MonoIdx { int n, i, j, k; };
__host__ __device__ constexpr MonoIdx mono_idx(int f) {
    int p = 0;
    for (int i = 0; i < 6; ++i, ++p)
        if (p == f) return {1, i, 0, 0};
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++p)
            if (p == f) return {2, i, j, 0};
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j)
            for (int k = j; k < 6; ++k, ++p)
                if (p == f) return {3, i, j, k};
    return {0, 0, 0, 0};  // padding columns 83..95
}

template <int F>
__device__ __forceinline__ float mono_at(const float (&a)[6]) {
    constexpr MonoIdx m = mono_idx(F);
    if constexpr (m.n == 1) return a[m.i];
    else if constexpr (m.n == 2) return a[m.i] * a[m.j];
    else if constexpr (m.n == 3) return (a[m.i] * a[m.j]) * a[m.k];
    else return 0.0f;
}

// "accumulator-layout" tile of monomials: register r of tile T holds feature 32T + 8(r>>2) + (r&3) on lane half h = 0
// and that + 4 on half 1
template <int T, int... R>
__device__ __forceinline__ f32x16 mono_tile(const float (&a)[6], int h, std::integer_sequence<int, R...>) {
    f32x16 v;
    ((v[R] = h ? mono_at<32 * T + 8 * (R >> 2) + (R & 3) + 4>(a) : mono_at<32 * T + 8 * (R >> 2) + (R & 3)>(a)), ...);
    return v;
}

// x / d.  FAST_RCP (the fp16x3 kernels): x * v_rcp_f32(d), 1 ulp, instead of the IEEE division sequence -- far inside the
// 1e-5 parity budget.  This is the ONLY difference between the two instantiations of edge_row; they are not bit-equal to
// each other, and a launch form must keep to the one its bit-identical siblings use.
template <bool FAST_RCP>
__device__ __forceinline__ float edge_row_div(float x, float d) {
    if constexpr (FAST_RCP) return x * __builtin_amdgcn_rcpf(d);
    else return x / d;
}

struct EdgeRow { float a[6]; float window; };

// attributes of one (edge slot, orientation) row  (transforms/invariants.py:82-88).  e = the row's edge index with the
// slot already clamped by the caller (each kernel has its own reason for the clamp it uses), valid = slot < degree.
template <bool FAST_RCP>
__device__ __forceinline__ EdgeRow edge_row(const float* __restrict__ nbr_dir, const float* __restrict__ nbr_dist,
                                            const float* __restrict__ ori, const float* __restrict__ Lm, size_t e,
                                            int o, float r_max, bool valid) {
    EdgeRow r;
    const float dx = nbr_dir[3 * e + 0], dy = nbr_dir[3 * e + 1], dz = nbr_dir[3 * e + 2];
    const float dist = nbr_dist[e];
    const float ox = ori[3 * o + 0], oy = ori[3 * o + 1], oz = ori[3 * o + 2];
    r.a[0] = (dx * ox + dy * oy) + dz * oz;  // inv1 = dir . o
    const float rx = dx - r.a[0] * ox, ry = dy - r.a[0] * oy, rz = dz - r.a[0] * oz;
    r.a[1] = sqrtf((rx * rx + ry * ry) + rz * rz);  // inv2 = |dir - inv1 o|
    r.a[2] = dist;
    // torch CosineSimilarity(dim=-1, eps=1e-8): normalise each vector by max(|v|, eps), then dot
    const float dn = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 1e-8f);
    const float ux = edge_row_div<FAST_RCP>(dx, dn), uy = edge_row_div<FAST_RCP>(dy, dn), uz = edge_row_div<FAST_RCP>(dz, dn);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float lx = Lm[3 * i], ly = Lm[3 * i + 1], lz = Lm[3 * i + 2];
        const float ln = fmaxf(sqrtf((lx * lx + ly * ly) + lz * lz), 1e-8f);
        r.a[3 + i] = (ux * edge_row_div<FAST_RCP>(lx, ln) + uy * edge_row_div<FAST_RCP>(ly, ln)) + uz * edge_row_div<FAST_RCP>(lz, ln);
    }
    // smooth cutoff (utils/windowing.py:21-29, p = 6), times (d < r_max)
    const float u = edge_row_div<FAST_RCP>(dist, r_max);
    const float u2 = u * u, u6 = u2 * u2 * u2;
    const float w = 1.0f - 28.0f * u6 + 48.0f * u6 * u - 21.0f * u6 * u2;
    r.window = (valid && dist < r_max) ? w : 0.0f;
    return r;
}
