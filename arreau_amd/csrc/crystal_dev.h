// Device helpers shared by the per-crystal kernels (one workgroup of CRYSTAL_WAVES waves per crystal): screen.hip, fingerprint.hip,
// coordination.hip, bond_order.hip, voronoi.hip, contact_guide.hip, symfind.hip, reduce.hip, symmetrize.hip, conventional.hip,
// match.hip, xrd.hip and ewald.hip.  What is here: the image walk (the flattened range e = j M + m dealt to threads by stride or in chunks, with 32-bit
// index arithmetic where the range allows it); the launch shape; the prologue; the wrap of a fractional coordinate and the
// Cartesian position; the positions staged in LDS; the cell and its image range; one periodic contact; the wave's butterfly sum and
// its self-synchronisation; the compaction of a workgroup's hits in thread order; the rarest species; the squared length of a
// fractional difference; the matrix of a rotation code, its integer inverse and the metric of a cell's image under it.  One
// float32 rounding per operation.
#pragma once

// ---- the image walk.  Plain C++: tests/crystal_walk_host.cpp compiles this part with the host compiler alone.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CRYSTAL_HD __host__ __device__ __forceinline__
#else
#define CRYSTAL_HD inline
#endif

// whether a walk of `span` entries by steps of `stride` stays inside 32 bits (the index may pass the span by one stride)
CRYSTAL_HD bool crystal_walk_narrow(unsigned long long span, unsigned stride) { return span <= 0xffffffffull - stride; }

// e = j M + m -> (j, m), in the arithmetic of E (unsigned, or unsigned long long where j M + m needs it)
template <class E>
CRYSTAL_HD void crystal_walk_index(E e, unsigned M, unsigned& j, unsigned& m) {
    const E q = e / M;
    j = (unsigned)q; m = (unsigned)(e - q * M);
}

template <class E, class F>
CRYSTAL_HD void crystal_walk_as(E span, unsigned M, E start, unsigned stride, F& fn) {
    for (E e = start; e < span; e += stride) {
        unsigned j, m;
        crystal_walk_index(e, M, j, m);
        fn(j, m);
    }
}

template <class E, class F>
CRYSTAL_HD void crystal_walk_chunks_as(E span, unsigned M, unsigned lane, unsigned width, F& fn) {
    for (E base = 0; base < span; base += width) {
        const E e = base + lane;
        unsigned j, m;
        crystal_walk_index(e, M, j, m);
        fn(e < span, j, m);
    }
}

// fn(j, m) for e = start, start + stride, ... < span, ascending: a thread's or a lane's share of the range
template <class F>
CRYSTAL_HD void crystal_walk(unsigned long long span, unsigned M, unsigned long long start, unsigned stride, F&& fn) {
    if (crystal_walk_narrow(span, stride) && start <= 0xffffffffull)  // (uniform) the usual case
        crystal_walk_as<unsigned>((unsigned)span, M, (unsigned)start, stride, fn);
    else
        crystal_walk_as<unsigned long long>(span, M, start, stride, fn);
}

// fn(valid, j, m) for e = lane, lane + width, ... in rounds of `width` entries (lane < width): every thread of the wave or the
// workgroup calls fn in every round, whether its own entry lies inside the span (valid) or not, so fn may hold ballots and barriers
template <class F>
CRYSTAL_HD void crystal_walk_chunks(unsigned long long span, unsigned M, unsigned lane, unsigned width, F&& fn) {
    if (crystal_walk_narrow(span, width))  // (uniform) the usual case
        crystal_walk_chunks_as<unsigned>((unsigned)span, M, lane, width, fn);
    else
        crystal_walk_chunks_as<unsigned long long>(span, M, lane, width, fn);
}

#if defined(__HIPCC__)  // ---- everything below is device code

#define CRYSTAL_WAVES 4
#define CRYSTAL_THREADS (64 * CRYSTAL_WAVES)
#define CRYSTAL_LDS_ATOMS 256  // crystals of up to this many atoms keep their per-atom data in LDS
#define SYM_CODES 19683        // 3^9 rotation codes (the symmetry search's; symmetrize.hip reads them)

// every fp32 operation below is spelled out (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn): one rounding each, no contraction
// to an FMA, so that the float32 host restatement (arreau_amd/diffusion/crystal_batch.py, screening.py) matches bit for bit
__device__ __forceinline__ float dot3_rn(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

__device__ __forceinline__ void cross_rn(const float* u, const float* v, float* o) {
    o[0] = __fsub_rn(__fmul_rn(u[1], v[2]), __fmul_rn(u[2], v[1]));
    o[1] = __fsub_rn(__fmul_rn(u[2], v[0]), __fmul_rn(u[0], v[2]));
    o[2] = __fsub_rn(__fmul_rn(u[0], v[1]), __fmul_rn(u[1], v[0]));
}

// (n_0 L_0d + n_1 L_1d) + n_2 L_2d: component d of a combination of the cell rows
__device__ __forceinline__ float rows_rn(const float* Lm, int d, float n0, float n1, float n2) {
    return __fadd_rn(__fadd_rn(__fmul_rn(n0, Lm[d]), __fmul_rn(n1, Lm[3 + d])), __fmul_rn(n2, Lm[6 + d]));
}

// w = f - floor(f), a result of 1 (a tiny negative f) becomes 0; then arreau_cart_component's expression on the wrapped
// coordinates, uncontracted
__device__ __forceinline__ float crystal_wrap(float f) {
    const float w = __fsub_rn(f, floorf(f));
    return w >= 1.0f ? 0.0f : w;
}

__device__ __forceinline__ float crystal_cart(const float* __restrict__ frac, const float* Lm, size_t atom, int d) {
    return rows_rn(Lm, d, crystal_wrap(frac[3 * atom]), crystal_wrap(frac[3 * atom + 1]), crystal_wrap(frac[3 * atom + 2]));
}

// The Cartesian positions of a crystal's atoms: staged in LDS when the crystal fits, else formed from global memory where they
// are used (the same values).  crystal_stage_positions fills the caller's spos[3 * CRYSTAL_LDS_ATOMS]; one barrier, every thread
// calls it (what else a caller stages ahead of the call is visible after it too).
struct crystal_positions {
    const float *spos, *frac, *Lm;
    size_t first;
    bool staged;
    __device__ __forceinline__ float operator()(int atom, int d) const { return staged ? spos[3 * atom + d] : crystal_cart(frac, Lm, first + atom, d); }
};

__device__ __forceinline__ crystal_positions crystal_stage_positions(float* spos, const float* __restrict__ frac, const float* Lm, int first, int n) {
    const bool staged = n <= CRYSTAL_LDS_ATOMS;
    if (staged)
        for (int a = threadIdx.x; a < 3 * n; a += CRYSTAL_THREADS) spos[a] = crystal_cart(frac, Lm, (size_t)first + a / 3, a % 3);
    __syncthreads();
    return {spos, frac, Lm, (size_t)first, staged};
}

// Crystal b's atom range (first, n), clamped into [0, N] so that a bad offset table cannot make a kernel read outside frac / types,
// its cell Lm[9], and whether a cell entry or a coordinate is not finite (workgroup-uniform: one barrier, every thread calls it);
// `before_barrier` is a caller's own pass over its inputs, run ahead of that barrier so that its loads overlap the others.
template <class Extra>
__device__ __forceinline__ bool crystal_prologue(const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets,
                                                 int b, int N, int& first, int& n, float* Lm, Extra&& before_barrier) {
    first = offsets[b];
    int last = offsets[b + 1];
    first = first < 0 ? 0 : (first > N ? N : first);
    last = last < first ? first : (last > N ? N : last);
    n = last - first;
    int bad = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        Lm[q] = lattice[9 * (size_t)b + q];
        bad |= !isfinite(Lm[q]);
    }
    for (int a = threadIdx.x; a < 3 * n; a += CRYSTAL_THREADS) bad |= !isfinite(frac[3 * (size_t)first + a]);
    before_barrier();
    return __syncthreads_or(bad);
}

// The cell as the contact search sees it: volume, shell quotients q_k = radius / (spacing of the planes across axis k); once the
// caller has accepted the cell by its own rule, the images per axis N_k, W_k = 2 N_k + 1, their number M, the index of (0, 0, 0).
struct crystal_cell {
    float volume, q[3];
    int N1, N2, N3;
    unsigned W2, W3, M, centre;
};

__device__ __forceinline__ float crystal_volume(const float* Lm) {
    float c0[3];
    cross_rn(Lm + 3, Lm + 6, c0);
    return fabsf(dot3_rn(Lm[0], Lm[1], Lm[2], c0[0], c0[1], c0[2]));
}

// fills volume and q; true when the volume is not finite or an axis needs more than max_shells images (every caller's CELL rule)
__device__ __forceinline__ bool crystal_cell_measure(const float* Lm, float radius, int max_shells, crystal_cell& c) {
    c.volume = crystal_volume(Lm);
    bool unbounded = !isfinite(c.volume);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float ck[3];
        cross_rn(Lm + 3 * ((k + 1) % 3), Lm + 3 * ((k + 2) % 3), ck);
        c.q[k] = __fdiv_rn(radius, __fdiv_rn(c.volume, sqrtf(dot3_rn(ck[0], ck[1], ck[2], ck[0], ck[1], ck[2]))));
        unbounded |= !(c.q[k] <= (float)max_shells);
    }
    return unbounded;
}

// q_k <= max_shells <= 8 in an accepted cell, so N_k <= 8 and M <= 17^3
__device__ __forceinline__ void crystal_cell_images(crystal_cell& c) {
    c.N1 = max(1, (int)ceilf(c.q[0])); c.N2 = max(1, (int)ceilf(c.q[1])); c.N3 = max(1, (int)ceilf(c.q[2]));
    c.W2 = 2u * c.N2 + 1u; c.W3 = 2u * c.N3 + 1u; c.M = (2u * c.N1 + 1u) * c.W2 * c.W3;
    c.centre = ((unsigned)c.N1 * c.W2 + (unsigned)c.N2) * c.W3 + (unsigned)c.N3;
}

// image m -> (n1, n2, n3), images in lexicographic order
__device__ __forceinline__ void crystal_image(const crystal_cell& c, unsigned m, int* im) {
    const unsigned m12 = m / c.W3;
    im[0] = (int)(m12 / c.W2) - c.N1; im[1] = (int)(m12 % c.W2) - c.N2; im[2] = (int)(m - m12 * c.W3) - c.N3;
}

// Receiver i at (pix, piy, piz) and image m of sender j: the image (n1, n2, n3), the shift s = (n1 L_0 + n2 L_1) + n3 L_2, the
// displacement (p_j + s) - p_i and d2 = (dx dx + dy dy) + dz dz, in the one operation order every contact search uses.
struct crystal_contact {
    int n1, n2, n3;
    float dx, dy, dz, d2;
};

template <class Position>
__device__ __forceinline__ crystal_contact crystal_contact_at(const crystal_cell& c, const float* Lm, const Position& position, int j, unsigned m,
                                                              float pix, float piy, float piz) {
    int im[3];
    crystal_image(c, m, im);
    crystal_contact k{im[0], im[1], im[2]};
    const float n1 = (float)im[0], n2 = (float)im[1], n3 = (float)im[2];
    const float sx = rows_rn(Lm, 0, n1, n2, n3), sy = rows_rn(Lm, 1, n1, n2, n3), sz = rows_rn(Lm, 2, n1, n2, n3);
    k.dx = __fsub_rn(__fadd_rn(position(j, 0), sx), pix);
    k.dy = __fsub_rn(__fadd_rn(position(j, 1), sy), piy);
    k.dz = __fsub_rn(__fadd_rn(position(j, 2), sz), piz);
    k.d2 = dot3_rn(k.dx, k.dy, k.dz, k.dx, k.dy, k.dz);
    return k;
}

// v <- v + shuffle_xor(v, w), w = 32 .. 1: the wave's sum in a fixed order; every lane ends with the same bits (a + b == b + a)
__device__ __forceinline__ float crystal_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off));
    return v;
}

// A wave that talks to itself: what one lane wrote (LDS or global memory) is read by the other lanes of its wave after this
__device__ __forceinline__ void crystal_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// This thread's rank among the workgroup's hits, in thread order, and their number.  One barrier, every thread calls it; `slots`
// are CRYSTAL_WAVES ints in LDS which the caller keeps unwritten until every thread has read them.
__device__ __forceinline__ int crystal_compact(bool hit, int lane, int wave, int* slots, int& total) {
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) slots[wave] = __popcll(mask);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < CRYSTAL_WAVES; ++w) {
        const int k = slots[w];
        before += w < wave ? k : 0;
        total += k;
    }
    return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// The species with the fewest atoms (the smallest id on ties) and p0, its first atom (n >= 1): what the candidate translations of
// symfind.hip and reduce.hip start from.  Key (count, id with the sign bit flipped: unsigned order = signed order), minimum over
// the wave by shuffles, over the waves through LDS.  Two barriers inside, every thread calls it; s_ka / s_kb are CRYSTAL_WAVES
// words of LDS each, read by every thread until its return.
template <class Species>
__device__ __forceinline__ int crystal_rarest_species(int n, int lane, int wave, Species&& species, unsigned* s_ka, unsigned* s_kb, int& p0) {
    const int tid = threadIdx.x;
    unsigned ka = 0xffffffffu, kb = 0xffffffffu;
    for (int a = tid; a < n; a += CRYSTAL_THREADS) {
        const int ta = species(a);
        unsigned cnt = 0;
        for (int j = 0; j < n; ++j) cnt += species(j) == ta ? 1u : 0u;
        const unsigned tb = (unsigned)ta ^ 0x80000000u;
        if (cnt < ka || (cnt == ka && tb < kb)) { ka = cnt; kb = tb; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned oa = __shfl_xor(ka, off), ob = __shfl_xor(kb, off);
        if (oa < ka || (oa == ka && ob < kb)) { ka = oa; kb = ob; }
    }
    if (lane == 0) { s_ka[wave] = ka; s_kb[wave] = kb; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < CRYSTAL_WAVES; ++w)
        if (s_ka[w] < ka || (s_ka[w] == ka && s_kb[w] < kb)) { ka = s_ka[w]; kb = s_kb[w]; }
    const int rare = (int)(kb ^ 0x80000000u);
    __syncthreads();  // (s_ka is written again below)
    unsigned p0u = 0xffffffffu;
    for (int a = tid; a < n; a += CRYSTAL_THREADS)
        if (species(a) == rare) { p0u = (unsigned)a; break; }  // (ascending a: the thread's first is its smallest)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p0u = min(p0u, (unsigned)__shfl_xor(p0u, off));
    if (lane == 0) s_ka[wave] = p0u;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < CRYSTAL_WAVES; ++w) p0u = min(p0u, s_ka[w]);
    p0 = (int)p0u;  // n >= 1, so the species exists
    return rare;
}

// |c|^2 of c_d = (e_0 L_0d + e_1 L_1d) + e_2 L_2d: the Cartesian image of a fractional difference (the symmetry search's rule 4)
__device__ __forceinline__ float crystal_frac_d2(float e0, float e1, float e2, const float* Lm) {
    const float cx = rows_rn(Lm, 0, e0, e1, e2), cy = rows_rn(Lm, 1, e0, e1, e2), cz = rows_rn(Lm, 2, e0, e1, e2);
    return dot3_rn(cx, cy, cz, cx, cy, cz);
}

// the matrix of a rotation code, W[3 r + c] = digit (3 r + c) - 1, and its determinant
__device__ __forceinline__ int decode_rotation(int code, int* W) {
#pragma unroll
    for (int p = 0; p < 9; ++p) {
        W[p] = code % 3 - 1;
        code /= 3;
    }
    return W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
}

// (W v)_r = (W_r0 v_0 + W_r1 v_1) + W_r2 v_2: the products by -1, 0, 1 are exact, two rounded sums
__device__ __forceinline__ float rot_row(const float* W, int r, float v0, float v1, float v2) {
    return __fadd_rn(__fadd_rn(__fmul_rn(W[3 * r], v0), __fmul_rn(W[3 * r + 1], v1)), __fmul_rn(W[3 * r + 2], v2));
}

// a'_j = (W_0j a_0 + W_1j a_1) + W_2j a_2 (the search's rule 2) and the six scalar products 00, 11, 22, 01, 02, 12 of the images
__device__ __forceinline__ void image_metric(const int* W, const float* Lm, float* g) {
    float img[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int d = 0; d < 3; ++d) img[3 * j + d] = rows_rn(Lm, d, (float)W[j], (float)W[3 + j], (float)W[6 + j]);
    const int pi[6] = {0, 1, 2, 0, 0, 1}, pj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int e = 0; e < 6; ++e)
        g[e] = dot3_rn(img[3 * pi[e]], img[3 * pi[e] + 1], img[3 * pi[e] + 2], img[3 * pj[e]], img[3 * pj[e] + 1], img[3 * pj[e] + 2]);
}

// the integer inverse of a matrix of determinant det = +-1: its adjugate times det
__device__ __forceinline__ void inverse_rotation(const int* W, int det, float* V) {
    V[0] = (float)(det * (W[4] * W[8] - W[5] * W[7])); V[1] = (float)(det * (W[2] * W[7] - W[1] * W[8])); V[2] = (float)(det * (W[1] * W[5] - W[2] * W[4]));
    V[3] = (float)(det * (W[5] * W[6] - W[3] * W[8])); V[4] = (float)(det * (W[0] * W[8] - W[2] * W[6])); V[5] = (float)(det * (W[2] * W[3] - W[0] * W[5]));
    V[6] = (float)(det * (W[3] * W[7] - W[4] * W[6])); V[7] = (float)(det * (W[1] * W[6] - W[0] * W[7])); V[8] = (float)(det * (W[0] * W[4] - W[1] * W[3]));
}

#endif  // __HIPCC__
