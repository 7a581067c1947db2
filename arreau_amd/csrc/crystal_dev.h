// Device helpers shared by the kernels that enumerate a crystal's periodic contacts (screen.hip, fingerprint.hip): the cell's
// cross products, the wrap of a fractional coordinate and the Cartesian position, one float32 rounding per operation.
#pragma once
#include <hip/hip_runtime.h>

// every fp32 operation below is spelled out (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn): one rounding each, no contraction
// to an FMA, so that the float32 host restatement (arreau_amd/diffusion/screening.py) matches bit for bit
__device__ __forceinline__ float dot3_rn(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

__device__ __forceinline__ void cross_rn(const float* u, const float* v, float* o) {
    o[0] = __fsub_rn(__fmul_rn(u[1], v[2]), __fmul_rn(u[2], v[1]));
    o[1] = __fsub_rn(__fmul_rn(u[2], v[0]), __fmul_rn(u[0], v[2]));
    o[2] = __fsub_rn(__fmul_rn(u[0], v[1]), __fmul_rn(u[1], v[0]));
}

// w = f - floor(f), a result of 1 (a tiny negative f) becomes 0; then arreau_cart_component's expression on the wrapped
// coordinates, uncontracted
__device__ __forceinline__ float crystal_wrap(float f) {
    const float w = __fsub_rn(f, floorf(f));
    return w >= 1.0f ? 0.0f : w;
}

__device__ __forceinline__ float crystal_cart(const float* __restrict__ frac, const float* Lm, size_t atom, int d) {
    const float w0 = crystal_wrap(frac[3 * atom]), w1 = crystal_wrap(frac[3 * atom + 1]), w2 = crystal_wrap(frac[3 * atom + 2]);
    return __fadd_rn(__fadd_rn(__fmul_rn(w0, Lm[d]), __fmul_rn(w1, Lm[3 + d])), __fmul_rn(w2, Lm[6 + d]));
}
