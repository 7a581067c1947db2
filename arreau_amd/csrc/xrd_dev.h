// The reflection walk of the powder pattern, shared by xrd.hip (arreau_crystal_xrd) and xrd_guide.hip (XRD guidance): the host's
// plan of a launch (rule 1 of the xrd section of include/arreau_hip.h), the cell and its box (rules 2 and 3), one box entry's
// reflection (rules 4-6), one Gaussian term (rule 7's expression and its 6 sigma test) and the whole forward walk into a pattern
// in LDS (rule 7).  Both kernels run this code and no copy of it, so the guidance kernel's pattern is the xrd launch's bit for
// bit.  The flat range dealt to the threads (crystal_walk_chunks) is the box index e = (h W_2 + (k + H_2)) W_3 + (l + H_3).
// ewald.hip (arreau_crystal_ewald) takes the parts that know nothing of a pattern: the cell (xrd_cell_rows), the box under its own
// cut (xrd_cell_box), the box walk, a box entry's lattice point (xrd_point_at), the atoms and the reduced phase.
#pragma once
#include "internal.h"
#include "crystal_dev.h"

// what the host derives from arreau_xrd_params in float64, once per launch (rule 1)
struct xrd_plan {
    double wavelength, g0, g1, step;  // the grid: g_p = g0 + p step, g_{n-1} = g1
    double sigma, six_sigma, norm;    // degrees; norm = 1 / (sigma sqrt(2 pi))
    double dlo2, dhi2, dhi;           // the cut on d*^2 and d*_max
    double b_iso;
    int n_points, max_index;
};

// ARREAU_EINVAL unless `params` is given and passes the xrd launch's validation (messages under `who`); fills *plan (xrd.hip)
int arreau_xrd_plan_of(const arreau_xrd_params* params, const char* who, xrd_plan* plan);

#if defined(__HIPCC__)

// rules 2 and 3: the reciprocal rows b_k (R[3 k ..]), 1 / V^2, the box and the float32 volume the screen's expression gives
struct xrd_cell {
    double R[9], inv_v2;
    int H1, H2, H3;
    float volume;
};

// rule 2: the cell A[9] in float64 from the float32 entries, the unnormalised reciprocal rows a_i x a_j in c.R, det and the float32
// volume; false when the cell has no volume (the callers' CELL).  xrd_cell_box finishes c.
__device__ __forceinline__ bool xrd_cell_rows(const float* Lm, xrd_cell& c, double* A, double& det) {
    c.volume = crystal_volume(Lm);
#pragma unroll
    for (int q = 0; q < 9; ++q) A[q] = (double)Lm[q];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* u = A + 3 * ((k + 1) % 3);
        const double* v = A + 3 * ((k + 2) % 3);
        c.R[3 * k] = u[1] * v[2] - u[2] * v[1]; c.R[3 * k + 1] = u[2] * v[0] - u[0] * v[2]; c.R[3 * k + 2] = u[0] * v[1] - u[1] * v[0];
    }
    det = (A[0] * c.R[0] + A[1] * c.R[1]) + A[2] * c.R[2];
    const double V = fabs(det);
    return c.volume > 0.f && isfinite(c.volume) && V > 0. && isfinite(V);
}

// rule 3: the box H_k = floor(g_max |a_k|) from the direct cell's lengths, then b_k = (a_i x a_j) / det and 1 / V^2; false when
// an H_k exceeds max_index (the callers' RANGE; c.R is then left unnormalised)
__device__ __forceinline__ bool xrd_cell_box(const double* A, double det, double g_max, int max_index, xrd_cell& c) {
    double Hd[3];
    bool wide = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Hd[k] = floor(g_max * sqrt((A[3 * k] * A[3 * k] + A[3 * k + 1] * A[3 * k + 1]) + A[3 * k + 2] * A[3 * k + 2]));
        wide |= !(Hd[k] <= (double)max_index);
    }
    if (wide) return false;
    c.H1 = (int)Hd[0]; c.H2 = (int)Hd[1]; c.H3 = (int)Hd[2];  // <= max_index <= 127
#pragma unroll
    for (int q = 0; q < 9; ++q) c.R[q] /= det;
    const double V = fabs(det);
    c.inv_v2 = 1.0 / (V * V);
    return true;
}

// 0, or the one of ARREAU_XRD_CELL / EMPTY / RANGE that applies (in that order); every thread computes the same values
__device__ __forceinline__ int xrd_cell_measure(const float* Lm, int n, const xrd_plan& P, xrd_cell& c) {
    double A[9], det;
    if (!xrd_cell_rows(Lm, c, A, det)) return ARREAU_XRD_CELL;
    if (n == 0) return ARREAU_XRD_EMPTY;
    if (!xrd_cell_box(A, det, P.dhi, P.max_index, c)) return ARREAU_XRD_RANGE;
    return 0;
}

// The atoms of a crystal as the structure factor reads them: wrapped coordinates and amplitudes, from LDS when staged, else formed
// from global memory where they are used (the same values).
struct xrd_atoms {
    const float *s_x, *s_w, *frac, *weights;
    size_t first;
    bool staged;
    __device__ __forceinline__ void operator()(int a, float& x, float& y, float& z, float& w) const {
        if (staged) {
            x = s_x[3 * a]; y = s_x[3 * a + 1]; z = s_x[3 * a + 2]; w = s_w[a];
        } else {
            const size_t g = first + a;
            x = crystal_wrap(frac[3 * g]); y = crystal_wrap(frac[3 * g + 1]); z = crystal_wrap(frac[3 * g + 2]); w = weights[g];
        }
    }
};

// the reduced phase of reflection (h, k, l) at a wrapped position, in revolutions (rule 5): t = (h x + k y) + l z, t - rint(t)
__device__ __forceinline__ float xrd_phase(float hf, float kf, float lf, float x, float y, float z) {
    const float t = __fadd_rn(__fadd_rn(__fmul_rn(hf, x), __fmul_rn(kf, y)), __fmul_rn(lf, z));
    return __fsub_rn(t, rintf(t));
}

// One box entry (rules 4-6).  kappa is what multiplies |F|^2 in rule 6, 2 DW LP / V^2 norm; G = (gx, gy, gz) the reciprocal
// vector; lo..hi the grid points that may lie inside the window, one to spare on either side (rule 7 tests each).
struct xrd_reflection {
    bool keep;
    int h, k, l, lo, hi;
    double gx, gy, gz, tt, kappa;
    float re, im, amp;
};

// the lattice point of box entry (uh, m) (rule 4): its indices, whether it lies in the walked half space and then G and d*^2, float64
struct xrd_point {
    bool half;
    int h, k, l;
    double gx, gy, gz, d2;
};

__device__ __forceinline__ xrd_point xrd_point_at(const xrd_cell& c, bool valid, unsigned uh, unsigned m) {
    const unsigned W3 = 2u * c.H3 + 1u;
    const unsigned uk = m / W3;
    const double* R = c.R;
    xrd_point p{};
    const int h = (int)uh, k = (int)uk - c.H2, l = (int)(m - uk * W3) - c.H3;
    p.h = h; p.k = k; p.l = l;
    p.half = valid && (h > 0 || k > 0 || (k == 0 && l > 0));  // (h >= 0 in the box)
    if (p.half) {
        p.gx = ((double)h * R[0] + (double)k * R[3]) + (double)l * R[6];
        p.gy = ((double)h * R[1] + (double)k * R[4]) + (double)l * R[7];
        p.gz = ((double)h * R[2] + (double)k * R[5]) + (double)l * R[8];
        p.d2 = (p.gx * p.gx + p.gy * p.gy) + p.gz * p.gz;
    }
    return p;
}

__device__ __forceinline__ xrd_reflection xrd_reflection_at(const xrd_plan& P, const xrd_cell& c, int n, const xrd_atoms& atoms, bool valid,
                                                            unsigned uh, unsigned m) {
    xrd_reflection r{};
    // ---- rule 4: the half space, d*^2 and the cut, float64
    const xrd_point pt = xrd_point_at(c, valid, uh, m);
    const int h = pt.h, k = pt.k, l = pt.l;
    r.h = h; r.k = k; r.l = l;
    r.lo = 0; r.hi = -1;
    const double d2 = pt.d2;
    const bool keep = pt.half && d2 >= P.dlo2 && d2 <= P.dhi2;
    if (pt.half) {
        r.gx = pt.gx; r.gy = pt.gy; r.gz = pt.gz;
    }
    r.keep = keep;
    if (keep) {
        // ---- rule 5: the structure factor, float32 in atom order, the phase in revolutions
        const float hf = (float)h, kf = (float)k, lf = (float)l;
        float re = 0.f, im = 0.f;
        for (int a = 0; a < n; ++a) {
            float x, y, z, w;
            atoms(a, x, y, z, w);
            float s, co;
            sincospif(__fmul_rn(2.0f, xrd_phase(hf, kf, lf, x, y, z)), &s, &co);
            re = __fadd_rn(re, __fmul_rn(w, co));
            im = __fadd_rn(im, __fmul_rn(w, s));
        }
        // ---- rule 6: the angle and the intensity, float64
        const double deg = 57.29577951308232087680;  // 180 / pi
        const double inv_step = 1.0 / P.step, last = (double)(P.n_points - 1);
        const double sth = 0.5 * P.wavelength * sqrt(d2), s2 = sth * sth, c2t = 1.0 - 2.0 * s2;
        const double lp = (1.0 + c2t * c2t) / (s2 * sqrt(1.0 - s2));
        const double f2 = (double)re * (double)re + (double)im * (double)im;
        const double dw = P.b_iso != 0. ? exp(-0.5 * P.b_iso * d2) : 1.0;  // exp(-B s^2)^2, s = d* / 2
        r.tt = 2.0 * deg * asin(sth);
        r.amp = (float)((2.0 * f2 * dw * lp * c.inv_v2) * P.norm);
        r.kappa = (2.0 * dw * lp * c.inv_v2) * P.norm;
        r.re = re; r.im = im;
        // the grid points that may lie inside the window, one to spare on either side; rule 7 tests each
        const double flo = floor((r.tt - P.six_sigma - P.g0) * inv_step), fhi = ceil((r.tt + P.six_sigma - P.g0) * inv_step);
        r.lo = (int)fmin(fmax(flo, 0.), last);
        r.hi = (int)fmin(fmax(fhi, 0.), last);
    }
    return r;
}

// rule 7's term of grid point p for a reflection at 2 theta = te: whether p lies within 6 sigma, and then G = expf(-0.5 z^2)
__device__ __forceinline__ bool xrd_gaussian(const xrd_plan& P, int p, double te, double inv_sigma, float& G) {
    const double dd = (p == P.n_points - 1 ? P.g1 : P.g0 + (double)p * P.step) - te;
    if (!(fabs(dd) <= P.six_sigma)) return false;
    const float z = (float)(dd * inv_sigma);
    G = expf(__fmul_rn(-0.5f, __fmul_rn(z, z)));
    return true;
}

// the box walk: fn(valid, h, m) for every thread in every round of CRYSTAL_THREADS box entries (fn may hold barriers)
template <class F>
__device__ __forceinline__ void xrd_box_walk(const xrd_cell& c, F&& fn) {
    const unsigned W2 = 2u * c.H2 + 1u, W3 = 2u * c.H3 + 1u, M = W2 * W3;
    const unsigned long long span = (unsigned long long)(c.H1 + 1) * M;  // <= 128 * 255^2
    crystal_walk_chunks(span, M, (unsigned)threadIdx.x, (unsigned)CRYSTAL_THREADS, fn);
}

// a round's list of kept reflections in LDS (CRYSTAL_THREADS entries each) and the CRYSTAL_WAVES slots of crystal_compact
struct xrd_round_lds {
    double* tt;
    float* amp;
    int *lo, *hi, *slots;
};

// The forward walk: s_pat [n_points] (zeroed by the caller, a barrier since) receives the pattern; returns the kept reflections of
// the half space.  A round's kept reflections are compacted in thread order and added one after another; thread t owns the grid
// points p = t (mod CRYSTAL_THREADS) throughout, so every point receives its terms in ascending box index, and after the walk a
// thread may read its own points without a barrier.
__device__ __forceinline__ int xrd_pattern_walk(const xrd_plan& P, const xrd_cell& c, int n, const xrd_atoms& atoms, float* s_pat,
                                                const xrd_round_lds& L) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double inv_sigma = 1.0 / P.sigma;
    int kept = 0;
    xrd_box_walk(c, [&](bool valid, unsigned uh, unsigned m) {
        const xrd_reflection r = xrd_reflection_at(P, c, n, atoms, valid, uh, m);
        int total;
        const int rank = crystal_compact(r.keep, lane, wave, L.slots, total);
        if (r.keep) {
            L.tt[rank] = r.tt; L.amp[rank] = r.amp; L.lo[rank] = r.lo; L.hi[rank] = r.hi;
        }
        __syncthreads();  // (also: every thread has read the slots before the next round writes them)
        // ---- rule 7: the round's reflections in ascending box index; this thread's points are p = tid (mod 256)
        for (int e = 0; e < total; ++e) {
            const int elo = L.lo[e], ehi = L.hi[e];
            const double te = L.tt[e];
            const float ae = L.amp[e];
            for (int p = elo + ((tid - elo) & (CRYSTAL_THREADS - 1)); p <= ehi; p += CRYSTAL_THREADS) {
                float G;
                if (xrd_gaussian(P, p, te, inv_sigma, G)) s_pat[p] = __fadd_rn(s_pat[p], __fmul_rn(ae, G));
            }
        }
        kept += total;
    });
    return kept;
}

#endif  // __HIPCC__
