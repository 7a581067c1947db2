// Conventional cells of a batch of primitive, Delaunay-reduced crystals (arreau_crystal_conventional; the rules are written out
// in include/arreau_hip.h): from the rotations the symmetry search stored for a crystal, its symmetry axes, the conventional basis
// of its crystal family, the centring, the Bravais lattice and the atoms of the conventional cell.  One launch, one workgroup of
// four waves per crystal, no atomics; needs no arreau_model.
//   rotations  the stored codes are sorted: the distinct ones are compacted into LDS in code order by the whole workgroup;
//   basis      one thread: every step is integer arithmetic on at most 48 matrices with entries in {-1, 0, 1}; floats only where
//              the squared lengths of lattice vectors are compared (rules 3, 4), one rounding per operation;
//   atoms      the whole workgroup: output atom k n + i is atom i moved by the k-th centring translation.
// A crystal flagged at any point is copied through.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

#define CONV_RANGE 3     // plane vectors are searched among the integer rows with entries in -CONV_RANGE..CONV_RANGE
#define CONV_MAX_ROT 48  // a lattice has at most 48 isometries

namespace {

struct conv_in {
    const int32_t *n_ops, *ops_rotation, *point_group, *flags;
};

struct conv_out {
    float *lattice, *lengths, *angles;
    int32_t *transform, *centring, *bravais, *n_points, *num_atoms, *flags;
    float* frac_out;
    int32_t *types_out, *source;
};

enum { CEN_P = 0, CEN_A, CEN_B, CEN_C, CEN_I, CEN_F, CEN_R };

__device__ __forceinline__ int idet3(const int* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// adj(M), M adj(M) = det(M) I
__device__ __forceinline__ void iadj3(const int* M, int* A) {
    A[0] = M[4] * M[8] - M[5] * M[7]; A[1] = M[2] * M[7] - M[1] * M[8]; A[2] = M[1] * M[5] - M[2] * M[4];
    A[3] = M[5] * M[6] - M[3] * M[8]; A[4] = M[0] * M[8] - M[2] * M[6]; A[5] = M[2] * M[3] - M[0] * M[5];
    A[6] = M[3] * M[7] - M[4] * M[6]; A[7] = M[1] * M[6] - M[0] * M[7]; A[8] = M[0] * M[4] - M[1] * M[3];
}

__device__ __forceinline__ void imatmul(const int* A, const int* B, int* C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

__device__ __forceinline__ void imatvec(const int* W, const int* v, int* o) {
    for (int r = 0; r < 3; ++r) o[r] = W[3 * r] * v[0] + W[3 * r + 1] * v[1] + W[3 * r + 2] * v[2];
}

__device__ __forceinline__ int igcd(int a, int b) {
    a = abs(a); b = abs(b);
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// v divided by the gcd of its entries, its first non-zero entry made positive; false for the zero vector
__device__ __forceinline__ bool primitive3(int* v) {
    const int g = igcd(igcd(v[0], v[1]), v[2]);
    if (g == 0) return false;
    const int lead = v[0] != 0 ? v[0] : (v[1] != 0 ? v[1] : v[2]);
    const int s = lead < 0 ? -g : g;
    v[0] /= s; v[1] /= s; v[2] /= s;
    return true;
}

// W' = det(W) W and its order from its trace (0: none of 3, -1, 0, 1, 2)
__device__ __forceinline__ int proper_part(const int* W, int det, int* Wp) {
    for (int p = 0; p < 9; ++p) Wp[p] = det * W[p];
    switch (Wp[0] + Wp[4] + Wp[8]) {
        case 3: return 1;
        case -1: return 2;
        case 0: return 3;
        case 1: return 4;
        case 2: return 6;
        default: return 0;
    }
}

// S = sum_{j < order} W'^j: the axis is its first non-zero column, the normal of the perpendicular plane its first non-zero row
__device__ __forceinline__ bool axis_of(const int* Wp, int order, int* axis, int* normal) {
    int S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[9];
    for (int j = 0; j < order; ++j) {
        for (int p = 0; p < 9; ++p) S[p] += M[p];
        imatmul(M, Wp, T);
        for (int p = 0; p < 9; ++p) M[p] = T[p];
    }
    int col = -1, row = -1;
    for (int j = 2; j >= 0; --j) {
        if (S[j] | S[3 + j] | S[6 + j]) col = j;
        if (S[3 * j] | S[3 * j + 1] | S[3 * j + 2]) row = j;
    }
    if (col < 0 || row < 0) return false;
    for (int k = 0; k < 3; ++k) { axis[k] = S[3 * k + col]; normal[k] = S[3 * row + k]; }
    return primitive3(axis) && primitive3(normal);
}

__device__ __forceinline__ void cart3(const int* v, const float* Lm, float* c) {
    for (int d = 0; d < 3; ++d) c[d] = rows_rn(Lm, d, (float)v[0], (float)v[1], (float)v[2]);
}

__device__ __forceinline__ float len2_of(const int* v, const float* Lm) {
    float c[3];
    cart3(v, Lm, c);
    return dot3_rn(c[0], c[1], c[2], c[0], c[1], c[2]);
}

// the centring of a transform of positive determinant: n_points, the sorted numerators pts [n_points, 3] over n_points, and the
// code of the listed set they are (-1: none)
__device__ __forceinline__ int centring_of(const int* P, int& det, int* pts) {
    det = idet3(P);
    for (int k = 0; k < 12; ++k) pts[k] = 0;
    if (det < 1 || det > 4) return -1;
    int A[9];
    iadj3(P, A);
    int count = 0;
    for (int i = 0; i < det; ++i)
        for (int j = 0; j < det; ++j)
            for (int k = 0; k < det; ++k) {
                int p[3];
                for (int c = 0; c < 3; ++c) {
                    p[c] = (i * A[c] + j * A[3 + c] + k * A[6 + c]) % det;
                    if (p[c] < 0) p[c] += det;
                }
                int at = 0;  // sorted insertion, no value twice
                bool have = false;
                for (; at < count; ++at) {
                    const int* q = pts + 3 * at;
                    if (q[0] == p[0] && q[1] == p[1] && q[2] == p[2]) { have = true; break; }
                    if (p[0] < q[0] || (p[0] == q[0] && (p[1] < q[1] || (p[1] == q[1] && p[2] < q[2])))) break;
                }
                if (have) continue;
                if (count == 4) return -1;
                for (int m = count; m > at; --m)
                    for (int c = 0; c < 3; ++c) pts[3 * m + c] = pts[3 * (m - 1) + c];
                for (int c = 0; c < 3; ++c) pts[3 * at + c] = p[c];
                ++count;
            }
    if (count != det) return -1;
    auto is = [&](int k, int x, int y, int z) { return pts[3 * k] == x && pts[3 * k + 1] == y && pts[3 * k + 2] == z; };
    if (det == 1) return CEN_P;
    if (det == 2) return is(1, 0, 1, 1) ? CEN_A : (is(1, 1, 0, 1) ? CEN_B : (is(1, 1, 1, 0) ? CEN_C : (is(1, 1, 1, 1) ? CEN_I : -1)));
    if (det == 3) return (is(1, 1, 2, 2) && is(2, 2, 1, 1)) ? CEN_R : -1;  // obverse; the reverse setting is no listed set
    return (is(1, 0, 2, 2) && is(2, 2, 0, 2) && is(3, 2, 2, 0)) ? CEN_F : -1;
}

// the lexicographically smallest (row-major) right-handed candidate so far
struct best_basis {
    int P[9];
    bool any;
    __device__ void consider(const int* a, int sa, const int* b, int sb, const int* c, int sc) {
        int Q[9];
        for (int k = 0; k < 3; ++k) { Q[k] = sa * a[k]; Q[3 + k] = sb * b[k]; Q[6 + k] = sc * c[k]; }
        if (idet3(Q) <= 0) return;
        bool less = !any;
        if (any)
            for (int p = 0; p < 9; ++p)
                if (Q[p] != P[p]) { less = Q[p] < P[p]; break; }
        if (less) {
            for (int p = 0; p < 9; ++p) P[p] = Q[p];
            any = true;
        }
    }
};

// the shortest non-zero row of the plane normal . v = 0 among the enumerated ones (lexicographic order, v_0 slowest; a strict
// comparison: the first wins); with `apart`, only rows not parallel to it
__device__ __forceinline__ bool shortest_in_plane(const int* normal, const float* Lm, const int* apart, int* best) {
    float best2 = __int_as_float(0x7f800000);
    bool found = false;
    for (int x = -CONV_RANGE; x <= CONV_RANGE; ++x)
        for (int y = -CONV_RANGE; y <= CONV_RANGE; ++y)
            for (int z = -CONV_RANGE; z <= CONV_RANGE; ++z) {
                if ((x | y | z) == 0 || normal[0] * x + normal[1] * y + normal[2] * z != 0) continue;
                if (apart && y * apart[2] - z * apart[1] == 0 && z * apart[0] - x * apart[2] == 0 && x * apart[1] - y * apart[0] == 0) continue;
                const int v[3] = {x, y, z};
                const float l2 = len2_of(v, Lm);
                if (l2 < best2) { best2 = l2; best[0] = x; best[1] = y; best[2] = z; found = true; }
            }
    return found;
}

// the distinct axes of the proper parts of one order, in code order; false when a part has none or there are more than three
__device__ __forceinline__ bool distinct_axes(const int* codes, int nrot, int order, int* axes, int& count) {
    count = 0;
    for (int m = 0; m < nrot; ++m) {
        int W[9], Wp[9], ax[3], nm[3];
        const int det = decode_rotation(codes[m], W);
        if (proper_part(W, det, Wp) != order) continue;
        if (!axis_of(Wp, order, ax, nm)) return false;
        bool have = false;
        for (int k = 0; k < count; ++k) have |= axes[3 * k] == ax[0] && axes[3 * k + 1] == ax[1] && axes[3 * k + 2] == ax[2];
        if (have) continue;
        if (count == 3) return false;
        for (int c = 0; c < 3; ++c) axes[3 * count + c] = ax[c];
        ++count;
    }
    return true;
}

// the first proper part of an order, in code order
__device__ __forceinline__ bool first_of_order(const int* codes, int nrot, int order, int* Wp) {
    for (int m = 0; m < nrot; ++m) {
        int W[9];
        const int det = decode_rotation(codes[m], W);
        if (proper_part(W, det, Wp) == order) return true;
    }
    return false;
}

// rules 2-4: the conventional basis of one crystal family (0 triclinic .. 5 cubic); false: no basis
__device__ bool conventional_basis(const int* codes, int nrot, int family, const float* Lm, int* P) {
    for (int m = 0; m < nrot; ++m) {
        int W[9], Wp[9];
        const int det = decode_rotation(codes[m], W);
        if (proper_part(W, det, Wp) == 0) return false;
    }
    best_basis best;
    best.any = false;
    if (family == 0) {
        const int id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int p = 0; p < 9; ++p) P[p] = id[p];
        return true;
    } else if (family == 1) {
        int Wp[9], b[3], normal[3], a[3], c[3];
        if (!first_of_order(codes, nrot, 2, Wp) || !axis_of(Wp, 2, b, normal)) return false;
        if (!shortest_in_plane(normal, Lm, nullptr, a) || !shortest_in_plane(normal, Lm, a, c)) return false;
        float ca[3], cc[3];
        cart3(a, Lm, ca);
        cart3(c, Lm, cc);
        const int sc = dot3_rn(ca[0], ca[1], ca[2], cc[0], cc[1], cc[2]) > 0.f ? -1 : 1;  // a . c <= 0
        for (int s = 1; s >= -1; s -= 2)
            for (int t = 1; t >= -1; t -= 2) best.consider(a, s, b, t, c, s * sc);
    } else if (family == 2) {
        int axes[9], count;
        if (!distinct_axes(codes, nrot, 2, axes, count) || count != 3) return false;
        float l2[3];
        for (int k = 0; k < 3; ++k) l2[k] = len2_of(axes + 3 * k, Lm);
        int order[3];  // by squared length, ties to the lower index
        for (int k = 0; k < 3; ++k) {
            int rank = 0;
            for (int j = 0; j < 3; ++j) rank += (l2[j] < l2[k] || (l2[j] == l2[k] && j < k)) ? 1 : 0;
            order[rank] = k;
        }
        int Q[9], det, pts[12];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Q[3 * r + c] = axes[3 * order[r] + c];
        if (idet3(Q) < 0)
            for (int p = 0; p < 9; ++p) Q[p] = -Q[p];
        const int centring = centring_of(Q, det, pts);
        int s[3] = {order[0], order[1], order[2]};
        if (centring == CEN_A) { s[0] = order[1]; s[1] = order[2]; s[2] = order[0]; }       // the centred face becomes C
        else if (centring == CEN_B) { s[1] = order[2]; s[2] = order[1]; }
        for (int p = 1; p >= -1; p -= 2)
            for (int q = 1; q >= -1; q -= 2)
                for (int r = 1; r >= -1; r -= 2) best.consider(axes + 3 * s[0], p, axes + 3 * s[1], q, axes + 3 * s[2], r);
    } else if (family == 3 || family == 4) {
        const int n = family == 3 ? 4 : 3;
        int main_part[9], R[9], Rinv[9], T[9], c[3], normal[3], a0[3];
        int main_order = n;
        if (family == 4 && first_of_order(codes, nrot, 6, main_part)) main_order = 6;
        else if (!first_of_order(codes, nrot, n, main_part)) return false;
        if (!first_of_order(codes, nrot, n, R) || !axis_of(main_part, main_order, c, normal)) return false;
        imatmul(R, R, Rinv);  // R^(n-1)
        if (n == 4) {
            imatmul(Rinv, R, T);
            for (int p = 0; p < 9; ++p) Rinv[p] = T[p];
        }
        if (!shortest_in_plane(normal, Lm, nullptr, a0)) return false;
        int a[3] = {a0[0], a0[1], a0[2]};
        for (int j = 0; j < n; ++j) {  // the vectors the group maps the shortest onto: +-R^j a0
            for (int s = 1; s >= -1; s -= 2) {
                const int as[3] = {s * a[0], s * a[1], s * a[2]};
                for (int k = 0; k < 2; ++k) {
                    int b[3], Q[9], det, pts[12];
                    imatvec(k == 0 ? R : Rinv, as, b);
                    for (int d = 0; d < 3; ++d) { Q[d] = as[d]; Q[3 + d] = b[d]; Q[6 + d] = c[d]; }
                    if (idet3(Q) <= 0) continue;
                    if (family == 4 && idet3(Q) == 3 && centring_of(Q, det, pts) != CEN_R) continue;  // the obverse setting
                    best.consider(as, 1, b, 1, c, 1);
                }
            }
            int next[3];
            imatvec(R, a, next);
            for (int d = 0; d < 3; ++d) a[d] = next[d];
        }
    } else {
        int axes[9], count, Wp[9];
        const int order = first_of_order(codes, nrot, 4, Wp) ? 4 : 2;
        if (!distinct_axes(codes, nrot, order, axes, count) || count != 3) return false;
        const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        for (int m = 0; m < 6; ++m)
            for (int p = 1; p >= -1; p -= 2)
                for (int q = 1; q >= -1; q -= 2)
                    for (int r = 1; r >= -1; r -= 2) best.consider(axes + 3 * perm[m][0], p, axes + 3 * perm[m][1], q, axes + 3 * perm[m][2], r);
    }
    if (!best.any) return false;
    for (int p = 0; p < 9; ++p) P[p] = best.P[p];
    return true;
}

// (family, centring) -> bravais code 0..13 (aP, mP, mS, oP, oS, oI, oF, tP, tI, hR, hP, cP, cI, cF), -1: not admitted
__device__ __forceinline__ int bravais_of(int family, int centring) {
    switch (family) {
        case 0: return centring == CEN_P ? 0 : -1;
        case 1: return centring == CEN_P ? 1 : ((centring == CEN_A || centring == CEN_C || centring == CEN_I) ? 2 : -1);
        case 2: return centring == CEN_P ? 3 : (centring == CEN_C ? 4 : (centring == CEN_I ? 5 : (centring == CEN_F ? 6 : -1)));
        case 3: return centring == CEN_P ? 7 : (centring == CEN_I ? 8 : -1);
        case 4: return centring == CEN_R ? 9 : (centring == CEN_P ? 10 : -1);
        default: return centring == CEN_P ? 11 : (centring == CEN_I ? 12 : (centring == CEN_F ? 13 : -1));
    }
}

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_conventional_kernel(
    const float* __restrict__ frac, const int32_t* __restrict__ types, const float* __restrict__ lattice,
    const int32_t* __restrict__ offsets, int B, int N, int max_ops, conv_in f, conv_out o) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ int s_code[CONV_MAX_ROT];
    __shared__ int s_slots[CRYSTAL_WAVES];
    __shared__ int s_P[9], s_adj[9], s_pts[12];
    __shared__ int s_flags, s_det;

    // ---- rule 1: NONFINITE alone, else CELL | EMPTY, else NO_GROUP (all workgroup-uniform)
    int flags = 0, nops = 0, pg = -1;
    if (bad) flags = ARREAU_CONV_NONFINITE;
    else {
        const float volume = crystal_volume(Lm);
        flags = ((!(volume > 0.f) || !isfinite(volume)) ? ARREAU_CONV_CELL : 0) | (n == 0 ? ARREAU_CONV_EMPTY : 0);
    }
    if (!flags) {
        nops = f.n_ops[b];
        pg = f.point_group[b];
        const int searched = f.flags[b];
        if ((searched & (ARREAU_SYM_AMBIGUOUS | ARREAU_SYM_OVERFLOW | ARREAU_SYM_NOT_A_GROUP)) || nops < 1 || nops > max_ops || pg < 0 || pg > 31)
            flags = ARREAU_CONV_NO_GROUP;
    }

    // ---- the distinct rotations in code order (the stored operations come sorted by code)
    int nrot = 0;
    if (!flags) {
        const int32_t* rot = f.ops_rotation + (size_t)b * max_ops;
        int badcode = 0;
        for (int base = 0; base < nops; base += CRYSTAL_THREADS) {
            const int m = base + tid;
            bool distinct = false;
            int code = -1;
            if (m < nops) {
                code = rot[m];
                int W[9];
                if (code < 0 || code >= SYM_CODES) badcode = 1;
                else {
                    const int det = decode_rotation(code, W);
                    if (det != 1 && det != -1) badcode = 1;
                    else distinct = m == 0 || rot[m - 1] != code;
                }
            }
            int total;
            const int rank = crystal_compact(distinct, lane, wave, s_slots, total);
            if (distinct && nrot + rank < CONV_MAX_ROT) s_code[nrot + rank] = code;
            nrot += total;
            __syncthreads();  // (s_slots is written again in the next round)
        }
        if (__syncthreads_or(badcode) || nrot > CONV_MAX_ROT) flags = ARREAU_CONV_NO_GROUP;
    }

    // ---- rules 2-5: one thread, integers; the transform, its adjugate, the centring translations
    if (tid == 0) {
        int P[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pts[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int det = 1, centring = CEN_P, bravais = -1, out_flags = flags;
        if (!flags) {
            const int family = pg < 2 ? 0 : (pg < 5 ? 1 : (pg < 8 ? 2 : (pg < 15 ? 3 : (pg < 27 ? 4 : 5))));
            bool ok = conventional_basis(s_code, nrot, family, Lm, P);
            if (ok) {
                centring = centring_of(P, det, pts);
                bravais = centring >= 0 ? bravais_of(family, centring) : -1;
                ok = bravais >= 0;
            }
            if (ok) {  // every rotation in the conventional basis, (P^T)^-1 W P^T = adj(P)^T W P^T / det, is an integer matrix
                iadj3(P, A);
                int At[9], Pt[9];
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) { At[3 * r + c] = A[3 * c + r]; Pt[3 * r + c] = P[3 * c + r]; }
                for (int m = 0; m < nrot && ok; ++m) {
                    int W[9], T1[9], T2[9];
                    decode_rotation(s_code[m], W);
                    imatmul(W, Pt, T1);
                    imatmul(At, T1, T2);
                    for (int p = 0; p < 9; ++p) ok &= T2[p] % det == 0;
                }
            }
            if (!ok) {
                out_flags = ARREAU_CONV_NO_BASIS;
                const int id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
                for (int p = 0; p < 9; ++p) { P[p] = id[p]; A[p] = id[p]; }
                for (int k = 0; k < 12; ++k) pts[k] = 0;
                det = 1; centring = CEN_P; bravais = -1;
            }
        }
        for (int p = 0; p < 9; ++p) { s_P[p] = P[p]; s_adj[p] = A[p]; }
        for (int k = 0; k < 12; ++k) s_pts[k] = pts[k];
        s_flags = out_flags;
        s_det = det;

        // ---- rule 6: the cell P L (a flagged crystal's own, bit for bit), its lengths and angles
        float cell[9];
        for (int r = 0; r < 3; ++r)
            for (int d = 0; d < 3; ++d)
                cell[3 * r + d] = out_flags ? Lm[3 * r + d] : rows_rn(Lm, d, (float)P[3 * r], (float)P[3 * r + 1], (float)P[3 * r + 2]);
        float len[3];
        for (int i = 0; i < 3; ++i) len[i] = sqrtf(dot3_rn(cell[3 * i], cell[3 * i + 1], cell[3 * i + 2], cell[3 * i], cell[3 * i + 1], cell[3 * i + 2]));
        for (int i = 0; i < 3; ++i) {  // angle i lies between the other two vectors
            const int j = (i + 1) % 3, k = (i + 2) % 3;
            const float c = __fdiv_rn(dot3_rn(cell[3 * j], cell[3 * j + 1], cell[3 * j + 2], cell[3 * k], cell[3 * k + 1], cell[3 * k + 2]),
                                      __fmul_rn(len[j], len[k]));
            o.lengths[3 * (size_t)b + i] = len[i];
            o.angles[3 * (size_t)b + i] = acosf(fminf(fmaxf(c, -1.f), 1.f));
        }
        for (int q = 0; q < 9; ++q) {
            o.lattice[9 * (size_t)b + q] = cell[q];
            o.transform[9 * (size_t)b + q] = P[q];
        }
        o.centring[b] = centring;
        o.bravais[b] = bravais;
        o.n_points[b] = det;
        o.num_atoms[b] = n * det;
        o.flags[b] = out_flags;
    }
    __syncthreads();
    flags = s_flags;

    // ---- rule 7: the atoms, at four times the input's offsets
    const size_t base = 4 * (size_t)first;
    const int det = s_det, total = n * det;
    if (!flags) {
        float A[9];
        for (int p = 0; p < 9; ++p) A[p] = (float)s_adj[p];
        const float fdet = (float)det;
        for (int idx = tid; idx < total; idx += CRYSTAL_THREADS) {
            const int k = idx / n, i = idx - k * n;
            const float* x = frac + 3 * ((size_t)first + i);
            const float w0 = crystal_wrap(x[0]), w1 = crystal_wrap(x[1]), w2 = crystal_wrap(x[2]);
            for (int c = 0; c < 3; ++c) {
                const float q = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w0, A[c]), __fmul_rn(w1, A[3 + c])), __fmul_rn(w2, A[6 + c])),
                                          (float)s_pts[3 * k + c]);
                o.frac_out[3 * (base + idx) + c] = crystal_wrap(__fdiv_rn(q, fdet));
            }
            o.types_out[base + idx] = types[(size_t)first + i];
            o.source[base + idx] = i;
        }
    } else {
        for (int a = tid; a < 3 * n; a += CRYSTAL_THREADS) o.frac_out[3 * base + a] = frac[3 * (size_t)first + a];
        for (int a = tid; a < n; a += CRYSTAL_THREADS) { o.types_out[base + a] = types[(size_t)first + a]; o.source[base + a] = a; }
    }
    for (int idx = total + tid; idx < 4 * n; idx += CRYSTAL_THREADS) {  // the unused slots
        o.frac_out[3 * (base + idx)] = 0.f; o.frac_out[3 * (base + idx) + 1] = 0.f; o.frac_out[3 * (base + idx) + 2] = 0.f;
        o.types_out[base + idx] = -1;
        o.source[base + idx] = -1;
    }
}

}  // namespace

extern "C" int arreau_crystal_conventional(const float* d_frac, const int32_t* d_types, const float* d_lattice,
                                           const int32_t* d_crystal_offsets, int32_t B, int32_t N, const arreau_symmetry_result* found,
                                           int32_t max_ops, arreau_conventional_result* out, void* stream) {
    ARREAU_REQUIRE(found != nullptr && out != nullptr, "arreau_crystal_conventional: null search result or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_conventional: bad size");
    ARREAU_REQUIRE(max_ops >= 1 && max_ops <= ARREAU_SYM_MAX_OPS_CAP, "arreau_crystal_conventional: max_ops must lie in 1..4096");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && ((d_frac && d_types) || N == 0), "arreau_crystal_conventional: null pointer");
    ARREAU_REQUIRE(found->n_ops && found->ops_rotation && found->point_group && found->flags,
                   "arreau_crystal_conventional: null array in the search result");
    ARREAU_REQUIRE(out->lattice && out->lengths && out->angles && out->transform && out->centring && out->bravais && out->n_points &&
                       out->num_atoms && out->flags,
                   "arreau_crystal_conventional: null result array");
    ARREAU_REQUIRE((out->frac_out && out->types_out && out->source) || N == 0, "arreau_crystal_conventional: null per-atom result array");
    conv_in f{found->n_ops, found->ops_rotation, found->point_group, found->flags};
    conv_out o{out->lattice, out->lengths, out->angles, out->transform, out->centring, out->bravais, out->n_points, out->num_atoms,
               out->flags, out->frac_out, out->types_out, out->source};
    ARREAU_LAUNCH(crystal_conventional_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_types, d_lattice,
                  d_crystal_offsets, (int)B, (int)N, (int)max_ops, f, o);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
