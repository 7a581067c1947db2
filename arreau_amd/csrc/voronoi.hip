// Voronoi cells of a batch of crystals (arreau_crystal_voronoi; the rules are written out in include/arreau_hip.h): per atom the
// faces of its Voronoi cell over every periodic image -- neighbour, solid angle, area, distance --, the weight of each face (its
// solid angle over the atom's largest), the number of faces of weight >= tol and the first max_faces of them in (j, m) order, the
// cell's volume and the certificate that it is closed; per crystal the sums and extremes.  The coordination search's image walk
// (coordination.hip) gathers the candidates; the cell is built from triples of bisecting planes, face by face.  One launch, one
// workgroup of four waves per crystal, one wave per atom, no atomics; needs no arreau_model.
//
// The planes are solved and tested in float64 (rule 2: the float32 displacements are taken as exact, so the cell is that of the
// numbers the kernel was given and no vertex is lost to rounding); the faces' fans, areas and solid angles are float32.
//
// LDS per workgroup: 50528 B (49.3 KiB) as the compiler reports it (group_segment_fixed_size), with 98 VGPRs and no scratch:
// three workgroups = 12 waves per CU (3 x 50528 = 151584 B of the CU's 163840 B; the compiler's occupancy line says 3 waves per
// SIMD; the plane test's slack PLANE_TOL cutoff |d_e| is one multiply in the loop, not a sixth array of doubles, which would
// leave room for two workgroups only).  What the bytes are:
//   spos                      3 * 256 floats                                     3072 B
//   per wave, x 4:            candidates x, y, z, h, |d| 5 * 128 doubles         5120 B
//                             candidate |d| as float, j, image m, order 4 * 128  2048 B
//                             face solid angle and area 2 * 128 floats           1024 B
//                             face vertices x, y, z, angle 4 * 128 floats        2048 B
//                             the same vertices in angular order 3 * 128 floats  1536 B     11776 B a wave, 47104 B
//   per-wave partial results  6 * 4 words                                          96 B     50272 B; the rest is alignment
// A wave talks to itself through its own slice alone, so the per-atom work needs no workgroup barrier: crystal_wave_sync() orders the
// wave's LDS writes before its reads.
#include "internal.h"
#include "crystal_dev.h"
#include <cmath>

namespace {

constexpr int VC = ARREAU_VORONOI_MAX_CANDIDATES;  // 128
constexpr int VF = ARREAU_VORONOI_FACE_VERTICES;   // 128

struct vor_wave {
    double cx[VC], cy[VC], cz[VC], ch[VC], cd[VC];  // d_e, h_e and |d_e|
    float cl[VC];                                           // |d_e| = sqrt(d2), the stored distance
    int cj[VC], cm[VC], ord[VC];
    float fo[VC], fa[VC];
    float vx[VF], vy[VF], vz[VF], va[VF];
    float sx[VF], sy[VF], sz[VF];
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(CRYSTAL_THREADS) void crystal_voronoi_kernel(
    const float* __restrict__ frac, const float* __restrict__ lattice, const int32_t* __restrict__ offsets, int B, int N, float tol,
    float r2 /* cutoff^2 */, float cutoff, int max_faces, int max_cand, int max_shells, arreau_voronoi_result out) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int first, n;
    float Lm[9];
    const bool bad = crystal_prologue(frac, lattice, offsets, b, N, first, n, Lm, [] {});

    __shared__ float spos[3 * CRYSTAL_LDS_ATOMS];
    __shared__ vor_wave s_wave[CRYSTAL_WAVES];
    __shared__ int s_faces[CRYSTAL_WAVES], s_lo[CRYSTAL_WAVES], s_hi[CRYSTAL_WAVES], s_flags[CRYSTAL_WAVES];
    __shared__ float s_eff[CRYSTAL_WAVES], s_vol[CRYSTAL_WAVES];

    const float qnan = __int_as_float(0x7fc00000);
    int4* const nb_rows = reinterpret_cast<int4*>(out.neighbors);
    auto blank_atom = [&](size_t A, int flags) {  // one thread: the per-atom scalars
        out.cn[A] = 0; out.atom_flags[A] = flags;
        out.volume[A] = qnan; out.omega_sum[A] = qnan; out.max_radius[A] = qnan; out.cn_eff[A] = qnan;
    };
    auto blank_slot = [&](size_t q) {
        nb_rows[q] = make_int4(-1, -1, -1, -1);
        out.face_weight[q] = qnan; out.face_solid_angle[q] = qnan; out.face_area[q] = qnan; out.face_distance[q] = qnan;
    };
    // NONFINITE / CELL (workgroup-uniform): nothing is computed, the reals are NaN, the lists -1, the counts 0
    auto blank = [&](int flags) {
        for (int a = tid; a < n; a += CRYSTAL_THREADS) blank_atom((size_t)first + a, 0);
        const size_t slots = (size_t)n * max_faces;
        for (size_t q = tid; q < slots; q += CRYSTAL_THREADS) blank_slot((size_t)first * max_faces + q);
        if (tid == 0) {
            out.n_faces[b] = 0; out.min_cn[b] = -1; out.max_cn[b] = -1;
            out.mean_cn[b] = qnan; out.mean_cn_eff[b] = qnan; out.volume_sum[b] = qnan; out.flags[b] = flags;
        }
    };
    if (bad) {
        blank(ARREAU_VORONOI_NONFINITE);
        return;
    }
    crystal_cell cell;
    if (crystal_cell_measure(Lm, cutoff, max_shells, cell)) {
        blank(ARREAU_VORONOI_CELL);
        return;
    }
    crystal_cell_images(cell);

    const crystal_positions position = crystal_stage_positions(spos, frac, Lm, first, n);
    const unsigned long long span = (unsigned long long)n * cell.M;
    const double ptol = (double)ARREAU_VORONOI_PLANE_TOL * (double)cutoff;  // the plane test's slack as a distance
    const float four_pi = 12.566370614359172f;
    vor_wave& W = s_wave[wave];

    int w_faces = 0, w_lo = 0x7fffffff, w_hi = -1, w_flags = 0;
    float w_eff = 0.f, w_vol = 0.f;
    for (int i = wave; i < n; i += CRYSTAL_WAVES) {
        const size_t A = (size_t)first + i;
        int4* const row = nb_rows + A * max_faces;
        const size_t frow = A * max_faces;
        const float pix = position(i, 0), piy = position(i, 1), piz = position(i, 2);
        crystal_wave_sync();  // (the slice is free: the previous atom's reads are done)

        // ---- rule 1: the candidates, every (j, m) but the atom itself with d2 <= r2, in ascending (j, m)
        int nc = 0, overlap = 0;
        crystal_walk_chunks(span, cell.M, (unsigned)lane, 64u, [&](bool valid, unsigned j, unsigned m) {
            bool hit = false;
            crystal_contact k{};
            if (valid && !(j == (unsigned)i && m == cell.centre)) {
                k = crystal_contact_at(cell, Lm, position, (int)j, m, pix, piy, piz);
                hit = k.d2 <= r2;
            }
            const unsigned long long hits = __ballot(hit);
            const int slot = nc + __popcll(hits & ((1ull << lane) - 1ull));
            if (hit && slot < max_cand) {  // (max_cand <= VC: inside the slice)
                const double x = (double)k.dx, y = (double)k.dy, z = (double)k.dz, h2 = (x * x + y * y) + z * z, len = sqrt(h2);
                W.cx[slot] = x; W.cy[slot] = y; W.cz[slot] = z;
                W.ch[slot] = 0.5 * h2; W.cd[slot] = len; W.cl[slot] = sqrtf(k.d2);
                W.cj[slot] = (int)j; W.cm[slot] = (int)m;
            }
            nc += __popcll(hits);
            overlap |= __ballot(hit && k.d2 == 0.f) != 0ull;
        });
        nc = __builtin_amdgcn_readfirstlane(nc);
        int aflags = overlap ? ARREAU_VORONOI_OVERLAP : 0;
        const int K = min(nc, max_cand);
        crystal_wave_sync();

        // ---- the order the planes are tested in: ascending distance (the answer of an AND does not depend on it; a far vertex
        // is thrown out by a near plane early)
        for (int k = lane; k < K; k += 64) {
            const double key = W.ch[k];
            int r = 0;
            for (int q = 0; q < K; ++q) {
                const double hq = W.ch[q];
                r += (hq < key || (hq == key && q < k)) ? 1 : 0;
            }
            W.ord[r] = k;
        }
        crystal_wave_sync();

        // ---- rules 2 and 3: face by face, the vertices on it from pairs of other planes
        float maxr2 = 0.f;
        bool vover = false;
        unsigned long long face_lo = 0ull, face_hi = 0ull;
        for (int a = 0; a < K && nc <= max_cand && !overlap; ++a) {
            const double ax = W.cx[a], ay = W.cy[a], az = W.cz[a], ha = W.ch[a], la = W.cd[a];
            int nv = 0;
            for (int bb = 0; bb < K; ++bb) {
                if (bb == a) continue;
                const double bx = W.cx[bb], by = W.cy[bb], bz = W.cz[bb], hb = W.ch[bb], lb = W.cd[bb];
                const double abx = ay * bz - az * by, aby = az * bx - ax * bz, abz = ax * by - ay * bx;
                for (int c0 = bb + 1; c0 < K; c0 += 64) {
                    const int c = c0 + lane;
                    bool ok = c < K && c != a;
                    double vx = 0., vy = 0., vz = 0.;
                    if (ok) {
                        const double cx = W.cx[c], cy = W.cy[c], cz = W.cz[c], hc = W.ch[c], lc = W.cd[c];
                        const double det = abx * cx + aby * cy + abz * cz;
                        ok = det != 0. && !(fabs(det) < (double)ARREAU_VORONOI_DET_TOL * (la * lb * lc));
                        if (ok) {
                            const double bcx = by * cz - bz * cy, bcy = bz * cx - bx * cz, bcz = bx * cy - by * cx;
                            const double cax = cy * az - cz * ay, cay = cz * ax - cx * az, caz = cx * ay - cy * ax;
                            const double inv = 1.0 / det;
                            vx = (ha * bcx + hb * cax + hc * abx) * inv;
                            vy = (ha * bcy + hb * cay + hc * aby) * inv;
                            vz = (ha * bcz + hb * caz + hc * abz) * inv;
                        }
                    }
                    if (__ballot(ok) != 0ull) {
                        for (int q = 0; q < K; ++q) {
                            const int e = W.ord[q];
                            const double s = (W.cx[e] * vx + W.cy[e] * vy + W.cz[e] * vz) - W.ch[e];
                            if (e != a && e != bb && e != c) ok = ok && (s <= ptol * W.cd[e]);
                            if (__ballot(ok) == 0ull) break;
                        }
                    }
                    const unsigned long long hits = __ballot(ok);
                    const int slot = nv + __popcll(hits & ((1ull << lane) - 1ull));
                    if (ok && slot < VF) {  // (the vertex leaves float64 here: the fan is float32)
                        const float fx = (float)vx, fy = (float)vy, fz = (float)vz;
                        W.vx[slot] = fx; W.vy[slot] = fy; W.vz[slot] = fz;
                        maxr2 = fmaxf(maxr2, fx * fx + fy * fy + fz * fz);
                    }
                    nv += __popcll(hits);
                }
            }
            nv = __builtin_amdgcn_readfirstlane(nv);
            float omega = 0.f, area = 0.f;
            if (nv > VF) vover = true;
            if (nv >= 3 && nv <= VF) {
                crystal_wave_sync();
                // the centroid, the in-plane axes (u1, u2, n right-handed) and each vertex's angle about the normal
                float px = 0.f, py = 0.f, pz = 0.f;
                for (int k = lane; k < nv; k += 64) { px += W.vx[k]; py += W.vy[k]; pz += W.vz[k]; }
                const float inv_nv = 1.0f / (float)nv;
                const float gx = crystal_wave_sum(px) * inv_nv, gy = crystal_wave_sum(py) * inv_nv, gz = crystal_wave_sum(pz) * inv_nv;
                const float il = 1.0f / W.cl[a], nx = (float)ax * il, ny = (float)ay * il, nz = (float)az * il;
                float tx = 0.f, ty = 0.f, tz = 0.f;  // the axis the normal leans on least
                if (fabsf(nx) <= fabsf(ny) && fabsf(nx) <= fabsf(nz)) tx = 1.f; else if (fabsf(ny) <= fabsf(nz)) ty = 1.f; else tz = 1.f;
                float u1x = ny * tz - nz * ty, u1y = nz * tx - nx * tz, u1z = nx * ty - ny * tx;
                const float iu = 1.0f / sqrtf(u1x * u1x + u1y * u1y + u1z * u1z);
                u1x *= iu; u1y *= iu; u1z *= iu;
                const float u2x = ny * u1z - nz * u1y, u2y = nz * u1x - nx * u1z, u2z = nx * u1y - ny * u1x;
                for (int k = lane; k < nv; k += 64) {
                    const float rx = W.vx[k] - gx, ry = W.vy[k] - gy, rz = W.vz[k] - gz;
                    W.va[k] = atan2f(rx * u2x + ry * u2y + rz * u2z, rx * u1x + ry * u1y + rz * u1z);
                }
                crystal_wave_sync();
                for (int k = lane; k < nv; k += 64) {  // a rank sort: ties (copies of a degenerate vertex) in hit order
                    const float key = W.va[k];
                    int r = 0;
                    for (int q = 0; q < nv; ++q) {
                        const float aq = W.va[q];
                        r += (aq < key || (aq == key && q < k)) ? 1 : 0;
                    }
                    W.sx[r] = W.vx[k]; W.sy[r] = W.vy[k]; W.sz[r] = W.vz[k];
                }
                crystal_wave_sync();
                // the fan about the centroid: triangle k = (g, w_k, w_k+1), cyclic
                const float gl = sqrtf(gx * gx + gy * gy + gz * gz);
                float l_area = 0.f, l_omega = 0.f;
                for (int k = lane; k < nv; k += 64) {
                    const int k1 = k + 1 == nv ? 0 : k + 1;
                    const float p0 = W.sx[k], p1 = W.sy[k], p2 = W.sz[k], q0 = W.sx[k1], q1 = W.sy[k1], q2 = W.sz[k1];
                    const float e0 = p0 - gx, e1 = p1 - gy, e2 = p2 - gz, f0 = q0 - gx, f1 = q1 - gy, f2 = q2 - gz;
                    l_area += 0.5f * (nx * (e1 * f2 - e2 * f1) + ny * (e2 * f0 - e0 * f2) + nz * (e0 * f1 - e1 * f0));
                    const float pl = sqrtf(p0 * p0 + p1 * p1 + p2 * p2), ql = sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
                    const float num = gx * (p1 * q2 - p2 * q1) + gy * (p2 * q0 - p0 * q2) + gz * (p0 * q1 - p1 * q0);
                    const float den = gl * pl * ql + (gx * p0 + gy * p1 + gz * p2) * ql + (gx * q0 + gy * q1 + gz * q2) * pl +
                                      (p0 * q0 + p1 * q1 + p2 * q2) * gl;
                    l_omega += 2.0f * atan2f(num, den);
                }
                area = crystal_wave_sum(l_area);
                omega = crystal_wave_sum(l_omega);
                if (a < 64) face_lo |= 1ull << a; else face_hi |= 1ull << (a - 64);
            }
            if (lane == 0) { W.fo[a] = omega; W.fa[a] = area; }
            crystal_wave_sync();
        }

        // ---- rules 4 and 5: weights, the stored faces, the sums, the certificate
        if (nc > max_cand || vover || overlap) {  // OVERFLOW: too many candidates, or a face with too many vertex copies; OVERLAP: no cell
            if (nc > max_cand || vover) aflags |= ARREAU_VORONOI_OVERFLOW;
            if (lane == 0) blank_atom(A, aflags);
            if (lane < max_faces) blank_slot(frow + lane);
            w_lo = min(w_lo, 0); w_hi = max(w_hi, 0);
            w_flags |= aflags;
            w_eff += qnan; w_vol += qnan;
            continue;
        }
        const int k0 = lane, k1 = lane + 64;
        const bool is0 = k0 < K && ((face_lo >> lane) & 1ull), is1 = k1 < K && ((face_hi >> lane) & 1ull);
        const float o0 = is0 ? W.fo[k0] : 0.f, o1 = is1 ? W.fo[k1] : 0.f;
        const float maxo = wave_max(fmaxf(is0 ? o0 : 0.f, is1 ? o1 : 0.f));
        // (a zero-area face's solid angle is rounding noise of either sign: it weighs 0; no face above 0: every weight is 0)
        const float wt0 = is0 && maxo > 0.f ? fmaxf(o0, 0.f) / maxo : 0.f, wt1 = is1 && maxo > 0.f ? fmaxf(o1, 0.f) / maxo : 0.f;
        const float ar0 = is0 ? W.fa[k0] : 0.f, ar1 = is1 ? W.fa[k1] : 0.f;
        const float ds0 = is0 ? W.cl[k0] : 0.f, ds1 = is1 ? W.cl[k1] : 0.f;
        int cn = 0;
        auto store = [&](bool sel, int k, float wt, float om, float ar, float ds) {
            const unsigned long long hits = __ballot(sel);
            const int slot = cn + __popcll(hits & ((1ull << lane) - 1ull));
            if (sel && slot < max_faces) {
                int im[3];
                crystal_image(cell, (unsigned)W.cm[k], im);
                row[slot] = make_int4(W.cj[k], im[0], im[1], im[2]);
                out.face_weight[frow + slot] = wt; out.face_solid_angle[frow + slot] = om;
                out.face_area[frow + slot] = ar; out.face_distance[frow + slot] = ds;
            }
            cn += __popcll(hits);
        };
        store(is0 && wt0 >= tol, k0, wt0, o0, ar0, ds0);
        store(is1 && wt1 >= tol, k1, wt1, o1, ar1, ds1);
        cn = __builtin_amdgcn_readfirstlane(cn);
        if (lane >= min(cn, max_faces) && lane < max_faces) blank_slot(frow + lane);  // (max_faces <= 64: one lane per slot)
        const float cn_eff = crystal_wave_sum(wt0 + wt1);
        const float omega_sum = crystal_wave_sum(o0 + o1);
        const float volume = crystal_wave_sum(ar0 * ds0 * (1.0f / 6.0f) + ar1 * ds1 * (1.0f / 6.0f));
        const float max_radius = sqrtf(wave_max(maxr2));
        if (2.0f * max_radius > cutoff || !(fabsf(omega_sum - four_pi) <= ARREAU_VORONOI_CLOSURE_TOL)) aflags |= ARREAU_VORONOI_OPEN;
        if (cn > max_faces) aflags |= ARREAU_VORONOI_TRUNCATED;
        if (lane == 0) {
            out.cn[A] = cn; out.atom_flags[A] = aflags;
            out.volume[A] = volume; out.omega_sum[A] = omega_sum; out.max_radius[A] = max_radius; out.cn_eff[A] = cn_eff;
        }
        w_faces += cn;
        w_lo = min(w_lo, cn); w_hi = max(w_hi, cn);
        w_flags |= aflags;
        w_eff += cn_eff; w_vol += volume;
    }

    // ---- rule 6, per crystal: the four waves' partial results through LDS, the reals summed in wave order
    if (lane == 0) {
        s_faces[wave] = w_faces; s_lo[wave] = w_lo; s_hi[wave] = w_hi; s_flags[wave] = w_flags; s_eff[wave] = w_eff; s_vol[wave] = w_vol;
    }
    __syncthreads();
    if (tid == 0) {
        int faces = 0, lo = 0x7fffffff, hi = -1, flags = n == 0 ? ARREAU_VORONOI_EMPTY : 0;
        float eff = 0.f, vol = 0.f;
        for (int w = 0; w < CRYSTAL_WAVES; ++w) {
            faces += s_faces[w];
            lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]);
            flags |= s_flags[w];
            eff += s_eff[w]; vol += s_vol[w];
        }
        out.n_faces[b] = faces;
        out.min_cn[b] = n == 0 ? -1 : lo; out.max_cn[b] = hi;
        out.mean_cn[b] = n == 0 ? qnan : (float)faces / (float)n;
        out.mean_cn_eff[b] = n == 0 ? qnan : eff / (float)n;
        out.volume_sum[b] = n == 0 ? qnan : vol;
        out.flags[b] = flags;
    }
}

}  // namespace

extern "C" int arreau_crystal_voronoi(const float* d_frac, const float* d_lattice, const int32_t* d_crystal_offsets, int32_t B, int32_t N,
                                      const arreau_voronoi_params* params, arreau_voronoi_result* out, void* stream) {
    ARREAU_REQUIRE(params != nullptr && out != nullptr, "arreau_crystal_voronoi: null params or result");
    ARREAU_REQUIRE(B >= 0 && N >= 0, "arreau_crystal_voronoi: bad size");
    ARREAU_REQUIRE(std::isfinite(params->tol) && params->tol >= 0.f && params->tol <= 1.f, "arreau_crystal_voronoi: tol must lie in [0, 1]");
    ARREAU_REQUIRE(std::isfinite(params->cutoff) && params->cutoff > 0.f, "arreau_crystal_voronoi: cutoff must be finite and > 0");
    ARREAU_REQUIRE(params->max_faces >= 1 && params->max_faces <= ARREAU_VORONOI_MAX_FACES, "arreau_crystal_voronoi: max_faces must lie in 1..64");
    ARREAU_REQUIRE(params->max_candidates >= 1 && params->max_candidates <= ARREAU_VORONOI_MAX_CANDIDATES,
                   "arreau_crystal_voronoi: max_candidates must lie in 1..128");
    ARREAU_REQUIRE(params->max_shells >= 1 && params->max_shells <= ARREAU_SCREEN_MAX_SHELLS, "arreau_crystal_voronoi: max_shells must lie in 1..8");
    if (B == 0) return ARREAU_OK;
    ARREAU_REQUIRE(d_lattice && d_crystal_offsets && (d_frac || N == 0), "arreau_crystal_voronoi: null pointer");
    ARREAU_REQUIRE(out->n_faces && out->min_cn && out->max_cn && out->mean_cn && out->mean_cn_eff && out->volume_sum && out->flags,
                   "arreau_crystal_voronoi: null per-crystal result array");
    ARREAU_REQUIRE(N == 0 || (out->cn && out->neighbors && out->face_weight && out->face_solid_angle && out->face_area && out->face_distance &&
                              out->volume && out->omega_sum && out->max_radius && out->cn_eff && out->atom_flags),
                   "arreau_crystal_voronoi: null per-atom result array");
    ARREAU_REQUIRE((reinterpret_cast<uintptr_t>(out->neighbors) & 15u) == 0, "arreau_crystal_voronoi: neighbors must be 16-byte aligned");
    const float r2 = (float)((double)params->cutoff * (double)params->cutoff);
    ARREAU_LAUNCH(crystal_voronoi_kernel, dim3((unsigned)B), dim3(CRYSTAL_THREADS), 0, (hipStream_t)stream, d_frac, d_lattice, d_crystal_offsets,
                  (int)B, (int)N, params->tol, r2, params->cutoff, (int)params->max_faces, (int)params->max_candidates, (int)params->max_shells, *out);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
