// Training-mode score network (BASELINE config 5): forward with saved activations and the backward pass, fp32.
//
// The sampling kernels (edge_f16.hip, node*.hip) keep nothing: activations live in registers and only K_l reaches HBM.
// A training step needs every layer's inputs again, so this file evaluates the same network in the textbook form --
// one dense product per Linear (sgemm_kernel below, exact fp32 on the matrix pipe, split-K for the weight gradients), small elementwise /
// gather / reduce kernels between them, every intermediate in HBM -- and walks it backwards.  At config-5 sizes (64
// crystals, about 540 atoms, 69 k (edge, orientation) rows per GPU) the whole step moves a few hundred MB; clarity
// and exact fp32 arithmetic matter more here than the last factor of two.  Measured on MI355X (profiles/r02i_*): 9.6 ms
// forward + backward for 64 crystals / 532 atoms (first version with FMA GEMMs and single-workgroup column sums: 38 ms).
//
// Reference: PonitaFiberBundle.forward (ponita/models/ponita.py:88-123), FiberBundleConv.forward / message
// (ponita/nn/conv.py:105-138; PyG sum aggregation onto edge_index[1]), ConvNext.forward (ponita/nn/convnext.py:20-33),
// the read-outs (ponita.py:126-155); the backward is what autograd derives from those (training_step,
// lightning_wrappers/diffusion.py:108-118).  Gradients are returned in the state_dict layout (arreau_state_dict with
// DEVICE pointers; non-trainable entries are ignored).
//
// The kernels are in train_kernels.h; this file holds the context, the launch helpers and the entry points.
#include <string.h>
#include <algorithm>
#include <vector>

#include "internal.h"
#include "edge_rows.h"
#include "sgemm.h"
#include "train_kernels.h"

// ---------------------------------------------------------------------------------------------
// context: buffers of one training step, owned by the model, grown on demand
// ---------------------------------------------------------------------------------------------
struct arreau_train_ctx {
    int N = 0, B = 0, capN = 0, capB = 0;
    // arithmetic of the dense products (sgemm.h): 0 exact fp32 MFMA, 1 fp16x3, 2 bf16x6.  The training step runs its forward
    // products on fp16x3 (activations x weights: the sampling kernels' arithmetic) and every product with a gradient operand
    // on bf16x6 (full exponent range); the shape-general SAMPLING path stays on the exact kernel (it is the arithmetic
    // cross-check of the fused kernels).  ARREAU_TRAIN_GEMM=exact|split|fp16 (default split).
    int fwd_mode = 0, bwd_mode = 0;
    // Launch merges of the training step (round 5): ARREAU_TRAIN_FUSE, read by train_fuse_on() once at the head of every entry point --
    // per call, not per process: A/B runs and tests change the environment between calls.
    bool fuse = true;
    float* buf = nullptr;
    size_t buf_floats = 0;
    // plain row-major weights (in the model blob): [C][96], [D][C], [L][C][D], [L][H][C], [L][C][H], [L][S+4][C]
    const float *w1f, *w2, *wk, *lin1, *lin2, *ro_w;
    // forward state
    int32_t *batch, *deg, *src, *cell, *rev_start, *rev_cnt, *rev_idx, *mono_cols;
    float *lattice, *cart, *cvec, *dir, *dist;
    float *mono, *window, *h1pre, *h1, *h2pre, *kb, *fpoly, *fh1pre, *fh1, *fh2pre, *fkb, *F;
    float *x, *x1, *xhat, *rstd, *hpre, *h, *out, *fk, *rbar, *gs, *kern;
    // backward temporaries
    float *dx, *dxro, *rbar_all, *dfkb_all, *dtmp, *dh, *drbar, *dx1, *dkern, *dkb, *dh1, *dfkb, *dfh1, *dw1f, *partial, *scratch_cols, *colpart;
    float* robias;  // [ROP] the one column sum of d(rbar) (every layer's read-out bias gradient)
    float *dxn_all, *dx2_all;  // [L][M][C]: d(LayerNorm output) and d(spherical conv output), for the batched bias / norm gradients
    float *xn_all, *dout_all, *dfk_all;  // [L][...]: LayerNorm outputs (forward), d(out) and d(fiber kernel) (backward), for the batched weight gradients
    double* std_part;  // [2][STD_PARTS] partial sums of arreau_train_conv_stats
    // The fiber branch (fiber basis MLP -> fiber kernels forward; their gradients backward) depends on the weights alone: a couple of
    // dozen launches over 256 rows, 4-6 us each on a handful of CUs.  They run on a second stream beside the edge-level products
    // (fork / join by events; ARREAU_TRAIN_SIDE_STREAM=0 keeps them in line) with their own split-K and column-sum scratch.
    // Measured (64 crystals, alternating on one box, 3 x 60 steps): 2.130 -> 2.108 ms per step -- 1 %, not the 0.19 ms the branch takes
    // in line: launches that share the chip slow each other (a 32-workgroup side launch beside a product of 1,024 workgroups, two per
    // CU, cost that product a third of a round: 30 -> 39 us in the kernel trace).
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_rev = nullptr;   // the reversed adjacency of the forward pass is complete (side stream; the backward pass waits for it)
    bool rev_pending = false;
    float *partial2 = nullptr, *colpart2 = nullptr;
    // Round 5: deferred reductions of the backward pass (main stream only): the k-slice sums of the weight-gradient products and the
    // chunk sums of the column-sum passes, each ONE launch at the end of arreau_train_backward (sgemm.h: arreau_sgemm_defer;
    // colsum4_final_multi_kernel).  Shared by the side stream's copy of this struct (pointers), never used through it.
    struct Deferred {
        arreau_sgemm_defer gemm;
        ColsumFinalList cols{};
        int ncols = 0, max_colblocks = 0;
        float* colscratch = nullptr;
        size_t colcap = 0, colused = 0;  // floats
    };
    Deferred* defer = nullptr;
};

namespace {
struct Carve {
    float* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t n) {
        off = (off + 63) & ~(size_t)63;
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (n * sizeof(T) + 3) / 4;
        return r;
    }
};
constexpr size_t PARTIAL_FLOATS = ARREAU_SGEMM_PARTIAL_FLOATS;

size_t layout(arreau_train_ctx& t, const arreau_model* m, int N, int B, float* base) {
    Carve c{base};
    const size_t C = m->C, D = m->D, L = m->L, H = m->H, k = m->k, S = m->S, RO = S + 4;
    const size_t R = (size_t)N * k * 16, M = (size_t)N * 16;
    t.w1f = m->t_w1f; t.w2 = m->t_w2; t.wk = m->t_wk; t.lin1 = m->t_lin1; t.lin2 = m->t_lin2; t.ro_w = m->t_ro_w;
    t.batch = c.take<int32_t>(N); t.deg = c.take<int32_t>(N); t.src = c.take<int32_t>(N * k); t.cell = c.take<int32_t>(N * k);
    t.rev_start = c.take<int32_t>(N); t.rev_cnt = c.take<int32_t>(N); t.rev_idx = c.take<int32_t>(N * k);
    t.mono_cols = c.take<int32_t>(ARREAU_MONO_PAD * 8);
    t.lattice = c.take<float>(B * 9); t.cart = c.take<float>(N * 3); t.cvec = c.take<float>(B * C);
    t.dir = c.take<float>(N * k * 3); t.dist = c.take<float>(N * k);
    t.mono = c.take<float>(R * ARREAU_MONO_PAD); t.window = c.take<float>(R);
    t.h1pre = c.take<float>(R * C); t.h1 = c.take<float>(R * C); t.h2pre = c.take<float>(R * D); t.kb = c.take<float>(R * D);
    t.fpoly = c.take<float>(256 * 3); t.fh1pre = c.take<float>(256 * C); t.fh1 = c.take<float>(256 * C);
    t.fh2pre = c.take<float>(256 * D); t.fkb = c.take<float>(256 * D); t.F = c.take<float>(M * (S + 78));
    t.x = c.take<float>((L + 1) * M * C); t.x1 = c.take<float>(L * M * C); t.xhat = c.take<float>(L * M * C);
    t.rstd = c.take<float>(L * M); t.hpre = c.take<float>(L * M * H); t.h = c.take<float>(L * M * H);
    t.out = c.take<float>(L * M * C); t.fk = c.take<float>(L * 256 * C); t.rbar = c.take<float>(M * RO); t.rbar_all = c.take<float>(L * M * RO); t.gs = c.take<float>(N * 3);
    t.kern = c.take<float>(R * L * C);   // all layers' spatial kernels, [R][L*C] (one GEMM: the basis is layer-independent)
    t.dx = c.take<float>(L * M * C);   // d x_l of every layer (round 5: kept per layer for the batched layer-scale / linear_2.bias column sums)
    t.dxro = c.take<float>(L * M * C); t.dtmp = c.take<float>(M * C); t.dh = c.take<float>(L * M * H); t.drbar = c.take<float>(M * ((RO + 3) & ~(size_t)3));
    t.xn_all = c.take<float>(L * M * C); t.dout_all = c.take<float>(L * M * C); t.dfk_all = c.take<float>(L * 256 * C);
    t.dxn_all = c.take<float>(L * M * C); t.dx2_all = c.take<float>(L * M * C);  // kept per layer for the batched weight gradients
    t.dx1 = c.take<float>(M * C); t.dkern = c.take<float>(R * L * C); t.dkb = c.take<float>(R * D); t.dh1 = c.take<float>(R * C);
    t.dfkb = c.take<float>(256 * D); t.dfkb_all = c.take<float>(L * 256 * D); t.dfh1 = c.take<float>(256 * C);
    t.dw1f = c.take<float>(C * ARREAU_MONO_PAD); t.partial = c.take<float>(PARTIAL_FLOATS); t.scratch_cols = c.take<float>(1024); t.robias = c.take<float>(1024);
    t.colpart = c.take<float>((size_t)2 * COLSUM4_MAX_BATCH * COLSUM4_MAX_CHUNKS * 1024);  // (two results per pass, up to eight matrices per call)
    t.std_part = c.take<double>(2 * STD_PARTS);
    t.partial2 = c.take<float>(PARTIAL_FLOATS);
    t.colpart2 = c.take<float>((size_t)2 * COLSUM4_MAX_BATCH * COLSUM4_MAX_CHUNKS * 1024);
    {   // deferred reductions: room for every weight gradient's k-slices at once (each product is capped at PARTIAL_FLOATS) and for
        // the chunk rows of every column-sum pass of a backward pass; a request that does not fit runs its reduction at once
        float* gs = c.take<float>(3 * PARTIAL_FLOATS);
        const size_t colcap = (size_t)2 * COLSUM4_MAX_BATCH * COLSUM4_MAX_CHUNKS * 1024;
        float* cs = c.take<float>(colcap);
        if (t.defer) {
            t.defer->gemm.scratch = gs; t.defer->gemm.cap = 3 * PARTIAL_FLOATS;
            t.defer->colscratch = cs; t.defer->colcap = colcap;
        }
    }
    return c.off;
}

// Round 5: launch merges of the training step (conv + mix forward, LayerNorm + mix backward, both conv gradients in one launch,
// column-sum and split-K reductions deferred to one launch each at the end of the backward pass).  ARREAU_TRAIN_FUSE=0 restores the
// one-kernel-per-operation sequence (same arithmetic per element: tests compare the two bit for bit).  The entry points store the
// answer in arreau_train_ctx::fuse; everything below them reads the field.
inline bool train_fuse_on() {
    const char* e = getenv("ARREAU_TRAIN_FUSE");
    return !e || atoi(e) != 0;
}
typedef arreau_sgemm_detail::SgemmEpilogue Epi;
int gemm(hipStream_t s, arreau_train_ctx& t, int mode, int M, int N, int K, const float* A, long as0, long as1, const float* B, long bs0,
         long bs1, float* C, int ldc, float alpha = 1.f, float beta = 0.f, const Epi* epi = nullptr, bool* fused = nullptr) {
    return arreau_sgemm(s, t.partial, M, N, K, A, as0, as1, B, bs0, bs1, C, ldc, alpha, beta, 1, 0, 0, 0, mode, epi, fused);
}
// Y[rows][out] = X[rows][in] . W[out][in]^T
int linear(hipStream_t s, arreau_train_ctx& t, long rows, int in, int out, const float* X, const float* W, float* Y,
           float alpha = 1.f, float beta = 0.f, const Epi* epi = nullptr, bool* fused = nullptr) {
    return gemm(s, t, t.fwd_mode, (int)rows, out, in, X, in, 1, W, 1, in, Y, out, alpha, beta, epi, fused);
}
// dX[rows][in] (+)= dY[rows][out] . W[out][in]
int linear_dx(hipStream_t s, arreau_train_ctx& t, long rows, int in, int out, const float* dY, const float* W, float* dX,
              float alpha = 1.f, float beta = 0.f, const Epi* epi = nullptr, bool* fused = nullptr) {
    return gemm(s, t, t.bwd_mode, (int)rows, in, out, dY, out, 1, W, in, 1, dX, in, alpha, beta, epi, fused);
}
// the same for `batch` layers in one launch (dY / X / dW of consecutive layers dy_bs / x_bs / out * in floats apart; 0 = shared)
int linear_dw_batched(hipStream_t s, arreau_train_ctx& t, int batch, long rows, int in, int out, const float* dY, long dy_bs,
                      const float* X, long x_bs, float* dW, float alpha = 1.f, bool defer = false, int dy_ld = 0 /* row pitch of dY (0: out) */) {
    return arreau_sgemm(s, t.partial, out, in, (int)rows, dY, 1, dy_ld ? dy_ld : out, X, in, 1, dW, in, alpha, 0.f, batch, dy_bs, x_bs, (long)out * in, t.bwd_mode,
                        nullptr, nullptr, defer && t.fuse && t.defer ? &t.defer->gemm : nullptr);
}
// dW[out][in] = alpha * dY[rows][out]^T . X[rows][in]
int linear_dw(hipStream_t s, arreau_train_ctx& t, long rows, int in, int out, const float* dY, const float* X, float* dW,
              float alpha = 1.f, bool defer = false) {
    return linear_dw_batched(s, t, 1, rows, in, out, dY, 0, X, 0, dW, alpha, defer);
}
// Column sums (colsum4_*_kernel): out[c] = scale * sum_r a[r][c] * (b ? b[r][c] : 1)  (+ out[c] if accumulate).
struct ColsumArgs {
    const float* a = nullptr;
    const float* b = nullptr;
    long rows = 0;
    int cols = 0;
    float scale = 1.0f;
    float* out = nullptr;
    int accumulate = 0;
    float* out2 = nullptr;            // also out2[c] = (colscale2 ? colscale2[c] : 1) * sum_r a[r][c]  (needs b)
    const float* colscale2 = nullptr;
    // `batch` > 1: the same sums for `batch` matrices (a / b a_bs / b_bs floats apart, results out_bs / out2_bs apart, colscale2 colscale2_bs
    // apart) in the two launches of one -- the bias gradients of the L layers
    int batch = 1;
    long a_bs = 0, b_bs = 0, out_bs = 0, out2_bs = 0, colscale2_bs = 0;
    float* scaled_out = nullptr;      // one matrix, no gelu_pre: also scaled_out = a * colscale_out, written by the same pass
    const float* colscale_out = nullptr;
    bool defer = false;               // the sums may wait for flush_deferred_colsums (main stream of the backward pass only)
    const float* gelu_pre = nullptr;  // one matrix: a *= gelu'(gelu_pre) * gelu_rowscale[row] in place first
    const float* gelu_rowscale = nullptr;
    ColsumGather* gather = nullptr;   // deferred passes over the same rows: collected here, launched together by launch_gathered
};
int colsum(hipStream_t s, arreau_train_ctx& t, const ColsumArgs& p) {
    const float *a = p.a, *b = p.b;
    const long rows = p.rows;
    const int cols = p.cols, batch = p.batch;
    if (cols > 1024) {
        arreau_set_error("colsum: more than 1024 columns");
        return ARREAU_EINVAL;
    }
    if (!(cols % 4 == 0 && (size_t)a % 16 == 0 && (b == nullptr || (size_t)b % 16 == 0) && p.a_bs % 4 == 0 && p.b_bs % 4 == 0)) {
        arreau_set_error("colsum: columns and operands must be 16-byte aligned");
        return ARREAU_EINVAL;
    }
    if (batch > COLSUM4_MAX_BATCH) {
        arreau_set_error("colsum: batch beyond the partial-sum scratch");
        return ARREAU_EINVAL;
    }
    if (p.out2 && !b) {
        arreau_set_error("colsum: a second result needs a second operand");
        return ARREAU_EINVAL;
    }
    if (p.gelu_pre && !(batch == 1 && (size_t)p.gelu_pre % 16 == 0)) {
        arreau_set_error("colsum: the GELU-backward form needs one matrix and 16-byte columns");
        return ARREAU_EINVAL;
    }
    const int chunks = (int)std::min<long>(COLSUM4_MAX_CHUNKS, std::max<long>(1, rows / 16));
    const long rpc = (rows + chunks - 1) / chunks;
    const bool dual = p.out2 != nullptr;
    f32x4* part = reinterpret_cast<f32x4*>(t.colpart);
    f32x4* part2 = dual ? part + (size_t)COLSUM4_MAX_BATCH * COLSUM4_MAX_CHUNKS * 256 : nullptr;
    const size_t need = (size_t)batch * chunks * cols * (dual ? 2 : 1);  // floats
    arreau_train_ctx::Deferred* df = p.defer && t.fuse ? t.defer : nullptr;
    const bool deferred = df && df->colscratch && df->colused + need <= df->colcap && df->ncols + batch <= COLSUM_DEFER_MAX;
    if (deferred) {
        part = reinterpret_cast<f32x4*>(df->colscratch + df->colused);
        part2 = dual ? part + (size_t)batch * chunks * (cols / 4) : nullptr;
        df->colused += (need + 63) & ~(size_t)63;
        for (int i = 0; i < batch; ++i) {
            ColsumFinalDesc& d = df->cols.d[df->ncols++];
            d.part = part + (size_t)i * chunks * (cols / 4);
            d.part2 = dual ? part2 + (size_t)i * chunks * (cols / 4) : nullptr;
            d.out = p.out + (long)i * p.out_bs;
            d.out2 = dual ? p.out2 + (long)i * p.out2_bs : nullptr;
            d.colscale2 = p.colscale2 ? p.colscale2 + (long)i * p.colscale2_bs : nullptr;
            d.chunks = chunks; d.cols4 = cols / 4; d.scale = p.scale; d.accumulate = p.accumulate;
        }
        df->max_colblocks = std::max(df->max_colblocks, (cols / 4 + 7) / 8);
    }
    ColsumGather* gather = p.gather;
    if (deferred && gather && !p.gelu_pre && !p.scaled_out && gather->n + batch <= COLSUM_PARTIAL_MULTI_MAX &&
        (gather->n == 0 || (gather->rows == rows && gather->chunks == chunks))) {
        gather->rows = rows; gather->chunks = chunks; gather->rpc = rpc;
        for (int i = 0; i < batch; ++i) {
            ColsumPartialDesc& d = gather->list.d[gather->n++];
            d.a = reinterpret_cast<const f32x4*>(a) + (long)i * (p.a_bs / 4);
            d.b = b ? reinterpret_cast<const f32x4*>(b) + (long)i * (p.b_bs / 4) : nullptr;
            d.part = part + (size_t)i * chunks * (cols / 4);
            d.part2 = part2 ? part2 + (size_t)i * chunks * (cols / 4) : nullptr;
            d.cols4 = cols / 4;
        }
        return ARREAU_OK;
    }
    if (p.gelu_pre)
        hipLaunchKernelGGL(colsum4_partial_kernel<true>, dim3(chunks, batch), dim3(256), 0, s, reinterpret_cast<f32x4*>(const_cast<float*>(a)),
                           reinterpret_cast<const f32x4*>(b), rows, cols / 4, rpc, part, part2, p.a_bs / 4, p.b_bs / 4, (f32x4*)nullptr,
                           (const f32x4*)nullptr, reinterpret_cast<const f32x4*>(p.gelu_pre), p.gelu_rowscale);
    else
        hipLaunchKernelGGL(colsum4_partial_kernel<false>, dim3(chunks, batch), dim3(256), 0, s, reinterpret_cast<const f32x4*>(a),
                           reinterpret_cast<const f32x4*>(b), rows, cols / 4, rpc, part, part2, p.a_bs / 4, p.b_bs / 4,
                           batch == 1 ? reinterpret_cast<f32x4*>(p.scaled_out) : (f32x4*)nullptr, reinterpret_cast<const f32x4*>(p.colscale_out),
                           (const f32x4*)nullptr, (const float*)nullptr);
    ARREAU_CHECK_HIP(hipGetLastError());
    if (deferred) return ARREAU_OK;
    hipLaunchKernelGGL(colsum4_final_kernel, dim3((cols / 4 + 7) / 8, batch), dim3(256), 0, s, part, part2, chunks, cols / 4, p.scale,
                       p.accumulate, p.out, p.out2, p.colscale2, p.out_bs, p.out2_bs);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
int launch_bias_gelu(hipStream_t s, float* pre, const float* bias, const float* rowscale, long rows, int cols, float* act) {
    if (rows <= 0) return ARREAU_OK;
    if (cols % 4 != 0 || ((size_t)pre | (size_t)bias | (size_t)act) % 16 != 0) {
        arreau_set_error("bias_gelu: columns and operands must be 16-byte aligned");
        return ARREAU_EINVAL;
    }
    const long n4 = rows * (cols / 4);
    hipLaunchKernelGGL(bias_gelu_kernel4, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<f32x4*>(pre),
                       reinterpret_cast<const f32x4*>(bias), rowscale, rows, cols / 4, reinterpret_cast<f32x4*>(act));
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
int launch_gelu_backward(hipStream_t s, float* g, const float* pre, const float* rowscale, long rows, int cols) {
    if (rows <= 0) return ARREAU_OK;
    if (cols % 4 != 0 || ((size_t)g | (size_t)pre) % 16 != 0) {
        arreau_set_error("gelu_backward: columns and operands must be 16-byte aligned");
        return ARREAU_EINVAL;
    }
    const long n4 = rows * (cols / 4);
    hipLaunchKernelGGL(gelu_backward_kernel4, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<f32x4*>(g),
                       reinterpret_cast<const f32x4*>(pre), rowscale, rows, cols / 4);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
// pre = X W^T + bias, act = gelu(pre) * rowscale: inside the product where the split kernel takes it, else as the element-wise launch
int linear_bias_gelu(hipStream_t s, arreau_train_ctx& t, long rows, int in, int out, const float* X, const float* W, const float* bias,
                     const float* rowscale, float* pre, float* act) {
    Epi e;
    e.kind = 1; e.vec = bias; e.row = rowscale; e.out = act;
    e.prefer_small = t.fuse;
    bool fused = false;
    int rc = linear(s, t, rows, in, out, X, W, pre, 1.f, 0.f, &e, &fused);
    if (rc || fused) return rc;
    return launch_bias_gelu(s, pre, bias, rowscale, rows, out, act);
}
// dX = (dY W) * gelu'(pre) * rowscale
int linear_dx_gelu_backward(hipStream_t s, arreau_train_ctx& t, long rows, int in, int out, const float* dY, const float* W, const float* pre,
                            const float* rowscale, float* dX) {
    Epi e;
    e.kind = 2; e.mat = pre; e.row = rowscale;
    bool fused = false;
    int rc = linear_dx(s, t, rows, in, out, dY, W, dX, 1.f, 0.f, &e, &fused);
    if (rc || fused) return rc;
    return launch_gelu_backward(s, dX, pre, rowscale, rows, in);
}
// out[m][n] = sum over z = 0 .. Z - 1, in that order, of part[z][m][n] (a running sum from zero: the association of Z accumulating launches)
int ordered_sum(hipStream_t s, const float* part, int Z, int M, int N, float* out) {
    hipLaunchKernelGGL(arreau_sgemm_detail::splitk_reduce_kernel<1>, dim3((unsigned)(((long)M * N + 255) / 256), 1), dim3(256), 0, s, part, Z, M, N, out, N,
                       1.0f, 0.0f, 0L);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}
// the deferred reductions of a backward pass (arreau_train_ctx::Deferred): one launch for the column sums, one for the k-slice sums
void reset_deferred(arreau_train_ctx& t) {
    if (!t.defer) return;
    arreau_sgemm_defer_reset(t.defer->gemm);
    t.defer->ncols = 0; t.defer->max_colblocks = 0; t.defer->colused = 0;
}
int flush_deferred_colsums(hipStream_t s, arreau_train_ctx& t) {
    arreau_train_ctx::Deferred* df = t.defer;
    if (df && df->ncols > 0) {
        hipLaunchKernelGGL(colsum4_final_multi_kernel, dim3(df->max_colblocks, df->ncols), dim3(256), 0, s, df->cols);
        ARREAU_CHECK_HIP(hipGetLastError());
    }
    if (df) { df->ncols = 0; df->max_colblocks = 0; df->colused = 0; }
    return ARREAU_OK;
}
int launch_gathered(hipStream_t s, ColsumGather& g) {
    if (g.n > 0) {
        hipLaunchKernelGGL(colsum4_partial_multi_kernel, dim3(g.chunks, g.n), dim3(256), 0, s, g.list, g.rows, g.rpc);
        ARREAU_CHECK_HIP(hipGetLastError());
    }
    g.n = 0;
    return ARREAU_OK;
}
int flush_deferred_gemms(hipStream_t s, arreau_train_ctx& t) {
    return t.defer ? arreau_sgemm_flush(s, t.defer->gemm) : ARREAU_OK;
}
#define V4(p) reinterpret_cast<const f32x4*>(p)
#define V4W(p) reinterpret_cast<f32x4*>(p)
#define TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
#define LAUNCH(kernel, grid, block, ...)                                  \
    do {                                                                  \
        hipLaunchKernelGGL(kernel, grid, block, 0, s, __VA_ARGS__);       \
        ARREAU_CHECK_HIP(hipGetLastError());                              \
    } while (0)
}  // namespace

void arreau_train_ctx_destroy(arreau_train_ctx* t) {
    if (!t) return;
    if (t->buf) (void)hipFree(t->buf);
    if (t->side) (void)hipStreamDestroy(t->side);
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    if (t->ev_join) (void)hipEventDestroy(t->ev_join);
    if (t->ev_rev) (void)hipEventDestroy(t->ev_rev);
    delete t->defer;
    delete t;
}

static int ensure_ctx(arreau_model* m, int N, int B, hipStream_t s) {
    arreau_train_ctx* t = m->train;
    if (t && N <= t->capN && B <= t->capB) {
        layout(*t, m, t->capN, t->capB, t->buf);
        t->N = N; t->B = B;
        return ARREAU_OK;
    }
    // Growing means a device synchronisation, a free and an allocation of gigabytes (milliseconds): a training loop whose
    // batches creep upwards in size must not pay that every few steps, so a regrown context gets 25 % headroom.
    int capN = N, capB = B;
    if (t) {
        capN = std::max(N, t->capN) + std::max(N, t->capN) / 4;
        capB = std::max(B, t->capB) + std::max(B, t->capB) / 4;
        ARREAU_CHECK_HIP(hipStreamSynchronize(s));
        arreau_train_ctx_destroy(t);
        m->train = nullptr;
        // a cached step graph of arreau_sample_loop (general path) points into the block just freed: never replay it
        m->graph_key = SampleGraphKey{};
    }
    t = new arreau_train_ctx();
    t->defer = new arreau_train_ctx::Deferred();
    t->capN = capN; t->capB = capB;
    arreau_train_ctx probe;
    t->buf_floats = layout(probe, m, capN, capB, nullptr);
    hipError_t e = hipMalloc((void**)&t->buf, t->buf_floats * sizeof(float));
    if (e != hipSuccess) {
        delete t->defer;
        delete t;
        arreau_set_error(std::string("hipMalloc(training buffers): ") + hipGetErrorString(e));
        return ARREAU_EHIP;
    }
    layout(*t, m, capN, capB, t->buf);
    t->N = N; t->B = B;
    m->train = t;
    ARREAU_CHECK_HIP(hipMemsetAsync(t->scratch_cols, 0, 1024 * sizeof(float), s));
    {
        // (read per context, i.e. per model: a test can build the one-stream form beside the default one in one process)
        const bool side_on = [] { const char* e = getenv("ARREAU_TRAIN_SIDE_STREAM"); return !e || atoi(e) != 0; }();
        if (side_on) {
            // (default priority: a lowest-priority side stream measured the same to slightly worse, tools/exp/ab_side_stream.sh)
            ARREAU_CHECK_HIP(hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking));
            ARREAU_CHECK_HIP(hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming));
            ARREAU_CHECK_HIP(hipEventCreateWithFlags(&t->ev_join, hipEventDisableTiming));
            ARREAU_CHECK_HIP(hipEventCreateWithFlags(&t->ev_rev, hipEventDisableTiming));
        }
    }
    hipLaunchKernelGGL(mono_columns_kernel, dim3(1), dim3(128), 0, s, t->mono_cols);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

// Side stream of the fiber branch.  fork: everything queued on `main_stream` so far happens before the side work; `ts` becomes a view
// of the context with the side stream's own scratch, `s` the stream to launch on (the main stream itself when the side stream is
// off: then this is a no-op and the work stays in line).  join: the main stream waits for the side work recorded in ev_join.
static int fork_side(arreau_train_ctx& t, hipStream_t main_stream, arreau_train_ctx& ts, hipStream_t& s) {
    ts = t;
    s = main_stream;
    if (!t.side) return ARREAU_OK;
    ARREAU_CHECK_HIP(hipEventRecord(t.ev_fork, main_stream));
    ARREAU_CHECK_HIP(hipStreamWaitEvent(t.side, t.ev_fork, 0));
    ts.partial = t.partial2; ts.colpart = t.colpart2;
    s = t.side;
    return ARREAU_OK;
}
static int join_side(arreau_train_ctx& t, hipStream_t main_stream) {
    if (!t.side) return ARREAU_OK;
    ARREAU_CHECK_HIP(hipStreamWaitEvent(main_stream, t.ev_join, 0));
    return ARREAU_OK;
}

// The fiber branch of the forward pass, on the stream and the context view fork_side hands out: fiber basis (ponita.py:66,95) and the
// fiber kernels of all layers, fk_l = fkb . Wfk_l^T (conv.py:113-116; one batched product)
static int fiber_forward(hipStream_t s, arreau_train_ctx& t, const arreau_model* m) {
    const int C = m->C, D = m->D, L = m->L;
    LAUNCH(fiber_poly_kernel, dim3(1), dim3(256), m->ori, t.fpoly);
    TRY(linear(s, t, 256, 3, C, t.fpoly, m->fiber_w1, t.fh1pre));
    TRY(launch_bias_gelu(s, t.fh1pre, m->fiber_b1, (const float*)nullptr, 256L, C, t.fh1));
    TRY(linear_bias_gelu(s, t, 256, C, D, t.fh1, m->fiber_w2, m->fiber_b2, (const float*)nullptr, t.fh2pre, t.fkb));
    TRY(arreau_sgemm(s, t.partial, 256, C, D, t.fkb, D, 1, m->fiber_wk, 1, D, t.fk, C, 1.f, 0.f, L, 0, (long)C * D, 256L * C, t.fwd_mode));
    return ARREAU_OK;
}

// The network from the edge basis to the read-outs, on graph arrays and layer-0 features supplied by the caller (t.x).
int arreau_general_network(arreau_model* m, const arreau_graph_view& g, const int32_t* d_off, int B, int N, float* d_eps,
                           float* d_logits, float* d_len0, hipStream_t s) {
    ARREAU_REQUIRE(m->train && m->train->capN >= N && m->train->capB >= B, "arreau_general_network: context not prepared");
    arreau_train_ctx& t = *m->train;
    const int C = m->C, D = m->D, L = m->L, H = m->H, k = m->k, S = m->S, RO = S + 4;
    const long R = (long)N * k * 16, M = (long)N * 16;
    if (N == 0) return ARREAU_OK;
    t.fuse = train_fuse_on();
    // edge basis: kb = gelu(W2 gelu(W1 poly + b1) + b2) * window   (ponita.py:65,94)
    auto edge_basis = [&]() -> int {
        LAUNCH(edge_rows_kernel, dim3(blocks(R)), dim3(256), g.dir, g.dist, g.deg, g.batch, g.lattice, m->ori, m->cfg.radius, N, k,
               t.mono, t.window);
        if (t.fuse) {   // (round 5: bias + GELU inside the product on its 64 x 64 tiles, as layer 2 and the ConvNext block had them)
            TRY(linear_bias_gelu(s, t, R, ARREAU_MONO_PAD, C, t.mono, t.w1f, m->b1, (const float*)nullptr, t.h1pre, t.h1));
        } else {
            TRY(linear(s, t, R, ARREAU_MONO_PAD, C, t.mono, t.w1f, t.h1pre));
            TRY(launch_bias_gelu(s, t.h1pre, m->b1, (const float*)nullptr, R, C, t.h1));
        }
        TRY(linear_bias_gelu(s, t, R, C, D, t.h1, t.w2, m->b2, (const float*)t.window, t.h2pre, t.kb));
        // kernel_l = kb . Wk_l^T for all layers in one product (conv.py:110; conv.kernel.weight stacked [L*C][D])
        TRY(linear(s, t, R, D, L * C, t.kb, t.wk, t.kern));
        return ARREAU_OK;
    };
    {   // the fiber branch: functions of the weights alone -- on the side stream, beside the edge basis
        arreau_train_ctx ts;
        hipStream_t ss;
        TRY(fork_side(t, s, ts, ss));
        // (the main stream's products are handed to the driver before the side branch's small launches: no difference in a free-running
        // loop -- the host is far ahead -- but under a tracer, whose launches cost more, the main stream no longer sits idle here)
        TRY(edge_basis());
        TRY(fiber_forward(ss, ts, m));
        if (t.side) ARREAU_CHECK_HIP(hipEventRecord(t.ev_join, t.side));
    }
    TRY(join_side(t, s));   // the fiber kernels: first used by the layer loop below
    for (int l = 0; l < L; ++l) {
        const float* xl = t.x + (size_t)l * M * C;
        float* xnext = t.x + (size_t)(l + 1) * M * C;
        float* x1 = t.x1 + (size_t)l * M * C;
        float* fk = t.fk + (size_t)l * 256 * C;
        if (t.fwd_mode == 1 && arreau_mlp_train_forward_available(m) && t.fuse && k == 8) {
            // round 5: spatial conv + spherical mix + LayerNorm + linear_1 + GELU + linear_2 + layer scale + residual as ONE launch of the
            // sampling step's one-node-per-workgroup kernel (node_f16m.hip, FUSE + TRAIN), which writes everything the backward pass reads
            TRY(arreau_launch_mlp_train_forward(m, l, nullptr, xl, xnext, t.xhat + (size_t)l * M * C, t.rstd + (size_t)l * M,
                                                t.xn_all + (size_t)l * M * C, t.hpre + (size_t)l * M * H, t.h + (size_t)l * M * H,
                                                t.out + (size_t)l * M * C, N, s, t.kern + (size_t)l * C, L * C, g.deg, g.src, fk, x1));
            continue;
        }
        if (t.fuse) {
            hipLaunchKernelGGL(conv_mix_forward_kernel4, dim3((unsigned)N), dim3(512), (size_t)16 * C * sizeof(float), s, V4(t.kern + (size_t)l * C),
                               L * C / 4, V4(xl), g.deg, g.src, N, k, C / 4, V4(fk), V4(m->conv_bias + (size_t)l * C), V4W(x1), V4W(t.dtmp));
            ARREAU_CHECK_HIP(hipGetLastError());
        } else {
            LAUNCH(conv_forward_kernel4, dim3(blocks(M * C / 4)), dim3(256), V4(t.kern + (size_t)l * C), L * C / 4, V4(xl), g.deg, g.src, N, k,
                   C / 4, V4W(x1));
            LAUNCH(mix_forward_kernel4, dim3(blocks(M * C / 4)), dim3(256), V4(x1), V4(fk), V4(m->conv_bias + (size_t)l * C), N, C / 4, V4W(t.dtmp));
        }
        float* hpre = t.hpre + (size_t)l * M * H;
        float* h = t.h + (size_t)l * M * H;
        float* out = t.out + (size_t)l * M * C;
        if (t.fwd_mode == 1 && arreau_mlp_train_forward_available(m)) {
            // LayerNorm + linear_1 + GELU + linear_2 + layer scale + residual as ONE launch of the sampling step's kernel, which also
            // writes what the backward pass reads (node_f16m.hip, TRAIN): 3 launches per layer instead of 5
            TRY(arreau_launch_mlp_train_forward(m, l, t.dtmp, xl, xnext, t.xhat + (size_t)l * M * C, t.rstd + (size_t)l * M,
                                                t.xn_all + (size_t)l * M * C, hpre, h, out, N, s));
            continue;
        }
        LAUNCH(ln_forward_kernel, dim3(blocks(M, 4)), dim3(256), t.dtmp, m->ln_w + (size_t)l * C, m->ln_b + (size_t)l * C, M, C,
               t.xhat + (size_t)l * M * C, t.rstd + (size_t)l * M, t.xn_all + (size_t)l * M * C);
        TRY(linear_bias_gelu(s, t, M, C, H, t.xn_all + (size_t)l * M * C, t.lin1 + (size_t)l * H * C, m->mb1 + (size_t)l * H, (const float*)nullptr,
                             hpre, h));
        {   // out = h W2^T + b2;  x_{l+1} = out * layer_scale + x_l  (in the product's epilogue where the split kernel runs it)
            Epi e;
            e.kind = 3; e.vec = m->mb2 + (size_t)l * C; e.vec2 = m->ls + (size_t)l * C; e.mat = xl; e.out = xnext;
            bool fused = false;
            TRY(linear(s, t, M, H, C, h, t.lin2 + (size_t)l * C * H, out, 1.f, 0.f, &e, &fused));
            if (!fused)
                LAUNCH(bias_scale_residual_kernel, dim3(blocks(M * C)), dim3(256), out, m->mb2 + (size_t)l * C, m->ls + (size_t)l * C, xl, M, C, xnext);
        }
    }
    // read-outs of all layers, averaged (ponita.py:105,108; biases are added in train_outputs_kernel): ONE batched product over the kept
    // x_1 .. x_L and a sum in layer order -- the same products and the same association as L accumulating launches inside the loop
    TRY(arreau_sgemm(s, t.partial, (int)M, RO, C, t.x + (size_t)M * C, C, 1, t.ro_w, 1, C, t.rbar_all, RO, 1.0f / (float)L, 0.f, L, (long)M * C,
                     (long)RO * C, (long)M * RO, t.fwd_mode));
    if (t.fuse) {
        LAUNCH(train_outputs_kernel, dim3(N), dim3(128), t.rbar_all, m->ro_b, m->ori, S, L, N, d_eps, d_logits, t.gs, L);
    } else {
        TRY(ordered_sum(s, t.rbar_all, L, (int)M, RO, t.rbar));
        LAUNCH(train_outputs_kernel, dim3(N), dim3(128), t.rbar, m->ro_b, m->ori, S, L, N, d_eps, d_logits, t.gs, 0);
    }
    LAUNCH(pool_crystals_kernel, dim3(blocks(3 * B, 128)), dim3(128), t.gs, d_off, B, d_len0);
    m->ran = ScorePlan{.general = true};
    return ARREAU_OK;
}

float* arreau_general_x0(arreau_model* m, int N, int B, hipStream_t s) {
    if (ensure_ctx(m, N, B, s) != ARREAU_OK) return nullptr;
    m->train->fwd_mode = 0;  // sampling through the shape-general path: exact fp32 products
    return m->train->x;
}

extern "C" int arreau_train_forward(arreau_model* m, const float* d_frac, const int32_t* d_types, const float* d_lengths,
                                    const float* d_angles, const int32_t* d_t, const int32_t* d_off, int32_t B, int32_t N,
                                    float* d_eps, float* d_logits, float* d_len0, void* stream) {
    ARREAU_REQUIRE(m && d_frac && d_types && d_lengths && d_angles && d_t && d_off && d_eps && d_logits && d_len0,
                   "arreau_train_forward: null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 1, "arreau_train_forward: bad size");
    hipStream_t s = (hipStream_t)stream;
    TRY(ensure_ctx(m, N, B, s));
    arreau_train_ctx& t = *m->train;
    const int C = m->C, k = m->k, S = m->S;
    const long M = (long)N * 16;
    t.fuse = train_fuse_on();
    {
        static const int env = [] {
            const char* e = getenv("ARREAU_TRAIN_GEMM");
            return !e || strcmp(e, "split") == 0 ? 1 : strcmp(e, "fp16") == 0 ? 2 : 0;
        }();
        // (fp16x3 while the weights fit fp16 and the caller has not asked for the full-range kernels -- arreau_model_set_variant(-1 or 3, 1),
        // what PONITA_DIFFUSION.training_step does after a non-finite step: the operand bounds of arreau_model_create do not follow
        // the optimizer; arreau_model_create itself sets train_full_range for a model whose bounds start a chain on bf16x6)
        t.fwd_mode = env == 0 ? 0 : (m->f16_ok && !m->train_full_range ? 1 : 2);
        t.bwd_mode = env == 0 ? 0 : (env == 2 && m->f16_ok ? 1 : 2);
    }
    const bool side_setup = t.side != nullptr && t.fuse;
    // (a previous forward's reversed adjacency may still be in flight on the side stream: the neighbour list below rewrites its input)
    if (t.rev_pending) { ARREAU_CHECK_HIP(hipStreamWaitEvent(s, t.ev_rev, 0)); t.rev_pending = false; }
    // geometry and graph: the sampling path's own kernels (prep, neighbour list)
    TRY(arreau_launch_prep(m, d_frac, d_lengths, d_angles, d_t, d_off, B, N, t.lattice, t.cart, t.batch, t.cvec, s));
    TRY(arreau_launch_neighbor(t.cart, t.lattice, d_off, t.batch, B, N, m->cfg.radius, k, t.deg, t.src, t.cell, t.dir, t.dist, s));
    // embedding (ponita.py:98): x_0 = F . W_emb^T, embT = W_emb^T [S+78][C]  (F is kept for the embedder's gradient).  Round 5: on the
    // side stream, in front of the network's fiber branch and beside its edge-level products -- x_0 is first read by the layer loop,
    // behind arreau_general_network's join.  (It needs prep's outputs only, but is NOT started beside the neighbour list: kernels of two
    // streams sharing a CU is where round 2 saw a receiver's neighbour list lose a candidate -- DESIGN.md section 8, cause unknown --
    // and a wrong edge is a different graph, not a rounding difference.)
    {
        arreau_train_ctx ts = t;
        hipStream_t ss = s;
        if (side_setup) TRY(fork_side(t, s, ts, ss));
        hipLaunchKernelGGL(features_kernel, dim3((unsigned)M), dim3(64), 0, ss, d_frac, d_types, d_lengths, d_angles, d_t, d_off, t.batch, t.lattice,
                           m->vp_betas, m->t_emb_w, m->ori, S, m->T, N, t.F);
        ARREAU_CHECK_HIP(hipGetLastError());
        TRY(gemm(ss, ts, t.fwd_mode, (int)M, C, S + 78, t.F, S + 78, 1, m->embT, C, 1, t.x, C));
    }
    // sender-side adjacency of this step's graph, for the ordered, atomic-free d(x_l) of the spatial conv in the backward pass
    // (built here, while the caller's offsets are certainly alive: the backward pass reads only the context's own arrays).  Round 5: only
    // the backward pass reads it, so it runs on the side stream behind the network's fiber branch (which waits for the neighbour list:
    // fork_side in arreau_general_network) and the backward pass waits for ev_rev
    if (!side_setup) LAUNCH(reverse_adjacency_kernel, dim3((unsigned)B), dim3(1024), d_off, t.deg, t.src, k, t.rev_start, t.rev_cnt, t.rev_idx);
    const int rc = arreau_general_network(m, arreau_graph_view{t.batch, t.deg, t.src, t.lattice, t.dir, t.dist}, d_off, B, N, d_eps,
                                          d_logits, d_len0, s);
    if (rc) return rc;
    if (side_setup) {
        hipLaunchKernelGGL(reverse_adjacency_kernel, dim3((unsigned)B), dim3(1024), 0, t.side, d_off, t.deg, t.src, k, t.rev_start, t.rev_cnt, t.rev_idx);
        ARREAU_CHECK_HIP(hipGetLastError());
        ARREAU_CHECK_HIP(hipEventRecord(t.ev_rev, t.side));
        t.rev_pending = true;
    }
    return ARREAU_OK;
}

// The fiber branch of the backward pass, on the stream and the context view fork_side hands out (the helpers take their scratch from the
// context they are handed): d(fiber kernel) of every layer and from there everything down to d(fiber_basis_fn).
static int fiber_backward(hipStream_t s, arreau_train_ctx& t, const arreau_model* m, const arreau_state_dict* g) {
    const int N = t.N, C = m->C, D = m->D, L = m->L;
    auto W = [](const float* p) { return const_cast<float*>(p); };
    // partial sums live in the split-K scratch (free here): as many layers per pair of launches as fit it -- all L at the
    // bench's 64 crystals, one at the reference's `make train` preset (batch 270, hidden_dim 200: ~2,200 atoms) -- and
    // atom chunks that grow with the batch once a single layer's partial sums would not fit
    int chunk = MIX_CHUNK;
    while ((size_t)((N + chunk - 1) / chunk) * 256 * C > PARTIAL_FLOATS) chunk *= 2;
    const int chunks = (N + chunk - 1) / chunk;
    const int Lg = (int)std::min<size_t>((size_t)L, PARTIAL_FLOATS / ((size_t)chunks * 256 * C));
    for (int l0 = 0; l0 < L; l0 += Lg) {
        const int nl = std::min(Lg, L - l0);
        LAUNCH(mix_backward_fk_partial_kernel, dim3(chunks, nl), dim3(128), t.x1 + (size_t)l0 * N * 16 * C,
               t.dx2_all + (size_t)l0 * N * 16 * C, N, C, t.partial, chunk);
        LAUNCH(mix_backward_fk_final_kernel, dim3(blocks(256L * C), nl), dim3(256), t.partial, chunks, C, t.dfk_all + (size_t)l0 * 256 * C);
    }
    // d(fiber basis) = sum over layers of d(fk_l) . Wfk_l: one batched product, summed in the order of the layer loop (L - 1 first:
    // slot z of the scratch holds layer L - 1 - z)
    TRY(arreau_sgemm(s, t.partial, 256, D, C, t.dfk_all + (size_t)(L - 1) * 256 * C, C, 1, m->fiber_wk + (size_t)(L - 1) * C * D, D, 1, t.dfkb_all, D,
                     1.0f, 0.f, L, -256L * C, -(long)C * D, 256L * D, t.bwd_mode));
    TRY(ordered_sum(s, t.dfkb_all, L, 256, D, t.dfkb));
    TRY(linear_dw_batched(s, t, L, 256, D, C, t.dfk_all, 256L * C, t.fkb, 0, W(g->conv_fiber_w)));
    // fiber basis MLP
    TRY(launch_gelu_backward(s, t.dfkb, t.fh2pre, (const float*)nullptr, 256L, D));
    TRY(linear_dw(s, t, 256, C, D, t.dfkb, t.fh1, W(g->fiber_w2)));
    TRY(colsum(s, t, {.a = t.dfkb, .rows = 256, .cols = D, .out = W(g->fiber_b2)}));
    TRY(linear_dx_gelu_backward(s, t, 256, C, D, t.dfkb, m->fiber_w2, t.fh1pre, (const float*)nullptr, t.dfh1));
    TRY(linear_dw(s, t, 256, 3, C, t.dfh1, t.fpoly, W(g->fiber_w1)));
    TRY(colsum(s, t, {.a = t.dfh1, .rows = 256, .cols = C, .out = W(g->fiber_b1)}));
    return ARREAU_OK;
}

extern "C" int arreau_train_backward(arreau_model* m, const float* d_g_eps, const float* d_g_logits, const float* d_g_len0,
                                     const arreau_state_dict* g, void* stream) {
    ARREAU_REQUIRE(m && d_g_eps && d_g_logits && d_g_len0 && g, "arreau_train_backward: null pointer");
    ARREAU_REQUIRE(m->train && m->train->N > 0, "arreau_train_backward: call arreau_train_forward first");
    const float* need[] = {g->basis_w1, g->basis_b1, g->basis_w2, g->basis_b2, g->fiber_w1, g->fiber_b1, g->fiber_w2, g->fiber_b2,
                           g->x_embedder_w, g->conv_kernel_w, g->conv_fiber_w, g->conv_bias, g->norm_w, g->norm_b, g->linear1_w,
                           g->linear1_b, g->linear2_w, g->linear2_b, g->readout_w, g->readout_b};
    for (const float* p : need) ARREAU_REQUIRE(p != nullptr, "arreau_train_backward: missing gradient buffer");
    ARREAU_REQUIRE(!m->cfg.has_layer_scale || g->layer_scale, "arreau_train_backward: missing layer_scale gradient buffer");
    hipStream_t s = (hipStream_t)stream;
    arreau_train_ctx& t = *m->train;
    const int N = t.N, C = m->C, D = m->D, L = m->L, H = m->H, k = m->k, S = m->S, RO = S + 4;
    const long R = (long)N * k * 16, M = (long)N * 16;
    auto W = [](const float* p) { return const_cast<float*>(p); };  // the gradient struct reuses the const state_dict type
    t.fuse = train_fuse_on();
    const bool fuse = t.fuse;
    reset_deferred(t);
    if (t.rev_pending) { ARREAU_CHECK_HIP(hipStreamWaitEvent(s, t.ev_rev, 0)); t.rev_pending = false; }
    // d(rbar) [M][ROP], ROP = RO rounded up to a multiple of four with zero pad columns (round 5): its products and its column sum run on
    // 16-byte fetches -- 94 columns sent the d(x) product to the exact fp32 kernel (24.6 us) and the bias gradient to the element-wise
    // column sum (15.1 us); the weight operand's pad rows are the next layer's first rows resp. zeros behind the last layer (model.hip)
    const int ROP = (RO + 3) & ~3;
    LAUNCH(train_outputs_backward_kernel, dim3((unsigned)M), dim3(128), d_g_eps, d_g_logits, d_g_len0, t.batch, m->ori, S, N, t.drbar, ROP);
    // The read-outs' contributions to d x_{l+1} = d(rbar) . W_ro,l / L depend on nothing inside the layer loop: ONE batched product for all
    // layers up front (they were L launches of the element-wise-fetch kernel -- 94 read-out columns are no multiple of four -- 13.6 us
    // each inside the chain); layer L - 1 starts from its slice, the others are added by the launch that completes d x_{l+1}.
    TRY(arreau_sgemm(s, t.partial, (int)M, C, ROP, t.drbar, ROP, 1, t.ro_w, C, 1, t.dxro, C, 1.0f / (float)L, 0.f, L, 0, (long)RO * C, (long)M * C,
                     t.bwd_mode));
    const float invL = 1.0f / (float)L;
    for (int l = L - 1; l >= 0; --l) {
        const float* xl = t.x + (size_t)l * M * C;
        const float* xhat = t.xhat + (size_t)l * M * C;
        const float* fk = t.fk + (size_t)l * 256 * C;
        const float* hpre = t.hpre + (size_t)l * M * H;
        const float* out = t.out + (size_t)l * M * C;
        // read-out (ponita.py:105,108); its weight gradient: one batched product over the layers, below the loop
        // (every layer's read-out sees the same d(rbar): the bias gradients are equal -- copied to the other layers in one launch below)
        // (ROP sums into the scratch row -- the pad columns sum to zero --, copied to every layer's slice at the end of the pass)
        // (with the batched column-sum pass behind the loop when the launches are merged: nothing waits for it)
        if (l == L - 1 && !fuse) TRY(colsum(s, t, {.a = t.drbar, .rows = M, .cols = ROP, .scale = invL, .out = t.robias, .defer = true}));
        const float* dxl = l == L - 1 ? t.dxro + (size_t)l * M * C : t.dx + (size_t)(l + 1) * M * C;   // d x_{l+1}
        float* dxo = t.dx + (size_t)l * M * C;                                                        // d x_l
        // round 5: below the top layer d(out) = d(x_{l+1}) * layer_scale was written by the previous iteration's conv-gradient launch, and
        // the column sums over d(x_{l+1}) (d(layer_scale), d(linear_2.bias): results nothing waits for) leave the chain: one batched
        // pass behind the loop.  The same multiplies and the same sums.
        const bool dout_ahead = m->cfg.has_layer_scale && fuse;
        const float* dx_add = l > 0 ? t.dxro + (size_t)(l - 1) * M * C : nullptr;
        // ConvNext tail: x_{l+1} = out * ls + x_l
        // d(layer_scale) = sum_rows dx * out and d(linear_2.bias) = sum_rows dout = ls * sum_rows dx, in one pass over dx
        // (d(out) = d(x) * layer_scale rides in the same pass; a model without layer_scale multiplies by its row of ones below)
        float* dout = t.dout_all + (size_t)l * M * C;
        if (m->cfg.has_layer_scale && !(dout_ahead && l < L - 1))
            TRY(colsum(s, t, {.a = dxl, .b = out, .rows = M, .cols = C, .out = W(g->layer_scale) + (size_t)l * C,
                              .out2 = W(g->linear2_b) + (size_t)l * C, .colscale2 = m->ls + (size_t)l * C, .scaled_out = dout,
                              .colscale_out = m->ls + (size_t)l * C, .defer = true}));
        // (the weight gradients of linear_2, linear_1, the read-out and the fiber kernel are products nothing below waits for:
        // their operands are kept per layer and each kind runs as ONE batched product after the loop)
        float* dh = t.dh + (size_t)l * M * H;
        if (!m->cfg.has_layer_scale) {
            LAUNCH(scale_cols_kernel, dim3(blocks(M * C)), dim3(256), dxl, m->ls + (size_t)l * C, M, C, dout);   // dout
            TRY(colsum(s, t, {.a = dout, .rows = M, .cols = C, .out = W(g->linear2_b) + (size_t)l * C}));
        }
        TRY(linear_dx_gelu_backward(s, t, M, H, C, dout, t.lin2 + (size_t)l * C * H, hpre, (const float*)nullptr, dh));   // dhpre
        float* dxn = t.dxn_all + (size_t)l * M * C;
        float* dx2 = t.dx2_all + (size_t)l * M * C;
        TRY(linear_dx(s, t, M, C, H, dh, t.lin1 + (size_t)l * H * C, dxn));                                          // dxn
        if (!fuse)
            LAUNCH(ln_backward_kernel, dim3(blocks(M, 4)), dim3(256), dxn, xhat, t.rstd + (size_t)l * M, m->ln_w + (size_t)l * C, M, C, dx2);
        // spherical conv: x2 = mix(x1, fk) / 16 + bias
        // spatial conv: x1 = sum_s kern * x_l[src]; the residual path already sits in dx (= d x_l so far)
        if (fuse) {
            hipLaunchKernelGGL(ln_mix_backward_kernel4, dim3((unsigned)N), dim3(1024), (size_t)16 * C * sizeof(float), s, dxn, xhat,
                               t.rstd + (size_t)l * M, m->ln_w + (size_t)l * C, V4(fk), N, C, dx2, V4W(t.dx1));
            ARREAU_CHECK_HIP(hipGetLastError());
            const unsigned dx_blocks = blocks(M * C / 4), kern_blocks = blocks(R * C / 4);
            LAUNCH(conv_backward_both_kernel4, dim3(dx_blocks + kern_blocks), dim3(256), (int)dx_blocks, V4(xl), V4(t.dx1), t.deg, t.src,
                   V4(t.kern + (size_t)l * C), L * C / 4, t.rev_start, t.rev_cnt, t.rev_idx, N, k, C / 4, V4(dxl),
                   dx_add ? V4(dx_add) : (const f32x4*)nullptr, V4W(dxo), V4W(t.dkern + (size_t)l * C),
                   dout_ahead && l > 0 ? V4W(t.dout_all + (size_t)(l - 1) * M * C) : (f32x4*)nullptr, V4(m->ls + (size_t)(l > 0 ? l - 1 : 0) * C));
        } else {
            LAUNCH(mix_backward_x_kernel4, dim3(blocks(M * C / 4)), dim3(256), V4(dx2), V4(fk), N, C / 4, V4W(t.dx1));
            LAUNCH(conv_backward_kern_kernel4, dim3(blocks(R * C / 4)), dim3(256), V4(xl), V4(t.dx1), t.deg, t.src, N, k, C / 4, L * C / 4,
                   V4W(t.dkern + (size_t)l * C));
            LAUNCH(conv_backward_dx_kernel4, dim3(blocks(M * C / 4)), dim3(256), V4(t.kern + (size_t)l * C), L * C / 4, V4(t.dx1), t.rev_start,
                   t.rev_cnt, t.rev_idx, N, k, C / 4, V4(dxl), dx_add ? V4(dx_add) : (const f32x4*)nullptr, V4W(dxo));
        }
    }
    // d(fiber kernel) of every layer = sum over nodes of x1 (x) dx2 / 16: one batched pair of launches (both operands were kept
    // per layer), then its two uses -- and from there the whole fiber branch down to d(fiber_basis_fn): on the side stream, beside the
    // edge-level weight gradients below (it reads x1 and d(x2) of the loop above and writes gradients nothing else touches)
    // the layers' weight gradients, one batched product per kind (operands kept per layer above / by the forward pass), and the batched
    // column sums: main-stream work that depends on nothing of the side branch
    auto main_batched = [&]() -> int {
        // (round 5: the k-slice sums of these products and the chunk sums of the column-sum passes below wait for the two launches at the
        // end of this function)
        TRY(linear_dw_batched(s, t, L, M, C, RO, t.drbar, 0, t.x + (size_t)M * C, (long)M * C, W(g->readout_w), invL, true, ROP));         // x_{l+1}
        TRY(linear_dw_batched(s, t, L, M, H, C, t.dout_all, (long)M * C, t.h, (long)M * H, W(g->linear2_w), 1.f, true));
        TRY(linear_dw_batched(s, t, L, M, C, H, t.dh, (long)M * H, t.xn_all, (long)M * C, W(g->linear1_w), 1.f, true));
        // the k-slice sums of the three products in one launch, while their 65 MB of partial tiles are still in the Infinity Cache
        // (ONE such launch at the very end of the pass read 125 MB of long-evicted tiles from HBM in plane-strided pieces: 60 us
        // against 49 us for the seven separate sums; per cluster of products it is three launches fewer and faster than both)
        TRY(flush_deferred_gemms(s, t));
        // ... and the column sums: d(linear_1.bias) = sum_rows dhpre; d(norm.weight) = sum_rows dxn * xhat and d(norm.bias) = sum_rows dxn
        // in one pass over dxn; d(conv.bias) = sum_rows dx2
        // (round 5: the three passes as ONE launch where their chunk sums are deferred -- 15 matrices of the same row count)
        ColsumGather cg;
        if (fuse)   // d(readout bias): the one column sum of d(rbar) (scratch row, copied to every layer's slice at the end)
            TRY(colsum(s, t, {.a = t.drbar, .rows = M, .cols = ROP, .scale = invL, .out = t.robias, .defer = true, .gather = &cg}));
        TRY(colsum(s, t, {.a = t.dh, .rows = M, .cols = H, .out = W(g->linear1_b), .batch = L, .a_bs = (long)M * H, .out_bs = H, .defer = true,
                          .gather = &cg}));
        TRY(colsum(s, t, {.a = t.dxn_all, .b = t.xhat, .rows = M, .cols = C, .out = W(g->norm_w), .out2 = W(g->norm_b), .batch = L,
                          .a_bs = (long)M * C, .b_bs = (long)M * C, .out_bs = C, .out2_bs = C, .defer = true, .gather = &cg}));
        TRY(colsum(s, t, {.a = t.dx2_all, .rows = M, .cols = C, .out = W(g->conv_bias), .batch = L, .a_bs = (long)M * C, .out_bs = C,
                          .defer = true, .gather = &cg}));
        // d(layer_scale) = sum_rows d(x_{l+1}) * out_l and d(linear_2.bias) = layer_scale * sum_rows d(x_{l+1}) of the layers below the top one
        // (the top layer's pass ran at the head of the loop; d(x_{l+1}) = slice l + 1 of the kept d(x))
        if (m->cfg.has_layer_scale && fuse && L > 1)
            TRY(colsum(s, t, {.a = t.dx + (size_t)M * C, .b = t.out, .rows = M, .cols = C, .out = W(g->layer_scale), .out2 = W(g->linear2_b),
                              .colscale2 = m->ls, .batch = L - 1, .a_bs = (long)M * C, .b_bs = (long)M * C, .out_bs = C, .out2_bs = C,
                              .colscale2_bs = C, .defer = true, .gather = &cg}));
        TRY(launch_gathered(s, cg));
        return ARREAU_OK;
    };
    {
        arreau_train_ctx ts;
        hipStream_t ss;
        TRY(fork_side(t, s, ts, ss));
        TRY(main_batched());   // (before the side branch's two dozen small launches: see the forward pass)
        TRY(fiber_backward(ss, ts, m, g));
        if (t.side) ARREAU_CHECK_HIP(hipEventRecord(t.ev_join, t.side));
    }
    // kernel projections of all layers at once: dWk [L*C][D] = dkern^T . kb,  dkb = dkern . Wk
    TRY(linear_dw(s, t, R, D, L * C, t.dkern, t.kb, W(g->conv_kernel_w)));
    if (fuse) {
        // (round 5: a 128 x 128 product takes no GELU epilogue -- sgemm.h -- so d(h2pre) = (dkern . Wk) * gelu'(h2pre) * window is finished by
        // the column-sum pass of d(basis_fn.2.bias), which had to read it anyway: one pass over 66 MB instead of two)
        bool fused = false;
        Epi e;
        e.kind = 2; e.mat = t.h2pre; e.row = t.window;
        TRY(linear_dx(s, t, R, D, L * C, t.dkern, t.wk, t.dkb, 1.f, 0.f, &e, &fused));
        TRY(colsum(s, t, {.a = t.dkb, .rows = R, .cols = D, .out = W(g->basis_b2), .defer = true, .gelu_pre = fused ? nullptr : t.h2pre,
                          .gelu_rowscale = fused ? nullptr : t.window}));
    } else
    TRY(linear_dx_gelu_backward(s, t, R, D, L * C, t.dkern, t.wk, t.h2pre, (const float*)t.window, t.dkb));   // dh2pre
    // embedding: x_0 = F . W_emb^T  -> dW_emb[c][i] = sum_rows dx[row][c] F[row][i]
    TRY(linear_dw(s, t, M, S + 78, C, t.dx, t.F, W(g->x_embedder_w), 1.f, true));
    // edge basis MLP
    TRY(linear_dw(s, t, R, C, D, t.dkb, t.h1, W(g->basis_w2), 1.f, true));
    TRY(flush_deferred_gemms(s, t));     // (x_embedder and basis_fn.2 weight gradients: one launch)
    if (!fuse) TRY(colsum(s, t, {.a = t.dkb, .rows = R, .cols = D, .out = W(g->basis_b2), .defer = true}));
    TRY(linear_dx_gelu_backward(s, t, R, C, D, t.dkb, t.w2, t.h1pre, (const float*)nullptr, t.dh1));   // dh1pre
    TRY(linear_dw(s, t, R, ARREAU_MONO_PAD, C, t.dh1, t.mono, t.dw1f));
    TRY(colsum(s, t, {.a = t.dh1, .rows = R, .cols = C, .out = W(g->basis_b1), .defer = true}));
    TRY(flush_deferred_gemms(s, t));     // (nothing pending on the default path: a product that did not fit its cluster's scratch)
    TRY(flush_deferred_colsums(s, t));   // every bias / norm / layer-scale gradient's chunk sum: one launch
    {   // d(readout bias): every layer's read-out sees the same d(rbar), so the one column sum (scratch row, complete behind the launch
        // above) is copied to all L slices
        CopySegments seg;
        const int nseg = std::min(L, 24);
        for (int l = 0; l < nseg; ++l) {
            seg.dst[l] = W(g->readout_b) + (size_t)l * RO; seg.src[l] = t.robias; seg.n[l] = (unsigned)RO;
        }
        LAUNCH(copy_segments_kernel, dim3(1, nseg), dim3(128), seg);
        for (int l = nseg; l < L; ++l)  // (more than 24 layers: the rest one by one)
            ARREAU_CHECK_HIP(hipMemcpyAsync(W(g->readout_b) + (size_t)l * RO, t.robias, RO * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    LAUNCH(unfold_poly_grad_kernel, dim3(blocks((long)C * ARREAU_POLY_COLS)), dim3(256), t.dw1f, C, W(g->basis_w1));
    TRY(join_side(t, s));   // the fiber branch's gradients are complete when this call's work is
    return ARREAU_OK;
}

// activation statistics of the first training forward for FiberBundleConv.callibrate (conv.py:121-123,140-146): the
// unbiased standard deviations of x (layer input), x_1 (after the spatial conv) and x_2 (after the spherical conv,
// before the bias) of every layer, as torch.std() computes them.   d_stats[L][3]
extern "C" int arreau_train_conv_stats(arreau_model* m, float* d_stats, void* stream) {
    ARREAU_REQUIRE(m && d_stats, "arreau_train_conv_stats: null pointer");
    ARREAU_REQUIRE(m->train && m->train->N > 0, "arreau_train_conv_stats: call arreau_train_forward first");
    hipStream_t s = (hipStream_t)stream;
    arreau_train_ctx& t = *m->train;
    const int N = t.N, C = m->C, L = m->L;
    const long M = (long)N * 16;
    double* part = t.std_part;  // (the launches are stream-ordered)
    auto std_of = [&](const float* a, float* out) {
        LAUNCH(std_partial_kernel, dim3(STD_PARTS), dim3(256), a, M * C, part);
        LAUNCH(std_final_kernel, dim3(1), dim3(256), (const double*)part, M * C, out);
        return ARREAU_OK;
    };
    for (int l = 0; l < L; ++l) {
        const float* xl = t.x + (size_t)l * M * C;
        const float* x1 = t.x1 + (size_t)l * M * C;
        TRY(std_of(xl, d_stats + 3 * l));
        TRY(std_of(x1, d_stats + 3 * l + 1));
        // x_2 without the bias: recompute the mix into scratch
        LAUNCH(mix_forward_kernel4, dim3(blocks(M * C / 4)), dim3(256), V4(x1), V4(t.fk + (size_t)l * 256 * C), V4(t.scratch_cols), N, C / 4,
               V4W(t.dtmp));
        TRY(std_of(t.dtmp, d_stats + 3 * l + 2));
    }
    return ARREAU_OK;
}

// After an optimizer step: refresh the plain fp32 weights the TRAINING path reads (this file, prep_kernel's embT, the
// biases / LayerNorm / layer-scale vectors) from the caller's DEVICE tensors -- device-to-device copies, one fold and one
// transpose kernel, no host work.  The packed operand planes of the sampling kernels are NOT rebuilt: the model is marked
// stale for sampling (arreau_predict_scores & co. then fail loudly) until it is re-created from the new state_dict.
extern "C" int arreau_model_update_train_weights(arreau_model* m, const arreau_state_dict* d, void* stream) {
    ARREAU_REQUIRE(m && d, "arreau_model_update_train_weights: null pointer");
    const float* need[] = {d->basis_w1, d->basis_b1, d->basis_w2, d->basis_b2, d->fiber_w1, d->fiber_b1, d->fiber_w2, d->fiber_b2,
                           d->x_embedder_w, d->conv_kernel_w, d->conv_fiber_w, d->conv_bias, d->norm_w, d->norm_b, d->linear1_w,
                           d->linear1_b, d->linear2_w, d->linear2_b, d->readout_w, d->readout_b};
    for (const float* p : need) ARREAU_REQUIRE(p != nullptr, "arreau_model_update_train_weights: missing state_dict entry");
    hipStream_t s = (hipStream_t)stream;
    const size_t C = m->C, D = m->D, L = m->L, H = m->H, S = m->S, RO = S + 4;
    auto W = [](const float* p) { return const_cast<float*>(p); };
    CopySegments seg;
    int nseg = 0;
    auto cp = [&](const float* dst, const float* src, size_t n) {
        seg.dst[nseg] = W(dst); seg.src[nseg] = src; seg.n[nseg] = (unsigned)n;
        ++nseg;
    };
    m->packed_stale = 1;
    if (!m->train) TRY(ensure_ctx(m, 1, 1, s));  // (the monomial column table lives in the training context)
    LAUNCH(fold_poly_weight_kernel, dim3(blocks((long)C * ARREAU_MONO_PAD)), dim3(256), d->basis_w1, (int)C, m->train->mono_cols, W(m->t_w1f));
    LAUNCH(transpose_kernel, dim3(blocks((long)C * (S + 78))), dim3(256), d->x_embedder_w, (int)C, (int)(S + 78), W(m->embT));
    cp(m->b1, d->basis_b1, C);
    cp(m->t_w2, d->basis_w2, D * C);
    cp(m->b2, d->basis_b2, D);
    cp(m->fiber_w1, d->fiber_w1, C * 3);
    cp(m->fiber_b1, d->fiber_b1, C);
    cp(m->fiber_w2, d->fiber_w2, D * C);
    cp(m->fiber_b2, d->fiber_b2, D);
    cp(m->t_wk, d->conv_kernel_w, L * C * D);
    cp(m->fiber_wk, d->conv_fiber_w, L * C * D);
    cp(m->conv_bias, d->conv_bias, L * C);
    cp(m->ln_w, d->norm_w, L * C);
    cp(m->ln_b, d->norm_b, L * C);
    cp(m->t_lin1, d->linear1_w, L * H * C);
    cp(m->mb1, d->linear1_b, L * H);
    cp(m->t_lin2, d->linear2_w, L * C * H);
    cp(m->mb2, d->linear2_b, L * C);
    if (m->cfg.has_layer_scale && d->layer_scale) cp(m->ls, d->layer_scale, L * C);
    cp(m->t_ro_w, d->readout_w, L * RO * C);
    cp(m->ro_b, d->readout_b, L * RO);
    LAUNCH(copy_segments_kernel, dim3(64, nseg), dim3(256), seg);
    TRY(arreau_repack_mlp_f16x3_m16(m, s));   // the plane stream the fused training forward of the ConvNext block reads
    return ARREAU_OK;
}

// The optimizer's second destination (optim.hip): where arreau_model_update_train_weights would copy each tensor to.  Stacked [L, ...]
// layout, the caller's own state_dict layout; NULL for the two tensors the training entry points read in a derived form.
extern "C" int arreau_model_train_weight_pointers(arreau_model* m, arreau_state_dict* out) {
    ARREAU_REQUIRE(m && out, "arreau_model_train_weight_pointers: null pointer");
    *out = arreau_state_dict{};
    out->basis_b1 = m->b1; out->basis_w2 = m->t_w2; out->basis_b2 = m->b2;
    out->fiber_w1 = m->fiber_w1; out->fiber_b1 = m->fiber_b1; out->fiber_w2 = m->fiber_w2; out->fiber_b2 = m->fiber_b2;
    out->conv_kernel_w = m->t_wk; out->conv_fiber_w = m->fiber_wk; out->conv_bias = m->conv_bias;
    out->norm_w = m->ln_w; out->norm_b = m->ln_b;
    out->linear1_w = m->t_lin1; out->linear1_b = m->mb1; out->linear2_w = m->t_lin2; out->linear2_b = m->mb2;
    if (m->cfg.has_layer_scale) out->layer_scale = m->ls;
    out->readout_w = m->t_ro_w; out->readout_b = m->ro_b;
    return ARREAU_OK;
}

// ... and what is left of arreau_model_update_train_weights when the optimizer has written those itself: the folded polynomial weight
// and the transposed embedder.
extern "C" int arreau_model_refresh_derived_train_weights(arreau_model* m, const float* d_basis_w1, const float* d_x_embedder_w, void* stream) {
    ARREAU_REQUIRE(m && d_basis_w1 && d_x_embedder_w, "arreau_model_refresh_derived_train_weights: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t C = m->C, S = m->S;
    auto W = [](const float* p) { return const_cast<float*>(p); };
    m->packed_stale = 1;
    if (!m->train) TRY(ensure_ctx(m, 1, 1, s));
    LAUNCH(fold_poly_weight_kernel, dim3(blocks((long)C * ARREAU_MONO_PAD)), dim3(256), d_basis_w1, (int)C, m->train->mono_cols, W(m->t_w1f));
    LAUNCH(transpose_kernel, dim3(blocks((long)C * (S + 78))), dim3(256), d_x_embedder_w, (int)C, (int)(S + 78), W(m->embT));
    TRY(arreau_repack_mlp_f16x3_m16(m, s));
    return ARREAU_OK;
}

extern "C" int arreau_debug_sgemm(int32_t mode, int32_t M, int32_t N, int32_t K, const float* d_A, int64_t as0, int64_t as1, const float* d_B,
                                  int64_t bs0, int64_t bs1, float* d_C, int32_t ldc, float alpha, float beta, void* stream) {
    ARREAU_REQUIRE(d_A && d_B && d_C, "arreau_debug_sgemm: null pointer");
    ARREAU_REQUIRE(M >= 0 && N >= 0 && K >= 1 && ldc >= N && mode >= 0 && mode <= 2, "arreau_debug_sgemm: bad size or mode");
    ARREAU_REQUIRE((as0 == 1 || as1 == 1) && (bs0 == 1 || bs1 == 1), "arreau_debug_sgemm: one stride of each operand must be 1");
    hipStream_t s = (hipStream_t)stream;
    float* partial = nullptr;
    ARREAU_CHECK_HIP(hipMalloc((void**)&partial, ARREAU_SGEMM_PARTIAL_FLOATS * sizeof(float)));
    int rc = arreau_sgemm(s, partial, M, N, K, d_A, (long)as0, (long)as1, d_B, (long)bs0, (long)bs1, d_C, ldc, alpha, beta, 1, 0, 0, 0, mode);
    const hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(partial);
    if (rc == ARREAU_OK && e != hipSuccess) {
        arreau_set_error(std::string("arreau_debug_sgemm: ") + hipGetErrorString(e));
        rc = ARREAU_EHIP;
    }
    return rc;
}
