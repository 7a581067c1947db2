// arreau_predict_scores: one evaluation of the score network on the current sampler state, plus the
// workspace carve-up and the hipEvent timing hook for the dominant (edge) kernel.
#include <mutex>
#include <vector>

#include "internal.h"

namespace {
struct Carver {
    char* base;
    size_t off = 0, cap;
    Carver(void* p, size_t c) : base((char*)p), cap(c) {}
    template <typename T>
    T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* r = (T*)(base ? base + off : nullptr);
        off += n * sizeof(T);
        return r;
    }
};

struct Workspace {
    float *lattice, *cart, *cvec, *dir, *dist, *kbuf, *xa, *xb, *xc, *xbar, *vsum, *gs;
    float *eps, *logits, *len0;  // network outputs of the sampling loop (arreau_sample_loop)
    int32_t *batch, *deg, *src, *cell, *t_next, *t_cur;
    int32_t* pass;  // the resampled loop's pass index (arreau_sample_loop_resampled)
    size_t bytes;
};

Workspace carve(const arreau_config* cfg, int64_t N, int64_t B, void* base, size_t cap) {
    Carver c(base, cap);
    Workspace w;
    const size_t C = cfg->hidden_dim, L = cfg->num_layers, k = cfg->max_neighbors, O = cfg->num_ori;
    w.lattice = c.take<float>(B * 9);
    w.cart = c.take<float>(N * 3);
    w.cvec = c.take<float>(B * C);
    w.batch = c.take<int32_t>(N);
    w.deg = c.take<int32_t>(N);
    w.src = c.take<int32_t>(N * k);
    w.cell = c.take<int32_t>(N * k);
    w.dir = c.take<float>(N * k * 3);
    w.dist = c.take<float>(N * k);
    w.kbuf = c.take<float>(L * N * k * O * C);
    w.xa = c.take<float>(N * O * C);
    w.xb = c.take<float>(N * O * C);
    w.xc = c.take<float>(N * O * C);
    w.xbar = c.take<float>(L * N * C);
    w.vsum = c.take<float>(N * O);
    w.gs = c.take<float>(N * 3);
    w.eps = c.take<float>(N * 3);
    w.logits = c.take<float>(N * (size_t)cfg->num_atomic_states);
    w.len0 = c.take<float>(B * 3);
    w.t_next = c.take<int32_t>(B);
    w.t_cur = c.take<int32_t>(B);
    w.pass = c.take<int32_t>(1);
    w.bytes = (c.off + 255) & ~(size_t)255;
    return w;
}

// hipEvent pairs around the edge kernel, on the stream it is launched on
struct EdgeProfile {
    std::mutex mu;
    bool enabled = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
} g_prof;
// the same for the per-layer message kernel of the basis form (conv_proj.hip), the dominant kernel since round 3
EdgeProfile g_prof_conv;
}  // namespace

// called by arreau_launch_conv_proj around its launch (internal.h)
void arreau_prof_conv(int end, hipStream_t s) {
    static thread_local hipEvent_t e0 = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_prof_conv.mu);
        if (!g_prof_conv.enabled) return;
    }
    if (!end) {
        if (hipEventCreate(&e0) != hipSuccess) { e0 = nullptr; return; }
        (void)hipEventRecord(e0, s);
        return;
    }
    if (!e0) return;
    hipEvent_t e1 = nullptr;
    if (hipEventCreate(&e1) == hipSuccess) {
        (void)hipEventRecord(e1, s);
        std::lock_guard<std::mutex> lock(g_prof_conv.mu);
        g_prof_conv.events.emplace_back(e0, e1);
    }
    e0 = nullptr;
}

extern "C" size_t arreau_workspace_bytes(const arreau_config* cfg, int64_t max_atoms, int64_t max_crystals) {
    if (!cfg || max_atoms < 0 || max_crystals < 0) return 0;
    return carve(cfg, max_atoms, max_crystals, nullptr, 0).bytes;
}

extern "C" int arreau_profile_edge_kernel(int32_t enable) {
    for (EdgeProfile* p : {&g_prof, &g_prof_conv}) {
        std::lock_guard<std::mutex> lock(p->mu);
        for (auto& ev : p->events) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        p->events.clear();
        p->enabled = enable != 0;
    }
    return ARREAU_OK;
}

extern "C" int arreau_conv_kernel_time_ms(double* mean_ms, int64_t* launches) {
    ARREAU_REQUIRE(mean_ms && launches, "arreau_conv_kernel_time_ms: null pointer");
    std::lock_guard<std::mutex> lock(g_prof_conv.mu);
    double tot = 0.0;
    int64_t n = 0;
    for (auto& ev : g_prof_conv.events) {
        ARREAU_CHECK_HIP(hipEventSynchronize(ev.second));
        float ms = 0.f;
        ARREAU_CHECK_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
        tot += ms;
        ++n;
    }
    *mean_ms = n ? tot / (double)n : 0.0;
    *launches = n;
    return ARREAU_OK;
}

extern "C" int arreau_edge_kernel_time_ms(double* mean_ms, int64_t* launches) {
    ARREAU_REQUIRE(mean_ms && launches, "arreau_edge_kernel_time_ms: null pointer");
    std::lock_guard<std::mutex> lock(g_prof.mu);
    double tot = 0.0;
    int64_t n = 0;
    for (auto& ev : g_prof.events) {
        ARREAU_CHECK_HIP(hipEventSynchronize(ev.second));
        float ms = 0.f;
        ARREAU_CHECK_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
        tot += ms;
        ++n;
    }
    *mean_ms = n ? tot / (double)n : 0.0;
    *launches = n;
    return ARREAU_OK;
}

namespace {
// the edge kernel, bracketed by hipEvents on its own stream when bench.py asked for its launch time
int run_edge_kernel(const arreau_model* m, const ScorePlan& plan, const float* dir, const float* dist, const int32_t* deg, const Workspace& w,
                    int N, hipStream_t s) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool prof = false;
    {
        std::lock_guard<std::mutex> lock(g_prof.mu);
        prof = g_prof.enabled;
    }
    if (prof) {
        ARREAU_CHECK_HIP(hipEventCreate(&e0));
        ARREAU_CHECK_HIP(hipEventCreate(&e1));
        ARREAU_CHECK_HIP(hipEventRecord(e0, s));
    }
    const int rc = arreau_launch_edge(m, plan, dir, dist, deg, w.batch, w.lattice, N, w.kbuf, s);
    if (prof) {
        ARREAU_CHECK_HIP(hipEventRecord(e1, s));
        std::lock_guard<std::mutex> lock(g_prof.mu);
        g_prof.events.emplace_back(e0, e1);
    }
    return rc;
}

// The neighbour list an evaluation builds or is given, and where its three outputs go.
struct EdgeList { int32_t *deg, *src; float *dir, *dist; };
struct ScoreOutputs { float *eps, *logits, *len0; };

// interaction layers (conv.py:105-129 + convnext.py:20-33) on the embedded features in w.xa, then the read-outs.  Every evaluation
// on the fused kernels ends here: the one place that records its plan.
int run_layers_and_readout(const arreau_model* m, const ScorePlan& plan, const Workspace& w, const int32_t* deg, const int32_t* src,
                           const int32_t* d_off, int B, int N, const ScoreOutputs& out, hipStream_t s) {
    int rc;
    if (N > 0) m->ran = plan;
    float* xin = w.xa;
    float* xout = w.xb;
    for (int l = 0; l < m->L; ++l) {
        if ((rc = arreau_launch_node_layer(m, plan, l, w.kbuf, deg, src, xin, w.xc, xout, w.xbar, w.vsum, N, s))) return rc;
        float* tmp = xin; xin = xout; xout = tmp;
    }
    return arreau_launch_readout(m, plan.readout, w.xbar, w.vsum, d_off, B, N, w.gs, out.eps, out.logits, out.len0, s);
}

// The score network after prep_kernel: neighbour list (unless given), edge kernel, embedding, interaction layers,
// read-outs, for the whole batch on `s`.
int run_network(const arreau_model* m, const ScorePlan& plan, const Workspace& w, bool given, const EdgeList& e, const float* d_frac,
                const int32_t* d_types, const int32_t* d_off, int B, int N, const ScoreOutputs& out, hipStream_t s) {
    const auto [deg, src, dir, dist] = e;
    int rc;
    if (plan.general) {
        // shape-general fp32 kernels (train_net.hip): any hidden_dim / basis_dim / widening, plain weights (never stale)
        arreau_model* mm = const_cast<arreau_model*>(m);  // the activation buffers are a cache owned by the model
        if (!given && (rc = arreau_launch_neighbor(w.cart, w.lattice, d_off, w.batch, B, N, m->cfg.radius, m->k, deg, src, w.cell, dir, dist, s)))
            return rc;
        float* x0 = arreau_general_x0(mm, N, B, s);
        if (!x0) return ARREAU_EHIP;
        if ((rc = arreau_launch_embed(m, d_frac, d_types, w.lattice, w.batch, w.cvec, N, x0, s))) return rc;
        return arreau_general_network(mm, arreau_graph_view{w.batch, deg, src, w.lattice, dir, dist}, d_off, B, N, out.eps, out.logits,
                                      out.len0, s);
    }
    if (!given) {
        // neighbour list and embedding side by side in one launch (both need prep_kernel's outputs only)
        if ((rc = arreau_launch_neighbor_embed(m, w.cart, w.lattice, d_off, w.batch, B, N, deg, src, w.cell, dir, dist, d_frac, d_types,
                                               w.cvec, w.xa, s)))
            return rc;
        if ((rc = run_edge_kernel(m, plan, dir, dist, deg, w, N, s))) return rc;
    } else {
        if ((rc = run_edge_kernel(m, plan, dir, dist, deg, w, N, s))) return rc;
        if ((rc = arreau_launch_embed(m, d_frac, d_types, w.lattice, w.batch, w.cvec, N, w.xa, s))) return rc;
    }
    return run_layers_and_readout(m, plan, w, deg, src, d_off, B, N, out, s);
}
}  // namespace

extern "C" int arreau_predict_scores(const arreau_model* m, const float* d_frac, const int32_t* d_types,
                                     const float* d_lengths, const float* d_angles, const int32_t* d_t,
                                     const int32_t* d_off, int32_t B, int32_t N, int32_t use_given_edges,
                                     int32_t* d_deg, int32_t* d_src, float* d_dir, float* d_dist, float* d_eps,
                                     float* d_logits, float* d_len0, void* d_workspace, size_t workspace_bytes,
                                     void* stream) {
    ARREAU_REQUIRE(m && d_frac && d_types && d_lengths && d_angles && d_t && d_off && d_eps && d_logits && d_len0,
                   "arreau_predict_scores: null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, "arreau_predict_scores: bad size");
    const ScorePlan plan = arreau_score_plan(m, N);
    ARREAU_REQUIRE(!m->packed_stale || plan.general,
                   "arreau_predict_scores: weights were updated for training only (arreau_model_update_train_weights); "
                   "re-create the model before sampling, or select the general path (arreau_model_set_variant(model, 5, -1))");
    ARREAU_REQUIRE(d_workspace != nullptr, "arreau_predict_scores: null workspace");
    Workspace w = carve(&m->cfg, N, B, d_workspace, workspace_bytes);
    if (w.bytes > workspace_bytes) {
        arreau_set_error("arreau_predict_scores: workspace too small");
        return ARREAU_ECAPACITY;
    }
    if (use_given_edges) {
        ARREAU_REQUIRE(d_deg && d_src && d_dir && d_dist, "arreau_predict_scores: teacher-forced edges missing");
    }
    const EdgeList e{d_deg ? d_deg : w.deg, d_src ? d_src : w.src, d_dir ? d_dir : w.dir, d_dist ? d_dist : w.dist};
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = arreau_launch_prep(m, d_frac, d_lengths, d_angles, d_t, d_off, B, N, w.lattice, w.cart, w.batch, w.cvec, s)))
        return rc;
    return run_network(m, plan, w, use_given_edges != 0, e, d_frac, d_types, d_off, B, N, {d_eps, d_logits, d_len0}, s);
}

// PonitaFiberBundle.forward on the reference's own batch attributes (the inner operator seam).
extern "C" int arreau_ponita_forward(const arreau_model* m, const float* d_x, const float* d_vec, const float* d_lattice,
                                     const int32_t* d_off, int32_t B, int32_t N, const int32_t* d_deg,
                                     const int32_t* d_src, const float* d_dir, const float* d_dist, float* d_logits,
                                     float* d_vec_out, float* d_global_scalar, void* d_workspace,
                                     size_t workspace_bytes, void* stream) {
    ARREAU_REQUIRE(m && d_x && d_vec && d_lattice && d_off && d_deg && d_src && d_dir && d_dist && d_logits && d_vec_out &&
                       d_global_scalar, "arreau_ponita_forward: null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, "arreau_ponita_forward: bad size");
    const ScorePlan plan = arreau_score_plan(m, N);
    ARREAU_REQUIRE(!m->packed_stale || plan.general,
                   "arreau_ponita_forward: weights were updated for training only; re-create the model or select the general path");
    ARREAU_REQUIRE(d_workspace != nullptr, "arreau_ponita_forward: null workspace");
    Workspace w = carve(&m->cfg, N, B, d_workspace, workspace_bytes);
    if (w.bytes > workspace_bytes) {
        arreau_set_error("arreau_ponita_forward: workspace too small");
        return ARREAU_ECAPACITY;
    }
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = arreau_launch_batch_index(d_off, B, N, w.batch, s))) return rc;
    w.lattice = const_cast<float*>(d_lattice);  // the edge kernel reads the caller's cells (cos features, invariants.py:82-85)
    if (plan.general) {
        arreau_model* mm = const_cast<arreau_model*>(m);
        float* x0 = arreau_general_x0(mm, N, B, s);
        if (!x0) return ARREAU_EHIP;
        if ((rc = arreau_launch_embed_general(m, d_x, d_vec, N, x0, s))) return rc;
        return arreau_general_network(mm, arreau_graph_view{w.batch, d_deg, d_src, d_lattice, d_dir, d_dist}, d_off, B, N,
                                      d_vec_out, d_logits, d_global_scalar, s);
    }
    if ((rc = run_edge_kernel(m, plan, d_dir, d_dist, d_deg, w, N, s))) return rc;
    if ((rc = arreau_launch_embed_general(m, d_x, d_vec, N, w.xa, s))) return rc;
    return run_layers_and_readout(m, plan, w, d_deg, d_src, d_off, B, N, {d_vec_out, d_logits, d_global_scalar}, s);
}

// ---------------------------------------------------------------------------------------------
// The hot loop of DiffusionLoss.sample (diffusion/diffusion_loss.py:318-347), enqueued in one call.
// ---------------------------------------------------------------------------------------------
namespace {
__global__ void fill_i32_kernel(int32_t* __restrict__ p, int32_t v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// The single-stream product loop runs WITHOUT a prep launch per step (plan.no_prep; round 3) when it can: the update launch of
// step i leaves the lattice and the per-crystal embedding of step i + 1 behind (reverse_crystal_block), the neighbour-list waves
// form the Cartesian positions themselves and advance the device-side timestep (neighbor_embed_kernel<LOOP>), and ONE prep launch
// in front of the loop (arreau_sample_loop) supplies the first step.  With a prep launch in every step (A/B, tests) the loop is
// bit-identical.
//
// Predictor-corrector sampling (arreau_sample_loop_corrected, opt.corr): only the first evaluation of a step advances the device
// timestep; the later ones rebuild the neighbour list and the per-atom embedding from the moved positions at the same timestep.
// The lattice and the per-crystal embedding stay valid: a corrector moves fractional coordinates only.
int enqueue_sample_step(const arreau_model* m, const ScorePlan& plan, const SampleState& st, const Workspace& w, hipStream_t s,
                        uint64_t seed, const StepOptions& opt) {
    int rc;
    const int32_t* next_t = opt.sched ? opt.sched->next : nullptr;  // respaced loop: the device timestep follows the table
    // fused kernels: the per-crystal pooling of the lattice read-out happens inside the lattice update (no launch of its own)
    const bool pool_in_update = !plan.general;
    for (int j = 0; j <= opt.corr.steps; ++j) {
        if (plan.no_prep) {
            if ((rc = arreau_launch_neighbor_embed(m, nullptr, w.lattice, st.offsets, w.batch, st.B, st.N, w.deg, w.src, w.cell, w.dir, w.dist,
                                                   st.frac, st.types, w.cvec, w.xa, s, w.t_cur, next_t, /*advance=*/j == 0)))
                return rc;
            if ((rc = run_edge_kernel(m, plan, w.dir, w.dist, w.deg, w, st.N, s))) return rc;
            if ((rc = run_layers_and_readout(m, plan, w, w.deg, w.src, st.offsets, st.B, st.N, {w.eps, w.logits, nullptr}, s))) return rc;
        } else {
            // the first set-up of the step advances the device timestep; a corrector's re-evaluation reads it (t_cur)
            if ((rc = j == 0 ? arreau_launch_prep(m, st.frac, st.lengths, st.angles, nullptr, st.offsets, st.B, st.N, w.lattice, w.cart, w.batch,
                                                  w.cvec, s, w.t_next, w.t_cur, 0, next_t)
                             : arreau_launch_prep(m, st.frac, st.lengths, st.angles, w.t_cur, st.offsets, st.B, st.N, w.lattice, w.cart, w.batch,
                                                  w.cvec, s)))
                return rc;
            if ((rc = run_network(m, plan, w, false, {w.deg, w.src, w.dir, w.dist}, st.frac, st.types, st.offsets, st.B, st.N,
                                  {w.eps, w.logits, pool_in_update ? nullptr : w.len0}, s)))
                return rc;
        }
        // contact guidance: the eps of this evaluation, guided in place, is what the corrector and the predictor below read
        if (opt.guide && (rc = arreau_launch_contact_guide(m, st, w.t_cur, w.lattice, w.eps, *opt.guide, s))) return rc;
        if (opt.xrd_guide && (rc = arreau_launch_xrd_guide(m, st, w.t_cur, w.lattice, w.eps, *opt.xrd_guide, nullptr, s))) return rc;
        if (j < opt.corr.steps && (rc = arreau_launch_corrector(m, st, w.t_cur, w.eps, nullptr, seed, (uint32_t)j, opt, s))) return rc;
    }
    // without a prep launch per step (fused kernels only) the update also leaves the next step's lattice and embedding behind
    ReverseInputs in{w.t_cur, w.eps, w.logits, w.len0, StepNoiseSrc{.seed = seed, .seeds = opt.crystal_seeds}, pool_in_update ? w.gs : nullptr,
                     w.batch};
    if (plan.no_prep) {
        in.lattice_ws = w.lattice;
        in.cvec_next = w.cvec;
    }
    return arreau_launch_reverse(m, st, in, opt, s);
}

// RePaint resampling (arreau_sample_loop_resampled): the blocks of one loop call, from the host's list of the steps it visits.
// Block k runs steps first .. first + count - 1 (indices into the visited list), R times; passes 1..R-1 start with the jump
// bottom -> top.
struct ResampleBlock { int first, count, top, bottom; };

// What an arreau_sample_loop* export (or arreau_invert_loop) was called with besides the model and the state.  The export fills it
// with designated initialisers: an option it does not take stays null.
struct LoopRequest {
    int32_t t_start = 0, n_steps = 0;
    uint64_t seed = 0;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    int32_t use_graph = 0;
    void* stream = nullptr;
    const arreau_sample_condition* condition = nullptr;
    const arreau_sample_schedule* schedule = nullptr;  // of an inversion loop: the ascending table
    const arreau_corrector* corrector = nullptr;
    const arreau_resampling* resampling = nullptr;
    const int32_t* d_length_tie = nullptr;
    const arreau_symmetry* symmetry = nullptr;
    const float* eta = nullptr;
    const arreau_multistep* multistep = nullptr;
    const arreau_species_control* species = nullptr;
    bool species_required = false;  // arreau_sample_loop_species and the exports built on it (their multistep rules have their own wording)
    const uint64_t* d_crystal_seeds = nullptr;
    const arreau_contact_guidance* guidance = nullptr;
    const arreau_xrd_guidance* xrd_guidance = nullptr;
    bool invert = false;  // arreau_invert_loop: t_start is the first level
};

// A request that passed resolve_loop_request: what the loop runs on.
struct LoopCall {
    ScorePlan score;  // of every evaluation of the call
    Workspace w;
    SampleOptions opt;
    std::vector<ResampleBlock> blocks;  // of a resampled loop (opt.resample_passes > 1)
};

// The blocks of a resampled loop: the visited steps t_1 .. t_n and the successor of t_n, from the host copy of the schedule (or
// t - 1 without one), cut every `jump` steps.
int resample_blocks(const char* who, const LoopRequest& req, const arreau_resampling* resampling, int jump,
                    std::vector<ResampleBlock>* blocks) {
    const int n_steps = req.n_steps, t_start = req.t_start;
    std::vector<int> steps;
    int last_succ = 0;
    if (req.schedule) {
        ARREAU_REQUIRE(resampling->timesteps != nullptr && resampling->n_timesteps >= 1,
                       std::string(who) + ": a respaced loop needs the host copy of its schedule (timesteps)");
        const int32_t* ts = resampling->timesteps;
        const int K = resampling->n_timesteps;
        int i0 = -1;
        for (int i = 0; i < K; ++i)
            if (ts[i] == t_start) { i0 = i; break; }
        ARREAU_REQUIRE(i0 >= 0 && (int64_t)i0 + n_steps <= K,
                       std::string(who) + ": the host schedule does not hold t_start followed by n_steps - 1 timesteps");
        steps.assign(ts + i0, ts + i0 + n_steps);
        last_succ = i0 + n_steps < K ? ts[i0 + n_steps] : 0;
    } else {
        for (int i = 0; i < n_steps; ++i) steps.push_back(t_start - i);
        last_succ = t_start - n_steps;
    }
    for (int a = 0; a < n_steps; a += jump) {
        const int cnt = n_steps - a < jump ? n_steps - a : jump;
        blocks->push_back(ResampleBlock{a, cnt, steps[a], a + cnt < n_steps ? steps[a + cnt] : last_succ});
    }
    return ARREAU_OK;
}

// The one place the rules of the options are applied (they are stated in include/arreau_hip.h): every check of a loop call, and
// what the accepted call runs on in *c.  The order is part of the interface -- the first failing check is the one reported
// (DESIGN.md lists it) --, and so are the messages, also where one names another export than `who`.  arreau_launch_reverse guards
// the combinations once more for the step exports, which reach it directly.
int resolve_loop_request(const char* who, const arreau_model* m, const SampleState& st, const LoopRequest& req, LoopCall* c) {
    const std::string name(who);
    SampleOptions& o = c->opt = SampleOptions{};
    const arreau_sample_condition* condition = req.condition;
    const arreau_corrector* corrector = req.corrector;
    const arreau_resampling* resampling = req.resampling;
    int rc;
    if (req.guidance && (rc = arreau_contact_guidance_check(req.guidance, who))) return rc;
    if (req.xrd_guidance && (rc = arreau_xrd_guidance_check(req.xrd_guidance, who, false))) return rc;
    if (req.species_required && (rc = arreau_species_check(req.species, who, &o.species))) return rc;  // (-0 -> +0)
    o.species_on = req.species_required;
    if (req.eta && (rc = arreau_eta_check(*req.eta, who))) return rc;
    ARREAU_REQUIRE(!req.symmetry || !req.eta, name + ": space-group symmetry is not combined with an eta");
    if (req.symmetry) {
        if ((rc = arreau_symmetry_check(req.symmetry, who))) return rc;
        ARREAU_REQUIRE(!resampling || resampling->passes <= 1, name + ": space-group symmetry is not combined with resampling (passes > 1)");
    }
    if (req.multistep) {
        // a multistep loop is the eta = 0 loop on the caller's history buffers; a schedule, a tie, species control, keys and guidance only
        const std::string ms = name + (req.species_required ? ": multistep is not combined with " : ": not combined with ");
        if ((rc = arreau_multistep_check(req.multistep, who))) return rc;
        if ((rc = arreau_condition_to_dev(condition, &o.cond))) return rc;
        ARREAU_REQUIRE(arreau_condition_empty(&o.cond), ms + "a condition");
        ARREAU_REQUIRE(!corrector || corrector->steps == 0, ms + "corrector steps");
        ARREAU_REQUIRE(!resampling || resampling->passes == 1, ms + "resampling (passes > 1)");
        ARREAU_REQUIRE(!req.symmetry, ms + "space-group symmetry");
        ARREAU_REQUIRE(!req.eta || *req.eta == 0.0f, name + ": a multistep loop is the eta = 0 loop");
        condition = nullptr; corrector = nullptr; resampling = nullptr;  // what they still hold is the loop without them: not read
    }
    o.eta = req.multistep ? 0.0f : (req.eta ? *req.eta + 0.0f /* -0 -> +0 */ : -1.0f);
    if (resampling) {
        if ((rc = arreau_resampling_check(resampling->passes, resampling->jump_length, who))) return rc;
        if (resampling->passes > 1) {
            o.resample_passes = resampling->passes;
            o.resample_jump = resampling->jump_length;
            if (req.n_steps > 0 && (rc = resample_blocks(who, req, resampling, o.resample_jump, &c->blocks))) return rc;
        }
    }
    ARREAU_REQUIRE(!req.invert || !req.guidance, "arreau_invert_loop: an inversion loop takes no contact guidance");
    ARREAU_REQUIRE(!req.invert || !req.xrd_guidance, "arreau_invert_loop: an inversion loop takes no xrd guidance");
    if (corrector) {
        if ((rc = arreau_corrector_check(corrector->steps, corrector->snr, "arreau_sample_loop_corrected"))) return rc;
        // a NULL corrector and steps == 0 are the same loop (and the same graph key): the snr is then not read
        if (corrector->steps > 0) o.corr = CorrectorDev{corrector->steps, corrector->snr};
    }
    ARREAU_REQUIRE(m && st.frac && st.types && st.lengths && st.angles && st.offsets && st.lattice, "arreau_sample_loop: null pointer");
    ARREAU_REQUIRE(st.B >= 1 && st.N >= 0 && req.n_steps >= 0, "arreau_sample_loop: bad size");
    c->score = arreau_score_plan(m, st.N);
    ARREAU_REQUIRE(!m->packed_stale || c->score.general,
                   "arreau_sample_loop: weights were updated for training only; re-create the model or select the general path");
    if (req.schedule) {
        ARREAU_REQUIRE(req.schedule->d_next != nullptr, "arreau_sample_loop_scheduled: null next-timestep table");
        ARREAU_REQUIRE(req.schedule->lattice_clipmax > 0.0f && req.schedule->lattice_clipmax <= 1.0f,
                       "arreau_sample_loop_scheduled: lattice_clipmax must lie in (0, 1]");
        // the loop starts one above t_start (d_next[t_start + 1] == t_start, include/arreau_hip.h), so t_start + 1 <= T
        ARREAU_REQUIRE(req.n_steps == 0 || (req.t_start >= 1 && req.t_start <= m->T - 1), "arreau_sample_loop_scheduled: t_start must lie in 1..T-1");
        o.sched = StepScheduleDev{req.schedule->d_next, nullptr, req.schedule->lattice_clipmax};
    } else {
        ARREAU_REQUIRE(req.t_start <= m->T && req.t_start - req.n_steps >= 0,
                       "arreau_sample_loop: timesteps t_start .. t_start-n_steps+1 must lie in 1..T");
    }
    ARREAU_REQUIRE(req.workspace != nullptr, "arreau_sample_loop: null workspace");
    c->w = carve(&m->cfg, st.N, st.B, req.workspace, req.workspace_bytes);
    if (c->w.bytes > req.workspace_bytes) {
        arreau_set_error("arreau_sample_loop: workspace too small");
        return ARREAU_ECAPACITY;
    }
    if ((rc = arreau_condition_to_dev(condition, &o.cond))) return rc;  // (without a mask: all null, the unconditioned loop)
    o.pass = o.resample_passes > 1 ? c->w.pass : nullptr;
    o.length_tie = req.d_length_tie;
    if (req.symmetry) o.sym = *req.symmetry;
    if (req.multistep) o.ms = *req.multistep;
    o.invert = req.invert;
    o.crystal_seeds = req.d_crystal_seeds;
    if (req.guidance && req.guidance->weight > 0.0f) o.guide = *req.guidance;  // weight 0: the loop without the option (and its graph key)
    if (req.xrd_guidance && req.xrd_guidance->weight > 0.0f) o.xrd_guide = *req.xrd_guidance;  // (the same)
    const bool plain = arreau_condition_empty(&o.cond) && o.corr.steps == 0 && o.resample_passes == 0;
    ARREAU_REQUIRE(!req.multistep || (plain && !req.symmetry && !req.invert && o.eta == 0.0f),
                   "arreau_sample_loop_multistep: a multistep loop takes no condition, corrector steps, resampling or symmetry");
    ARREAU_REQUIRE(!req.invert || (plain && req.schedule && !req.d_length_tie && !req.symmetry && o.eta < 0.0f),
                   "arreau_invert_loop: an inversion loop takes its ascending table and no sampling option");
    // (read for n_steps > 0 only: an empty loop with these options is accepted)
    ARREAU_REQUIRE(req.n_steps == 0 || !req.symmetry || plain,
                   "arreau_sample_loop_sym: space-group symmetry is not combined with a condition, corrector steps or resampling");
    return ARREAU_OK;
}

// What every arreau_sample_loop* export and arreau_invert_loop run, `who` being the export: the checks, then the loop.
int run_sample_loop(const char* who, arreau_model* m, const SampleState& st, const LoopRequest& req) {
    LoopCall c;
    int rc;
    if ((rc = resolve_loop_request(who, m, st, req, &c))) return rc;
    if (req.n_steps == 0) return ARREAU_OK;
    const int B = st.B, N = st.N, t_start = req.t_start, n_steps = req.n_steps;
    const uint64_t seed = req.seed;
    const ScorePlan& score = c.score;  // of every evaluation of this call
    const Workspace& w = c.w;
    const StepOptions opt = c.opt.view();  // the options of every step of this call
    const bool resampled = c.opt.resample_passes > 1;
    hipStream_t s = (hipStream_t)req.stream;
    if (score.no_prep) {
        // t_cur holds the timestep of the step in progress; every step's first launch advances it, so it starts one above (in a
        // respaced loop at the table entry t_start + 1, whose successor is t_start) -- an inversion loop, which climbs, one below
        // (the ascending table's entry t_start - 1, whose successor is t_start)
        const int before = opt.invert ? -1 : 1;
        ARREAU_LAUNCH(fill_i32_kernel, dim3((B + 255) / 256), dim3(256), 0, s, w.t_cur, t_start + before, B);
        ARREAU_CHECK_HIP(hipGetLastError());
        if ((rc = arreau_launch_prep(m, st.frac, st.lengths, st.angles, w.t_cur, st.offsets, B, N, w.lattice, w.cart, w.batch, w.cvec, s,
                                     nullptr, nullptr, -before)))
            return rc;
    } else {
        ARREAU_LAUNCH(fill_i32_kernel, dim3((B + 255) / 256), dim3(256), 0, s, w.t_next, t_start, B);
        ARREAU_CHECK_HIP(hipGetLastError());
    }
    // steps run (every pass of every block counts)
    int64_t n_runs = n_steps;
    if (resampled) {
        n_runs = 0;
        for (const ResampleBlock& bl : c.blocks) n_runs += (int64_t)c.opt.resample_passes * bl.count;
    }
    const bool graph_mode = req.use_graph && n_runs >= 3;
    hipStream_t user = s;
    hipEvent_t ev = nullptr;
    SampleGraphKey key{};
    hipGraphExec_t exec = nullptr;
    bool have_exec = false;
    if (graph_mode) {
        // One step captured into a hipGraph and replayed: the timestep lives on the device (prep_kernel advances it), the noise
        // is a function of (seed, timestep, element) -- and in a resampled loop of the pass index, another device word -- so every
        // replay is the next step of the same trajectory as the eager loop.
        // Capture is not allowed on the legacy default stream (which is what callers usually pass), so the loop runs on a
        // stream of the model's own, joined to the caller's stream by events on both sides: still no host synchronisation.
        if (!m->loop_stream) {
            hipStream_t ls = nullptr;
            ARREAU_CHECK_HIP(hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
            hipEvent_t e0 = nullptr;
            ARREAU_CHECK_HIP(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
            m->loop_stream = (void*)ls;
            m->loop_event = (void*)e0;
        }
        ev = (hipEvent_t)m->loop_event;
        s = (hipStream_t)m->loop_stream;
        ARREAU_CHECK_HIP(hipEventRecord(ev, user));
        ARREAU_CHECK_HIP(hipStreamWaitEvent(s, ev, 0));
        // The executable graph is kept with the model and reused while the next call names the same buffers, sizes, seed, plan and
        // options (a sampler drawing sub-batch after sub-batch through the caching allocator does): capture + instantiation, about
        // 2 ms, are then paid once.  The timestep is not part of the graph (it lives in t_next / t_cur, set above).
        key = SampleGraphKey{st, req.workspace, seed, score, c.opt};
        exec = (hipGraphExec_t)m->retired_graph;
        have_exec = exec && key == m->graph_key;
    }
    // one step of the trajectory: eager, or (graph mode) the first one eager and captured behind it, then replays
    auto run_step = [&]() -> int {
        int r;
        if (!graph_mode || !have_exec) {
            // (eager: the first step of a capture also forces lazy module loading, which must not happen inside a capture)
            if ((r = enqueue_sample_step(m, score, st, w, s, seed, opt))) return r;
            if (!graph_mode) return ARREAU_OK;
            hipGraph_t graph = nullptr;
            ARREAU_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            r = enqueue_sample_step(m, score, st, w, s, seed, opt);
            hipError_t e = hipStreamEndCapture(s, &graph);
            if (r) {
                if (graph) (void)hipGraphDestroy(graph);
                return r;
            }
            ARREAU_CHECK_HIP(e);
            exec = nullptr;
            e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            ARREAU_CHECK_HIP(e);
            arreau_model_retire_graph(m, (void*)exec, (void*)s);  // takes ownership; frees the previous one after its stream drained
            m->graph_key = key;
            have_exec = true;
            return ARREAU_OK;
        }
        ARREAU_CHECK_HIP(hipGraphLaunch(exec, s));
        return ARREAU_OK;
    };
    if (!resampled) {
        for (int i = 0; i < n_steps; ++i)
            if ((rc = run_step())) return rc;
    } else {
        // every block runs R passes; pass r >= 1 starts with the jump bottom -> top, which also sets the device timestep to the
        // top, prepares the next step for it and sets the pass word to r; the word goes back to 0 after the block
        const JumpLoopDev loop{w.lattice, w.cvec, w.t_next, w.t_cur, w.pass};
        ARREAU_LAUNCH(fill_i32_kernel, dim3(1), dim3(256), 0, s, w.pass, 0, 1);
        ARREAU_CHECK_HIP(hipGetLastError());
        for (const ResampleBlock& bl : c.blocks) {
            for (int r = 0; r < c.opt.resample_passes; ++r) {
                if (r > 0 && (rc = arreau_launch_resample_jump(m, st, /*d_s=*/nullptr, /*d_t=*/nullptr, bl.bottom, bl.top, w.batch,
                                                               StepNoiseSrc{.seed = seed, .seeds = opt.crystal_seeds}, (uint32_t)r, opt.cond, &loop,
                                                               opt.length_tie, s)))
                    return rc;
                for (int i = 0; i < bl.count; ++i)
                    if ((rc = run_step())) return rc;
            }
            ARREAU_LAUNCH(fill_i32_kernel, dim3(1), dim3(256), 0, s, w.pass, 0, 1);
            ARREAU_CHECK_HIP(hipGetLastError());
        }
    }
    if (!graph_mode) return ARREAU_OK;
    ARREAU_CHECK_HIP(hipEventRecord(ev, s));
    ARREAU_CHECK_HIP(hipStreamWaitEvent(user, ev, 0));  // the caller's stream continues after the loop
    return ARREAU_OK;
}
}  // namespace

// The exports: each is a fill of the state and of a LoopRequest with what it takes, and one call of run_sample_loop under its own
// name.  The first six are each the one before plus one option (NULL: the loop without it); _eta, _multistep and _sym are the tied
// one plus theirs; _species takes all of those, _keyed, _guided and _xrd_guided one more each.  The rules of the options are stated in
// include/arreau_hip.h and applied by resolve_loop_request.
extern "C" int arreau_sample_loop(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                  const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                  const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice, void* d_workspace,
                                  size_t workspace_bytes, int32_t use_graph, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream});
}

extern "C" int arreau_sample_loop_conditioned(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                              const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                              const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                              void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                              const arreau_sample_condition* condition, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_conditioned", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition});
}

extern "C" int arreau_sample_loop_scheduled(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                            const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                            const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                            void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                            const arreau_sample_condition* condition, const arreau_sample_schedule* schedule, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_scheduled", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule});
}

extern "C" int arreau_sample_loop_corrected(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                            const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                            const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                            void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                            const arreau_sample_condition* condition, const arreau_sample_schedule* schedule,
                                            const arreau_corrector* corrector, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_corrected", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector});
}

extern "C" int arreau_sample_loop_resampled(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                            const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                            const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                            void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                            const arreau_sample_condition* condition, const arreau_sample_schedule* schedule,
                                            const arreau_corrector* corrector, const arreau_resampling* resampling, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_resampled", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling});
}

extern "C" int arreau_sample_loop_tied(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                       const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                       const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice, void* d_workspace,
                                       size_t workspace_bytes, int32_t use_graph, const arreau_sample_condition* condition,
                                       const arreau_sample_schedule* schedule, const arreau_corrector* corrector,
                                       const arreau_resampling* resampling, const int32_t* d_length_tie, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_tied", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie});
}

extern "C" int arreau_sample_loop_eta(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                      const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                      const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice, void* d_workspace,
                                      size_t workspace_bytes, int32_t use_graph, const arreau_sample_condition* condition,
                                      const arreau_sample_schedule* schedule, const arreau_corrector* corrector,
                                      const arreau_resampling* resampling, const int32_t* d_length_tie, float eta, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_eta", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie, .eta = &eta});
}

// Second-order multistep sampling: the eta = 0 loop whose steps extrapolate with the previous step's prediction, kept in the
// caller's history buffers (required).
extern "C" int arreau_sample_loop_multistep(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                            const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                            const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                            void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                            const arreau_sample_condition* condition, const arreau_sample_schedule* schedule,
                                            const arreau_corrector* corrector, const arreau_resampling* resampling,
                                            const int32_t* d_length_tie, const arreau_multistep* multistep, void* stream) {
    int rc;
    if ((rc = arreau_multistep_check(multistep, "arreau_sample_loop_multistep"))) return rc;  // (required here: NULL is an error)
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_multistep", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie, .multistep = multistep});
}

extern "C" int arreau_sample_loop_sym(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                      const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                      const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice, void* d_workspace,
                                      size_t workspace_bytes, int32_t use_graph, const arreau_sample_condition* condition,
                                      const arreau_sample_schedule* schedule, const arreau_corrector* corrector,
                                      const arreau_resampling* resampling, const int32_t* d_length_tie, const arreau_symmetry* symmetry,
                                      void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_sym", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie, .symmetry = symmetry});
}

// Species control: whichever of the loops above the options name, its steps the SPEC instances; `species` is required.
extern "C" int arreau_sample_loop_species(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                          const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                          const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                          void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                          const arreau_sample_condition* condition, const arreau_sample_schedule* schedule,
                                          const arreau_corrector* corrector, const arreau_resampling* resampling,
                                          const int32_t* d_length_tie, const arreau_symmetry* symmetry, const float* eta,
                                          const arreau_multistep* multistep, const arreau_species_control* species, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_species", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie, .symmetry = symmetry, .eta = eta, .multistep = multistep,
                            .species = species, .species_required = true});
}

// Keyed sampling: arreau_sample_loop_species with the table of stream seeds, which every draw of the loop -- steps, corrector
// moves, jumps -- is keyed by; a NULL table is arreau_sample_loop_species bit for bit.
extern "C" int arreau_sample_loop_keyed(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                        const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                        const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice, void* d_workspace,
                                        size_t workspace_bytes, int32_t use_graph, const arreau_sample_condition* condition,
                                        const arreau_sample_schedule* schedule, const arreau_corrector* corrector,
                                        const arreau_resampling* resampling, const int32_t* d_length_tie, const arreau_symmetry* symmetry,
                                        const float* eta, const arreau_multistep* multistep, const arreau_species_control* species,
                                        const uint64_t* d_crystal_seeds, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_keyed", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie, .symmetry = symmetry, .eta = eta, .multistep = multistep,
                            .species = species, .species_required = true, .d_crystal_seeds = d_crystal_seeds});
}

// Contact guidance: arreau_sample_loop_keyed whose every network evaluation is followed by the guidance launch on its eps; a NULL
// struct or weight == 0 is arreau_sample_loop_keyed bit for bit.
extern "C" int arreau_sample_loop_guided(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                         const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                         const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice, void* d_workspace,
                                         size_t workspace_bytes, int32_t use_graph, const arreau_sample_condition* condition,
                                         const arreau_sample_schedule* schedule, const arreau_corrector* corrector,
                                         const arreau_resampling* resampling, const int32_t* d_length_tie, const arreau_symmetry* symmetry,
                                         const float* eta, const arreau_multistep* multistep, const arreau_species_control* species,
                                         const uint64_t* d_crystal_seeds, const arreau_contact_guidance* guidance, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_guided", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie, .symmetry = symmetry, .eta = eta, .multistep = multistep,
                            .species = species, .species_required = true, .d_crystal_seeds = d_crystal_seeds, .guidance = guidance});
}

// XRD guidance: arreau_sample_loop_guided whose every network evaluation is also followed by the XRD guidance launch on its eps,
// after contact guidance's; a NULL struct or weight == 0 is arreau_sample_loop_guided bit for bit.
extern "C" int arreau_sample_loop_xrd_guided(arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, const float* d_angles,
                                             const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, int32_t n_steps, uint64_t seed,
                                             const int32_t* d_const_types, const float* d_fixed_lengths, float* d_lattice,
                                             void* d_workspace, size_t workspace_bytes, int32_t use_graph,
                                             const arreau_sample_condition* condition, const arreau_sample_schedule* schedule,
                                             const arreau_corrector* corrector, const arreau_resampling* resampling,
                                             const int32_t* d_length_tie, const arreau_symmetry* symmetry, const float* eta,
                                             const arreau_multistep* multistep, const arreau_species_control* species,
                                             const uint64_t* d_crystal_seeds, const arreau_contact_guidance* guidance,
                                             const arreau_xrd_guidance* xrd_guidance, void* stream) {
    const SampleState st{d_frac, d_types, d_lengths, d_angles, d_off, B, N, d_const_types, d_fixed_lengths, d_lattice};
    return run_sample_loop("arreau_sample_loop_xrd_guided", m, st,
                           {.t_start = t_start, .n_steps = n_steps, .seed = seed, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .condition = condition, .schedule = schedule, .corrector = corrector,
                            .resampling = resampling, .d_length_tie = d_length_tie, .symmetry = symmetry, .eta = eta, .multistep = multistep,
                            .species = species, .species_required = true, .d_crystal_seeds = d_crystal_seeds, .guidance = guidance,
                            .xrd_guidance = xrd_guidance});
}

// DDIM inversion: the sampling loop climbing the levels of an ascending table, every step the network evaluation at the crystals'
// level and the INVERT update to the next one.  The same loop code in both forms, with graph replay and on the shape-general
// path; no seed, no corrector, no jump.
extern "C" int arreau_invert_loop(arreau_model* m, float* d_frac, const int32_t* d_types, float* d_lengths, const float* d_angles,
                                  const int32_t* d_off, int32_t B, int32_t N, int32_t t_first, int32_t n_steps, const int32_t* d_up,
                                  const float* d_fixed_lengths, float* d_lattice, void* d_workspace, size_t workspace_bytes,
                                  int32_t use_graph, void* stream) {
    ARREAU_REQUIRE(m && d_up, "arreau_invert_loop: null pointer");
    ARREAU_REQUIRE(n_steps >= 0 && t_first >= 1 && (int64_t)t_first + n_steps <= m->T,
                   "arreau_invert_loop: the levels t_first < ... (n_steps climbs) must lie in 1..T");
    // (the species are read by the network and never written: the pointer only completes the state)
    const SampleState st{d_frac, const_cast<int32_t*>(d_types), d_lengths, d_angles, d_off, B, N, nullptr, d_fixed_lengths, d_lattice};
    const arreau_sample_schedule up{d_up, 1.0f /* not read by an inversion step */};
    return run_sample_loop("arreau_invert_loop", m, st,
                           {.t_start = t_first, .n_steps = n_steps, .workspace = d_workspace, .workspace_bytes = workspace_bytes,
                            .use_graph = use_graph, .stream = stream, .schedule = &up, .invert = true});
}

// ---------------------------------------------------------------------------------------------
// Uninitialised-state probe (internal.h: ARREAU_LAUNCH).  One workgroup per CU takes the CU's whole LDS (160 KiB, so no
// second one fits beside it) and 16 waves x ~112 registers per lane = most of the four SIMDs' register files, writes the
// pattern everywhere and leaves.  The workgroups wait for each other (bounded: a clock limit, so the grid always drains)
// to make sure none of them is placed on a CU another one has already left.
// ---------------------------------------------------------------------------------------------
unsigned arreau_debug_pollution = 0;
namespace {
__global__ __launch_bounds__(1024) void pollute_kernel(unsigned pattern, unsigned* __restrict__ arrived, unsigned target) {
    extern __shared__ unsigned pl[];
    for (int i = threadIdx.x; i < 40960; i += 1024) pl[i] = pattern;
    float r[112];
#pragma unroll
    for (int i = 0; i < 112; ++i) asm volatile("v_mov_b32 %0, %1" : "=v"(r[i]) : "v"(pattern));
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(arrived, 1u);
        const long long t0 = wall_clock64();  // 100 MHz
        while (__hip_atomic_load(arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target && wall_clock64() - t0 < 20000) {}
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 112; ++i) asm volatile("" : : "v"(r[i]));
    if (pl[(threadIdx.x * 37) % 40960] != pattern) arrived[1] = 1;  // (keeps the LDS writes alive; never true)
}
unsigned* g_pollute_counter = nullptr;
unsigned g_pollute_launches = 0;
}  // namespace

int arreau_debug_pollute(hipStream_t s) {
    const int n_cu = arreau_cu_count();
    if (!g_pollute_counter) {
        ARREAU_CHECK_HIP(hipMalloc(&g_pollute_counter, 8));
        ARREAU_CHECK_HIP(hipMemset(g_pollute_counter, 0, 8));
        ARREAU_CHECK_HIP(hipFuncSetAttribute((const void*)pollute_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
    }
    ++g_pollute_launches;
    hipLaunchKernelGGL(pollute_kernel, dim3(n_cu), dim3(1024), 163840, s, arreau_debug_pollution, g_pollute_counter,
                       g_pollute_launches * (unsigned)n_cu);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

// Positive control of the probe: a kernel that READS what it never wrote -- every CU's whole LDS and 32 vector registers
// per lane -- and counts the words equal to `pattern`.  Launched through ARREAU_LAUNCH with the pollution switched on it
// must find (nearly) nothing else; the test asserts that, so a clean probe run means "no dependence on leftovers", not
// "the polluter did not reach them".
namespace {
__global__ __launch_bounds__(1024) void leftover_kernel(unsigned pattern, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned pl[];
    unsigned lds_hits = 0, reg_hits = 0;
    for (int i = threadIdx.x; i < 40960; i += 1024) lds_hits += pl[i] == pattern;
    asm volatile("" ::: "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109",
                 "v110", "v111");  // make the registers read below part of this wave's allocation
#define ARREAU_LEFTOVER_REG(n) { unsigned x; asm volatile("v_mov_b32 %0, v" #n : "=v"(x)); reg_hits += x == pattern; }
    ARREAU_LEFTOVER_REG(96) ARREAU_LEFTOVER_REG(97) ARREAU_LEFTOVER_REG(98) ARREAU_LEFTOVER_REG(99)
    ARREAU_LEFTOVER_REG(100) ARREAU_LEFTOVER_REG(101) ARREAU_LEFTOVER_REG(102) ARREAU_LEFTOVER_REG(103)
    ARREAU_LEFTOVER_REG(104) ARREAU_LEFTOVER_REG(105) ARREAU_LEFTOVER_REG(106) ARREAU_LEFTOVER_REG(107)
    ARREAU_LEFTOVER_REG(108) ARREAU_LEFTOVER_REG(109) ARREAU_LEFTOVER_REG(110) ARREAU_LEFTOVER_REG(111)
#undef ARREAU_LEFTOVER_REG
    atomicAdd(&counts[0], (unsigned long long)lds_hits);
    atomicAdd(&counts[1], (unsigned long long)reg_hits);
}
}  // namespace

extern "C" int arreau_debug_leftover_fraction(uint32_t pattern, double* lds_fraction, double* reg_fraction, void* stream) {
    ARREAU_REQUIRE(lds_fraction && reg_fraction, "arreau_debug_leftover_fraction: null pointer");
    const int n_cu = arreau_cu_count();
    unsigned long long* d_counts = nullptr;
    ARREAU_CHECK_HIP(hipMalloc(&d_counts, 16));
    hipStream_t s = (hipStream_t)stream;
    ARREAU_CHECK_HIP(hipMemsetAsync(d_counts, 0, 16, s));
    ARREAU_CHECK_HIP(hipFuncSetAttribute((const void*)leftover_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
    ARREAU_LAUNCH(leftover_kernel, dim3(n_cu), dim3(1024), 163840, s, pattern, d_counts);
    ARREAU_CHECK_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    ARREAU_CHECK_HIP(hipMemcpyAsync(h, d_counts, 16, hipMemcpyDeviceToHost, s));
    ARREAU_CHECK_HIP(hipStreamSynchronize(s));
    ARREAU_CHECK_HIP(hipFree(d_counts));
    *lds_fraction = (double)h[0] / ((double)n_cu * 40960.0);
    *reg_fraction = (double)h[1] / ((double)n_cu * 1024.0 * 16.0);
    return ARREAU_OK;
}

extern "C" int arreau_debug_set_pollution(uint32_t pattern) {
    arreau_debug_pollution = pattern;
    return ARREAU_OK;
}
