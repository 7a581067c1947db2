// K6: the reverse updates of one denoising step (diffusion/diffusion_loss.py:338-347).
#include "update_dev.h"


// VP_lattice.reverse_given_x0 (diffusion_helpers.py:185-199) on lengths, then lattice_from_params.
// Note the reference adds `variance * z` (not sqrt(variance)) and zeroes z when t <= 1.
// TIE: the lattice-system tie of the lengths (length_tie[b]); the three x0 and current lengths are exchanged by shuffles.
// ETA: the eta move of the lengths (update_dev.h).
// INVERT: the inversion move of the lengths, from the crystal's level up to its target (update_dev.h; not with TIE or ETA).
// MS: the multistep move of the lengths (update_dev.h; with ETA, eta = 0); lane 0 of the crystal's four reads its history level,
// hands it on by a shuffle and overwrites it.
template <bool TIE, bool ETA, bool INVERT = false, bool MS = false>
__device__ __forceinline__ void reverse_lattice_body(int gt /* global thread of the lattice part */, float* __restrict__ lengths, const float* __restrict__ angles,
                                       const int32_t* __restrict__ tstep, const int32_t* __restrict__ offsets,
                                       const float* __restrict__ len0, StepNoiseSrc noise,
                                       const float* __restrict__ alpha_bars, const float* __restrict__ betas, int B,
                                       int T, float* __restrict__ lattice, const float* __restrict__ fixed_lengths,
                                       int32_t* __restrict__ status, int b0,
                                       // sampling loop: pool the per-atom read-out here (same ordered sum as
                                       // readout_crystals_kernel) instead of a launch of its own; len0_out receives it
                                       const float* __restrict__ gs_atoms, float* __restrict__ len0_out, const SampleConditionDev* cond,
                                       const StepScheduleDev* sched, uint32_t word3, const int32_t* __restrict__ length_tie,
                                       float eta, const arreau_multistep& ms = {} /* MS only */) {
    // four lanes per crystal: lane i < 3 owns length component i (pooling, update), lane 0 then writes the cell
    const int b = b0 + (gt >> 2), i = gt & 3;
    const bool live = b < B;  // (whole groups of four are live or not; the shuffles below need every lane)
    const int bc = live ? b : B - 1;
    int t = tstep[bc], s_to;
    if constexpr (INVERT) {
        static_assert(!TIE && !ETA, "the INVERT instances are untied and take no eta");
        t = invert_level(t, T, status, live && i == 0);
        s_to = invert_target(sched, bc, t, T, status, live && i == 0);
    } else {
        if (live && i == 0 && (t < 1 || t > T)) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
        t = t < 1 ? 1 : (t > T ? T : t);
        s_to = step_target(sched, bc, t, status, live && i == 0);
    }
    const int first = offsets[bc], last = offsets[bc + 1];
    float mylen = 0.f;
    int hist_p = 0;
    if constexpr (MS) {
        static_assert(ETA && !INVERT, "the MS instances are ETA instances (at eta = 0)");
        if (live && i == 0) hist_p = ms.hist_t_len[b];
        hist_p = __shfl(hist_p, (threadIdx.x & 63) & ~3, 64);
    }
    if constexpr (TIE) {
        const int code = length_tie_code(length_tie, cond ? cond->len_mask : nullptr, bc, status, live && i == 0);
        float x0 = 0.f, xt = 0.f, x0p = 0.f;
        if (live && i < 3) {
            x0 = length_x0_component(b, i, first, last, len0, gs_atoms, len0_out);
            xt = lengths[3 * b + i];
            if constexpr (MS) x0p = ms.hist_x0[3 * b + i];
        }
        const int lead = (threadIdx.x & 63) & ~3;
        float x0s[3], xts[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            x0s[q] = __shfl(x0, lead + q, 64);
            xts[q] = __shfl(xt, lead + q, 64);
        }
        if constexpr (MS) {
            float x0ps[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) x0ps[q] = __shfl(x0p, lead + q, 64);
            if (live && i < 3)
                mylen = tied_length_component<ETA, true>(b, i, code, x0s, xts, t, s_to, sched, lengths, noise, alpha_bars, betas, fixed_lengths,
                                                         cond, word3, eta, ms, x0ps, hist_p, T);
        } else {
            if (live && i < 3)
                mylen = tied_length_component<ETA>(b, i, code, x0s, xts, t, s_to, sched, lengths, noise, alpha_bars, betas, fixed_lengths, cond,
                                                   word3, eta);
        }
    } else if constexpr (MS) {
        if (live && i < 3)
            mylen = reverse_length_component<ETA, false, true>(b, i, t, s_to, sched, first, last, lengths, len0, noise, alpha_bars, betas,
                                                               fixed_lengths, gs_atoms, len0_out, cond, word3, eta, ms, hist_p, T);
    } else {
        if (live && i < 3)
            mylen = reverse_length_component<ETA, INVERT>(b, i, t, s_to, sched, first, last, lengths, len0, noise, alpha_bars, betas,
                                                          fixed_lengths, gs_atoms, len0_out, cond, word3, eta);
    }
    if constexpr (MS) {
        if (live && i == 0) ms.hist_t_len[b] = t;
    }
    const int base = (threadIdx.x & 63) & ~3;
    float newlen[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) newlen[q] = __shfl(mylen, base + q, 64);
    if (!live || i != 0) return;
    // lattice_from_params (lattice_helpers.py:55-105)
    const float* ang = angles + 3 * b;
    const float ca = cosf(ang[0]), cb = cosf(ang[1]), cg = cosf(ang[2]);
    const float sa = sinf(ang[0]), sb = sinf(ang[1]);
    float val = (ca * cb - cg) / (sa * sb);
    val = fminf(fmaxf(val, -1.0f), 1.0f);
    const float gs = acosf(val);
    float* Lm = lattice + 9 * b;
    Lm[0] = newlen[0] * sb;             Lm[1] = 0.0f;                      Lm[2] = newlen[0] * cb;
    Lm[3] = -newlen[1] * sa * cosf(gs); Lm[4] = newlen[1] * sa * sinf(gs); Lm[5] = newlen[1] * ca;
    Lm[6] = 0.0f;                       Lm[7] = 0.0f;                      Lm[8] = newlen[2];
}

// ONE launch for the four updates of a step (round 3; they were two): the first `lat_blocks` workgroups (256 threads = 64
// crystals, four lanes each) run the lattice update, the others the atom update, one wave per atom.  The two parts touch
// disjoint data (lengths / lattice / pooled read-out against coordinates / types), so nothing orders them.
// COND: conditioned sampling (the condition argument is read); SCHED: a respaced step (the schedule argument is read: s from a
// per-crystal array or the loop's next-timestep table).  reverse_kernel<false, false, false> is the plain kernel, whose helpers
// see a null condition and a null schedule and compile to what they were before either existed.
// RESAMPLE: a step of a resampled loop (arreau_sample_loop_resampled) in pass r of a block, r read from the loop's device word
// `pass` (set by the jump in front of the pass, reset after the block), so one captured step serves every pass.  Every draw of
// the step takes counter word3 = 256 r; pass 0 draws what the plain kernel draws.  Without RESAMPLE `pass` is not read.
// TIE: lattice systems (arreau_sample_loop_tied): the lengths of crystal b are tied by the code length_tie[b] (0 none, 1 a = b,
// 2 a = b = c; rules in include/arreau_hip.h).  Without TIE `length_tie` is not read.
// SYM: space-group symmetry (arreau_sample_loop_sym): the atom part runs reverse_atoms_body_sym on the orbit tables `sym_arg`
// (a leader's wave updates its whole orbit, members leave).  Only without COND and RESAMPLE.  Without SYM `sym_arg` is not read.
// ETA: DDIM-style sampling (arreau_sample_loop_eta): positions and lengths make the eta moves of update_dev.h, the noise scaled
// by `eta` in [0, 1] and not read at 0; the species step is unchanged.  Not with SYM.  Without ETA `eta` is not read.
// INVERT: DDIM inversion (arreau_invert_loop / arreau_invert_step): every crystal climbs from its level `tstep` up to the target the
// schedule argument names (the ascending table or the per-crystal array), lengths and positions by the inversion moves of
// update_dev.h; the atom part is the position move alone (invert_atoms_body), so `types`, `logits` and the noise are not read.
// Only with SCHED and none of the others.
// MS: second-order multistep sampling (arreau_sample_loop_multistep): an ETA instance, launched with eta = 0, whose position and
// length moves extrapolate with the previous step's prediction kept in the history buffers `ms_arg` (update_dev.h; rules in
// include/arreau_hip.h).  Only SCHED and TIE vary.  Without MS `ms_arg` is not read.
// SPEC: species control (arreau_sample_loop_species): the species half of the atom part admits, per crystal, the classes of the
// row spec_arg.d_allow[b] only and scales its Gumbel term by spec_arg.temperature (update_dev.h: d3pm_reverse_class<true>; rules
// in include/arreau_hip.h).  Positions and lengths do not see it, so it goes with every instance but INVERT, which has no species
// half.  Without SPEC `spec_arg` is not read.
template <bool COND, bool SCHED, bool RESAMPLE, bool TIE, bool SYM, bool ETA, bool INVERT = false, bool MS = false, bool SPEC = false>
__global__ __launch_bounds__(256) void reverse_kernel(
    int lat_blocks, float* __restrict__ lengths, const float* __restrict__ angles, const int32_t* __restrict__ tstep,
    const int32_t* __restrict__ offsets, const float* __restrict__ len0, StepNoiseSrc noise, const float* __restrict__ alpha_bars,
    const float* __restrict__ betas, int B_lat, int T, float* __restrict__ lattice, const float* __restrict__ fixed_lengths,
    int32_t* __restrict__ status, int b0, const float* __restrict__ gs_atoms, float* __restrict__ len0_out,
    float* __restrict__ frac, int32_t* __restrict__ types, int B, int N, const float* __restrict__ eps,
    const float* __restrict__ logits, const float* __restrict__ ve_sigmas, const float* __restrict__ q1t,
    const float* __restrict__ qmats, int S, const int32_t* __restrict__ const_types, int absorbing, int n0,
    const int32_t* __restrict__ batch,
    // sampling loop: the lattice part is one workgroup per crystal, which also prepares the next step (reverse_crystal_block)
    float* __restrict__ lattice_ws, float* __restrict__ cvec_next, const float* __restrict__ t_emb_w, const float* __restrict__ embT, int C,
    SampleConditionDev cond_arg, StepScheduleDev sched_arg, const int32_t* __restrict__ pass, const int32_t* __restrict__ length_tie,
    arreau_symmetry sym_arg, float eta, arreau_multistep ms_arg, arreau_species_control spec_arg) {
    const uint32_t word3 = RESAMPLE ? 256u * (uint32_t)pass[0] : 0u;  // the counter word of pass r
    const SampleConditionDev* cond = COND ? &cond_arg : nullptr;
    const StepScheduleDev* sched = SCHED ? &sched_arg : nullptr;
    if ((int)blockIdx.x < lat_blocks && cvec_next != nullptr) {  // (kernel argument: uniform)
        if constexpr (MS)
            reverse_crystal_block<TIE, ETA, false, true>(b0 + (int)blockIdx.x, lengths, angles, tstep, offsets, len0, noise, alpha_bars, betas,
                                                         T, lattice, fixed_lengths, status, gs_atoms, len0_out, lattice_ws, cvec_next, t_emb_w,
                                                         embT, S, C, cond, sched, word3, length_tie, eta, ms_arg);
        else
            reverse_crystal_block<TIE, ETA, INVERT>(b0 + (int)blockIdx.x, lengths, angles, tstep, offsets, len0, noise, alpha_bars, betas, T,
                                                    lattice, fixed_lengths, status, gs_atoms, len0_out, lattice_ws, cvec_next, t_emb_w, embT, S,
                                                    C, cond, sched, word3, length_tie, eta);
        return;
    }
    if ((int)blockIdx.x < lat_blocks) {
        if constexpr (MS)
            reverse_lattice_body<TIE, ETA, false, true>(blockIdx.x * blockDim.x + threadIdx.x, lengths, angles, tstep, offsets, len0, noise,
                                                        alpha_bars, betas, B_lat, T, lattice, fixed_lengths, status, b0, gs_atoms, len0_out, cond,
                                                        sched, word3, length_tie, eta, ms_arg);
        else
            reverse_lattice_body<TIE, ETA, INVERT>(blockIdx.x * blockDim.x + threadIdx.x, lengths, angles, tstep, offsets, len0, noise,
                                                   alpha_bars, betas, B_lat, T, lattice, fixed_lengths, status, b0, gs_atoms, len0_out, cond,
                                                   sched, word3, length_tie, eta);
        return;
    }
    if constexpr (MS) {
        static_assert(!COND && !RESAMPLE && !SYM && ETA && !INVERT, "the MS instances vary in SCHED and TIE only");
        reverse_atoms_body<true, true, SPEC>((int)blockIdx.x - lat_blocks, frac, types, tstep, offsets, B, N, eps, logits, noise, ve_sigmas, q1t,
                                             qmats, S, T, const_types, absorbing, status, n0, batch, cond, sched, word3, eta, ms_arg, spec_arg);
    } else if constexpr (INVERT) {
        static_assert(!COND && SCHED && !RESAMPLE && !TIE && !SYM && !ETA && !SPEC, "the INVERT instance takes a schedule and no other option");
        invert_atoms_body((int)blockIdx.x - lat_blocks, frac, tstep, offsets, B, N, eps, ve_sigmas, T, status, n0, batch, sched);
    } else if constexpr (SYM) {
        static_assert(!COND && !RESAMPLE && !ETA, "the SYM instances are unconditioned, not resampled and take no eta");
        reverse_atoms_body_sym<SPEC>((int)blockIdx.x - lat_blocks, frac, types, tstep, offsets, B, N, eps, logits, noise, ve_sigmas, q1t, qmats,
                                     S, T, const_types, absorbing, status, n0, batch, sched, sym_arg, spec_arg);
    } else {
        reverse_atoms_body<ETA, false, SPEC>((int)blockIdx.x - lat_blocks, frac, types, tstep, offsets, B, N, eps, logits, noise, ve_sigmas, q1t,
                                             qmats, S, T, const_types, absorbing, status, n0, batch, cond, sched, word3, eta, {}, spec_arg);
    }
}

namespace {
// the instance of one step: TIE and RESAMPLE from the options' pointers
template <bool COND, bool SCHED, bool ETA, bool SPEC>
auto reverse_kernel_of(const StepOptions& opt) {
    return opt.length_tie ? (opt.pass ? reverse_kernel<COND, SCHED, true, true, false, ETA, false, false, SPEC>
                                      : reverse_kernel<COND, SCHED, false, true, false, ETA, false, false, SPEC>)
                          : (opt.pass ? reverse_kernel<COND, SCHED, true, false, false, ETA, false, false, SPEC>
                                      : reverse_kernel<COND, SCHED, false, false, false, ETA, false, false, SPEC>);
}
// SPEC: species control; every instance below has its SPEC twin, the inversion step excepted
template <bool COND, bool SCHED, bool SPEC>
void enqueue_reverse_kernel(const arreau_model* m, int lat_blocks, int atom_blocks, const SampleState& st, const ReverseInputs& in,
                            const SampleConditionDev& cond, const StepScheduleDev& sched, const StepOptions& opt, hipStream_t s) {
    auto kernel = opt.eta >= 0.0f ? reverse_kernel_of<COND, SCHED, true, SPEC>(opt) : reverse_kernel_of<COND, SCHED, false, SPEC>(opt);
    if constexpr (!COND && SCHED && !SPEC) {
        if (opt.invert) kernel = reverse_kernel<false, true, false, false, false, false, true>;
    }
    if constexpr (!COND) {
        if (opt.ms)
            kernel = opt.length_tie ? reverse_kernel<false, SCHED, false, true, false, true, false, true, SPEC>
                                    : reverse_kernel<false, SCHED, false, false, false, true, false, true, SPEC>;
    }
    if constexpr (!COND) {
        if (opt.sym)
            kernel = opt.length_tie ? reverse_kernel<false, SCHED, false, true, true, false, false, false, SPEC>
                                    : reverse_kernel<false, SCHED, false, false, true, false, false, false, SPEC>;
    }
    ARREAU_LAUNCH(kernel, dim3(lat_blocks + atom_blocks), dim3(256), 0, s, lat_blocks, st.lengths, st.angles, in.t, st.offsets, in.len0, in.noise,
                  m->vp_alpha_bars, m->vp_betas, st.B, m->T, st.lattice, st.fixed_lengths, m->status, 0, in.gs_atoms,
                  in.gs_atoms ? const_cast<float*>(in.len0) : nullptr, st.frac, st.types, st.B, st.N, in.eps, in.logits, m->ve_sigmas, m->q1t,
                  m->qmats, m->S, st.const_types, m->qmats_absorbing, 0, in.batch, in.lattice_ws, in.cvec_next, m->t_emb_w, m->embT, m->C,
                  cond, sched, opt.pass, opt.length_tie, opt.sym ? *opt.sym : arreau_symmetry{}, opt.eta,
                  opt.ms ? *opt.ms : arreau_multistep{}, opt.species ? *opt.species : arreau_species_control{});
}
}  // namespace

int arreau_launch_reverse(const arreau_model* m, const SampleState& st, const ReverseInputs& in, const StepOptions& opt, hipStream_t s) {
    const bool prep_next = in.cvec_next != nullptr;  // one workgroup per crystal, which also prepares the next step
    ARREAU_REQUIRE(!prep_next || in.lattice_ws != nullptr, "reverse update: the next step's set-up needs the workspace lattice");
    const int lat_blocks = st.B > 0 ? (prep_next ? st.B : (4 * st.B + 255) / 256) : 0;
    const int atom_blocks = st.N > 0 ? (st.N + 3) / 4 : 0;
    const bool conditioned = !arreau_condition_empty(opt.cond);
    ARREAU_REQUIRE(!conditioned || (!in.noise.z_lattice && !in.noise.z_frac && !in.noise.u_types),
                   "reverse update: conditioned sampling needs the in-kernel (Philox) noise");
    const bool scheduled = opt.sched != nullptr;
    ARREAU_REQUIRE(!scheduled || (opt.sched->next != nullptr) != (opt.sched->s_of != nullptr),
                   "reverse update: a respaced step takes either the next-timestep table or the per-crystal targets");
    ARREAU_REQUIRE(!opt.sym || (!conditioned && opt.pass == nullptr),
                   "reverse update: space-group symmetry is not combined with a condition or a resampled loop");
    ARREAU_REQUIRE(!opt.sym || opt.eta < 0.0f, "reverse update: space-group symmetry is not combined with an eta");
    ARREAU_REQUIRE(!opt.invert || (scheduled && !conditioned && !opt.pass && !opt.length_tie && !opt.sym && opt.eta < 0.0f && opt.corr.steps == 0),
                   "reverse update: an inversion step takes its targets and no other option");
    ARREAU_REQUIRE(!opt.ms || (!conditioned && !opt.pass && !opt.sym && !opt.invert && opt.corr.steps == 0 && opt.eta == 0.0f),
                   "reverse update: a multistep step is the eta = 0 step and takes a schedule and a tie only");
    ARREAU_REQUIRE(!opt.ms || (opt.ms->hist_eps && opt.ms->hist_x0 && opt.ms->hist_t_atom && opt.ms->hist_t_len),
                   "reverse update: a multistep history pointer is null");
    ARREAU_REQUIRE(!opt.species || !opt.invert, "reverse update: an inversion step has no species half to control");
    ARREAU_REQUIRE(!opt.species || (std::isfinite(opt.species->temperature) && opt.species->temperature >= 0.0f),
                   "reverse update: the species temperature must be finite and not negative");
    if (lat_blocks + atom_blocks == 0) return ARREAU_OK;
    const SampleConditionDev c = conditioned ? *opt.cond : SampleConditionDev{};
    const StepScheduleDev sc = scheduled ? *opt.sched : StepScheduleDev{};
    auto enqueue = opt.species ? (conditioned ? (scheduled ? enqueue_reverse_kernel<true, true, true> : enqueue_reverse_kernel<true, false, true>)
                                              : (scheduled ? enqueue_reverse_kernel<false, true, true> : enqueue_reverse_kernel<false, false, true>))
                               : (conditioned ? (scheduled ? enqueue_reverse_kernel<true, true, false> : enqueue_reverse_kernel<true, false, false>)
                                              : (scheduled ? enqueue_reverse_kernel<false, true, false> : enqueue_reverse_kernel<false, false, false>));
    enqueue(m, lat_blocks, atom_blocks, st, in, c, sc, opt, s);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

extern "C" int arreau_reverse_step(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                   const float* d_angles, const int32_t* d_t, const int32_t* d_off, int32_t B,
                                   int32_t N, const float* d_eps, const float* d_logits, const float* d_len0,
                                   const float* d_z_lattice, const float* d_z_frac, const float* d_u_types,
                                   float* d_lattice, void* stream) {
    ARREAU_REQUIRE(m && d_frac && d_types && d_lengths && d_angles && d_t && d_off && d_eps && d_logits && d_len0 &&
                       d_z_lattice && d_z_frac && d_u_types && d_lattice, "arreau_reverse_step: null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, "arreau_reverse_step: bad size");
    const SampleState st{.frac = d_frac, .types = d_types, .lengths = d_lengths, .angles = d_angles, .offsets = d_off, .B = B, .N = N,
                         .lattice = d_lattice};
    const ReverseInputs in{d_t, d_eps, d_logits, d_len0, StepNoiseSrc{d_z_lattice, d_z_frac, d_u_types, 0}};
    return arreau_launch_reverse(m, st, in, StepOptions{}, (hipStream_t)stream);
}

// What the arreau_reverse_step_to family of exports share, as the caller gave it: arreau_reverse_step's arguments, the per-crystal
// targets s and the clip.  Each export fills it, names its options in a StepOptions and calls reverse_step_to.
struct StepToArgs {
    const arreau_model* m;
    float *frac, *lengths, *lattice;
    int32_t* types;
    const float *angles, *eps, *logits, *len0, *z_lattice, *z_frac, *u_types;
    const int32_t *t, *s, *offsets;
    int32_t B, N;
    float clipmax;
    void* stream;
};

// arreau_reverse_step from timestep t to a per-crystal target s (respaced sampling; rules in include/arreau_hip.h), with the
// options of `opt` (its schedule is set here).
static int reverse_step_to(const char* who, const StepToArgs& a, StepOptions opt) {
    // (at eta = 0 the draws of the lengths and positions are not read: their arrays may be null; so may the species' uniforms at a
    // species temperature of 0)
    ARREAU_REQUIRE(a.m && a.frac && a.types && a.lengths && a.angles && a.t && a.s && a.offsets && a.eps && a.logits && a.len0 &&
                       ((a.z_lattice && a.z_frac) || opt.eta == 0.0f) && (a.u_types || (opt.species && opt.species->temperature == 0.0f)) &&
                       a.lattice, std::string(who) + ": null pointer");
    ARREAU_REQUIRE(a.B >= 1 && a.N >= 0, std::string(who) + ": bad size");
    ARREAU_REQUIRE(a.clipmax > 0.0f && a.clipmax <= 1.0f, std::string(who) + ": lattice_clipmax must lie in (0, 1]");
    const SampleState st{.frac = a.frac, .types = a.types, .lengths = a.lengths, .angles = a.angles, .offsets = a.offsets, .B = a.B, .N = a.N,
                         .lattice = a.lattice};
    const ReverseInputs in{a.t, a.eps, a.logits, a.len0, StepNoiseSrc{a.z_lattice, a.z_frac, a.u_types, 0}};
    const StepScheduleDev sched{nullptr, a.s, a.clipmax};
    opt.sched = &sched;
    return arreau_launch_reverse(a.m, st, in, opt, (hipStream_t)a.stream);
}

extern "C" int arreau_reverse_step_to(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                      const float* d_angles, const int32_t* d_t, const int32_t* d_s, const int32_t* d_off, int32_t B,
                                      int32_t N, const float* d_eps, const float* d_logits, const float* d_len0,
                                      const float* d_z_lattice, const float* d_z_frac, const float* d_u_types, float* d_lattice,
                                      float lattice_clipmax, void* stream) {
    const StepToArgs a{.m = m, .frac = d_frac, .lengths = d_lengths, .lattice = d_lattice, .types = d_types, .angles = d_angles, .eps = d_eps,
                       .logits = d_logits, .len0 = d_len0, .z_lattice = d_z_lattice, .z_frac = d_z_frac, .u_types = d_u_types, .t = d_t,
                       .s = d_s, .offsets = d_off, .B = B, .N = N, .clipmax = lattice_clipmax, .stream = stream};
    return reverse_step_to("arreau_reverse_step_to", a, StepOptions{});
}

// arreau_reverse_step_to with the lattice-system tie of the lengths (rules in include/arreau_hip.h); NULL = arreau_reverse_step_to.
extern "C" int arreau_reverse_step_tied(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                        const float* d_angles, const int32_t* d_t, const int32_t* d_s, const int32_t* d_off, int32_t B,
                                        int32_t N, const float* d_eps, const float* d_logits, const float* d_len0,
                                        const float* d_z_lattice, const float* d_z_frac, const float* d_u_types, float* d_lattice,
                                        float lattice_clipmax, const int32_t* d_length_tie, void* stream) {
    const StepToArgs a{.m = m, .frac = d_frac, .lengths = d_lengths, .lattice = d_lattice, .types = d_types, .angles = d_angles, .eps = d_eps,
                       .logits = d_logits, .len0 = d_len0, .z_lattice = d_z_lattice, .z_frac = d_z_frac, .u_types = d_u_types, .t = d_t,
                       .s = d_s, .offsets = d_off, .B = B, .N = N, .clipmax = lattice_clipmax, .stream = stream};
    return reverse_step_to("arreau_reverse_step_tied", a, StepOptions{.length_tie = d_length_tie});
}

// DDIM-style sampling: an eta that is finite and lies in [0, 1], or ARREAU_EINVAL.
int arreau_eta_check(float eta, const char* who) {
    ARREAU_REQUIRE(std::isfinite(eta) && eta >= 0.0f && eta <= 1.0f, std::string(who) + ": eta must be finite and lie in [0, 1]");
    return ARREAU_OK;
}

// arreau_reverse_step_tied as the eta step (rules in include/arreau_hip.h); the tie pointer may be NULL.
extern "C" int arreau_reverse_step_eta(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                       const float* d_angles, const int32_t* d_t, const int32_t* d_s, const int32_t* d_off, int32_t B,
                                       int32_t N, const float* d_eps, const float* d_logits, const float* d_len0,
                                       const float* d_z_lattice, const float* d_z_frac, const float* d_u_types, float* d_lattice,
                                       float lattice_clipmax, const int32_t* d_length_tie, float eta, void* stream) {
    int rc;
    if ((rc = arreau_eta_check(eta, "arreau_reverse_step_eta"))) return rc;
    const StepToArgs a{.m = m, .frac = d_frac, .lengths = d_lengths, .lattice = d_lattice, .types = d_types, .angles = d_angles, .eps = d_eps,
                       .logits = d_logits, .len0 = d_len0, .z_lattice = d_z_lattice, .z_frac = d_z_frac, .u_types = d_u_types, .t = d_t,
                       .s = d_s, .offsets = d_off, .B = B, .N = N, .clipmax = lattice_clipmax, .stream = stream};
    return reverse_step_to("arreau_reverse_step_eta", a, StepOptions{.length_tie = d_length_tie, .eta = eta + 0.0f /* -0 -> +0 */});
}

// Second-order multistep sampling: every history pointer given, or ARREAU_EINVAL.
int arreau_multistep_check(const arreau_multistep* ms, const char* who) {
    ARREAU_REQUIRE(ms && ms->hist_eps && ms->hist_x0 && ms->hist_t_atom && ms->hist_t_len,
                   std::string(who) + ": a multistep history pointer is null");
    return ARREAU_OK;
}

// arreau_reverse_step_eta at eta = 0 as the multistep step on the caller's history (rules in include/arreau_hip.h).
extern "C" int arreau_reverse_step_multistep(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                             const float* d_angles, const int32_t* d_t, const int32_t* d_s, const int32_t* d_off, int32_t B,
                                             int32_t N, const float* d_eps, const float* d_logits, const float* d_len0,
                                             const float* d_z_lattice, const float* d_z_frac, const float* d_u_types, float* d_lattice,
                                             float lattice_clipmax, const int32_t* d_length_tie, const arreau_multistep* multistep,
                                             void* stream) {
    int rc;
    if ((rc = arreau_multistep_check(multistep, "arreau_reverse_step_multistep"))) return rc;
    const StepToArgs a{.m = m, .frac = d_frac, .lengths = d_lengths, .lattice = d_lattice, .types = d_types, .angles = d_angles, .eps = d_eps,
                       .logits = d_logits, .len0 = d_len0, .z_lattice = d_z_lattice, .z_frac = d_z_frac, .u_types = d_u_types, .t = d_t,
                       .s = d_s, .offsets = d_off, .B = B, .N = N, .clipmax = lattice_clipmax, .stream = stream};
    return reverse_step_to("arreau_reverse_step_multistep", a, StepOptions{.length_tie = d_length_tie, .eta = 0.0f, .ms = multistep});
}

// Species control: a temperature that is finite and not negative, or ARREAU_EINVAL; *out the struct the kernels take (-0 -> +0).
int arreau_species_check(const arreau_species_control* species, const char* who, arreau_species_control* out) {
    ARREAU_REQUIRE(species != nullptr, std::string(who) + ": null species control");
    ARREAU_REQUIRE(std::isfinite(species->temperature) && species->temperature >= 0.0f,
                   std::string(who) + ": the species temperature must be finite and not negative");
    *out = arreau_species_control{species->d_allow, species->temperature + 0.0f};
    return ARREAU_OK;
}

// The step of whichever of arreau_reverse_step_to / _tied / _sym / _eta / _multistep the options name, under species control (rules in
// include/arreau_hip.h).  What those do not combine is rejected as there (arreau_launch_reverse).
extern "C" int arreau_reverse_step_species(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                           const float* d_angles, const int32_t* d_t, const int32_t* d_s, const int32_t* d_off, int32_t B,
                                           int32_t N, const float* d_eps, const float* d_logits, const float* d_len0,
                                           const float* d_z_lattice, const float* d_z_frac, const float* d_u_types, float* d_lattice,
                                           float lattice_clipmax, const int32_t* d_length_tie, const arreau_symmetry* symmetry,
                                           const float* eta, const arreau_multistep* multistep, const arreau_species_control* species,
                                           void* stream) {
    const char* who = "arreau_reverse_step_species";
    int rc;
    arreau_species_control sp;
    if ((rc = arreau_species_check(species, who, &sp))) return rc;
    if (eta && (rc = arreau_eta_check(*eta, who))) return rc;
    if (symmetry && (rc = arreau_symmetry_check(symmetry, who))) return rc;
    if (multistep) {
        if ((rc = arreau_multistep_check(multistep, who))) return rc;
        ARREAU_REQUIRE(!eta || *eta == 0.0f, std::string(who) + ": a multistep step is the eta = 0 step");
    }
    const float e = multistep ? 0.0f : (eta ? *eta + 0.0f /* -0 -> +0 */ : -1.0f);
    const StepToArgs a{.m = m, .frac = d_frac, .lengths = d_lengths, .lattice = d_lattice, .types = d_types, .angles = d_angles, .eps = d_eps,
                       .logits = d_logits, .len0 = d_len0, .z_lattice = d_z_lattice, .z_frac = d_z_frac, .u_types = d_u_types, .t = d_t,
                       .s = d_s, .offsets = d_off, .B = B, .N = N, .clipmax = lattice_clipmax, .stream = stream};
    return reverse_step_to(who, a, StepOptions{.length_tie = d_length_tie, .sym = symmetry, .eta = e, .ms = multistep, .species = &sp});
}

// DDIM inversion: one step from level d_s[b] up to level d_t[b] on the caller's network outputs (rules in include/arreau_hip.h).
extern "C" int arreau_invert_step(const arreau_model* m, float* d_frac, const int32_t* d_types, float* d_lengths, const float* d_angles,
                                  const int32_t* d_s, const int32_t* d_t, const int32_t* d_off, int32_t B, int32_t N,
                                  const float* d_eps, const float* d_len0, const float* d_fixed_lengths, float* d_lattice, void* stream) {
    ARREAU_REQUIRE(m && d_frac && d_types && d_lengths && d_angles && d_s && d_t && d_off && d_eps && d_len0 && d_lattice,
                   "arreau_invert_step: null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, "arreau_invert_step: bad size");
    // (the species are not read by the update and never written: the pointer only completes the state)
    const SampleState st{.frac = d_frac, .types = const_cast<int32_t*>(d_types), .lengths = d_lengths, .angles = d_angles, .offsets = d_off,
                         .B = B, .N = N, .fixed_lengths = d_fixed_lengths, .lattice = d_lattice};
    const ReverseInputs in{d_s, d_eps, /*logits=*/nullptr, d_len0, StepNoiseSrc{}};
    const StepScheduleDev sched{nullptr, d_t, 0.0f};
    return arreau_launch_reverse(m, st, in, StepOptions{.sched = &sched, .invert = true}, (hipStream_t)stream);
}

// arreau_reverse_step_tied with space-group symmetry (rules in include/arreau_hip.h); NULL = arreau_reverse_step_tied.
extern "C" int arreau_reverse_step_sym(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                       const float* d_angles, const int32_t* d_t, const int32_t* d_s, const int32_t* d_off, int32_t B,
                                       int32_t N, const float* d_eps, const float* d_logits, const float* d_len0,
                                       const float* d_z_lattice, const float* d_z_frac, const float* d_u_types, float* d_lattice,
                                       float lattice_clipmax, const int32_t* d_length_tie, const arreau_symmetry* symmetry, void* stream) {
    int rc;
    if (symmetry && (rc = arreau_symmetry_check(symmetry, "arreau_reverse_step_sym"))) return rc;
    const StepToArgs a{.m = m, .frac = d_frac, .lengths = d_lengths, .lattice = d_lattice, .types = d_types, .angles = d_angles, .eps = d_eps,
                       .logits = d_logits, .len0 = d_len0, .z_lattice = d_z_lattice, .z_frac = d_z_frac, .u_types = d_u_types, .t = d_t,
                       .s = d_s, .offsets = d_off, .B = B, .N = N, .clipmax = lattice_clipmax, .stream = stream};
    return reverse_step_to("arreau_reverse_step_sym", a, StepOptions{.length_tie = d_length_tie, .sym = symmetry});
}

// the host checks of a symmetry table set: every pointer given, sizes positive (the kernel checks every index it follows)
int arreau_symmetry_check(const arreau_symmetry* y, const char* who) {
    ARREAU_REQUIRE(y->leader && y->op && y->orbit && y->orbit_ptr && y->orbit_atoms && y->stab_ptr && y->stab_ops && y->rot && y->rot_inv &&
                       y->trans, std::string(who) + ": a symmetry table is null");
    ARREAU_REQUIRE(y->n_orbits >= 1 && y->n_orbit_atoms >= 1 && y->n_stab_ops >= 1 && y->n_ops >= 1,
                   std::string(who) + ": symmetry table sizes must be positive");
    return ARREAU_OK;
}

// The sampler's in-kernel noise, written out: out[i] = the draw (seed, timestep, kind, element i, word3) -- standard normal for
// kinds 0/1/3/4/5/6/7, uniform [0,1) for kinds 2 and 8.  For tests (known-answer / statistics) and for reproducing a Philox trajectory
// through arreau_reverse_step / arreau_corrector_step.
__global__ void philox_fill_kernel(uint64_t seed, uint32_t timestep, uint32_t kind, uint32_t word3, int64_t n, float* __restrict__ out,
                                   uint32_t* __restrict__ raw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (raw) {
        const Philox4 r = philox4x32_10((uint32_t)i, timestep, kind, word3, (uint32_t)seed, (uint32_t)(seed >> 32));
        for (int j = 0; j < 4; ++j) raw[4 * i + j] = r.x[j];
    }
    if (out) out[i] = (kind == ARREAU_DRAW_U_TYPES || kind == ARREAU_DRAW_U_JUMP_TYPES) ? philox_uniform(seed, timestep, kind, (uint32_t)i, word3)
                                                  : philox_normal(seed, timestep, kind, (uint32_t)i, word3);
}

extern "C" int arreau_philox_fill_word(uint64_t seed, int32_t timestep, int32_t kind, uint32_t word3, int64_t n, float* d_out,
                                       uint32_t* d_raw, void* stream) {
    ARREAU_REQUIRE((d_out || d_raw) && n >= 0 && kind >= 0 && kind <= (int32_t)ARREAU_DRAW_U_JUMP_TYPES,
                   "arreau_philox_fill_word: bad argument");
    if (n == 0) return ARREAU_OK;
    ARREAU_LAUNCH(philox_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed,
                  (uint32_t)timestep, (uint32_t)kind, word3, n, d_out, d_raw);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

extern "C" int arreau_philox_fill(uint64_t seed, int32_t timestep, int32_t kind, int64_t n, float* d_out, uint32_t* d_raw,
                                  void* stream) {
    ARREAU_REQUIRE((d_out || d_raw) && n >= 0 && kind >= 0 && kind <= 4, "arreau_philox_fill: bad argument");
    return arreau_philox_fill_word(seed, timestep, kind, 0u, n, d_out, d_raw, stream);
}

// Keyed sampling (rules in include/arreau_hip.h): the draws of the keyed loop written out in batch layout.  One workgroup per
// crystal b strides over its n_b * width (per atom) or width (per crystal) elements e: the draw (seeds[b], timestep, kind, e, word3)
// goes to row offsets[b] * width + e (per atom) or b * width + e (per crystal) -- what the caller's-noise exports read at that row.
__global__ __launch_bounds__(256) void philox_fill_crystals_kernel(const uint64_t* __restrict__ seeds, const int32_t* __restrict__ offsets,
                                                                   uint32_t timestep, uint32_t kind, uint32_t word3, int width, int per_atom,
                                                                   int uniform, float* __restrict__ out, uint32_t* __restrict__ raw) {
    const int b = blockIdx.x;
    const uint64_t seed = seeds[b];
    const int first = offsets[b], last = offsets[b + 1];
    const int64_t n = per_atom ? (int64_t)(last - first) * width : width;
    const int64_t row0 = per_atom ? (int64_t)first * width : (int64_t)b * width;
    for (int64_t e = threadIdx.x; e < n; e += blockDim.x) {
        if (raw) {
            const Philox4 r = philox4x32_10((uint32_t)e, timestep, kind, word3, (uint32_t)seed, (uint32_t)(seed >> 32));
            for (int j = 0; j < 4; ++j) raw[4 * (row0 + e) + j] = r.x[j];
        }
        if (out) out[row0 + e] = uniform ? philox_uniform(seed, timestep, kind, (uint32_t)e, word3) : philox_normal(seed, timestep, kind, (uint32_t)e, word3);
    }
}

extern "C" int arreau_philox_fill_crystals(const uint64_t* d_seeds, const int32_t* d_offsets, int32_t B, int32_t timestep, int32_t kind,
                                           uint32_t word3, int32_t per_atom_width, int32_t per_crystal_width, float* d_out, uint32_t* d_raw,
                                           void* stream) {
    ARREAU_REQUIRE(d_seeds && d_offsets && (d_out || d_raw) && B >= 0 && timestep >= 0, "arreau_philox_fill_crystals: bad argument");
    ARREAU_REQUIRE(kind >= 0 && kind <= (int32_t)ARREAU_DRAW_U_INIT_ANGLES && !(kind >= (int32_t)ARREAU_DRAW_U_TIMESTEP && kind <= (int32_t)ARREAU_DRAW_Z_TRAIN_LENGTHS),
                   "arreau_philox_fill_crystals: not a draw kind of the sampler");
    ARREAU_REQUIRE((per_atom_width > 0) != (per_crystal_width > 0) && per_atom_width >= 0 && per_crystal_width >= 0,
                   "arreau_philox_fill_crystals: give either a per-atom or a per-crystal width");
    if (B == 0) return ARREAU_OK;
    const int uniform = kind == (int32_t)ARREAU_DRAW_U_TYPES || kind == (int32_t)ARREAU_DRAW_U_JUMP_TYPES || kind == (int32_t)ARREAU_DRAW_U_INIT_ANGLES;
    ARREAU_LAUNCH(philox_fill_crystals_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, d_seeds, d_offsets, (uint32_t)timestep,
                  (uint32_t)kind, word3, per_atom_width > 0 ? per_atom_width : per_crystal_width, per_atom_width > 0 ? 1 : 0, uniform, d_out,
                  d_raw);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

// Conditioned sampling, rule 5 (include/arreau_hip.h): the known components of the initial state at tau = t_start, i.e. the
// helpers of the in-loop replacement with Philox timestep key t_start + 1.  One thread per known-position component (3 N),
// per known-length component (3 B) and per known species (N).
// Keyed sampling (arreau_condition_initial_state_keyed): with the table `seeds` (then `offsets` is read) a crystal's draws take its
// stream seed and elements counted within it; a thread finds its atom's crystal by bisection of `offsets`.
__global__ void condition_initial_state_kernel(float* __restrict__ frac, int32_t* __restrict__ types, float* __restrict__ lengths,
                                               int B, int N, int t_key, uint64_t seed, SampleConditionDev cond,
                                               const float* __restrict__ ve_sigmas, const float* __restrict__ alpha_bars,
                                               const int32_t* __restrict__ offsets, const uint64_t* __restrict__ seeds) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const StepNoiseSrc src{nullptr, nullptr, nullptr, seed, seeds};
    if (g < 3 * (int64_t)N) {
        if (cond.pos_mask && cond.pos_mask[g / 3]) {
            const int i = (int)(g / 3);
            int lo = 0;
            if (seeds != nullptr) {  // largest b with offsets[b] <= i
                int hi = B;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (offsets[mid] <= i) lo = mid; else hi = mid;
                }
            }
            const DrawKey dk = atom_draw_key(src, offsets, lo, i);
            frac[g] = known_frac_component(&cond, (size_t)g, 3u * dk.atom + (uint32_t)(g - 3 * (int64_t)i), t_key, t_key - 1, dk.seed, ve_sigmas, 0u);
        }
    } else if (g < 3 * (int64_t)N + 3 * (int64_t)B) {
        const int c = (int)(g - 3 * (int64_t)N), b = c / 3;
        if (cond.len_mask && cond.len_mask[b])
            lengths[c] = known_length_component(&cond, b, c - 3 * b, t_key, t_key - 1, length_draw_key(src, b), alpha_bars, 0u);
    } else if (g < 4 * (int64_t)N + 3 * (int64_t)B) {
        const int i = (int)(g - 3 * (int64_t)N - 3 * (int64_t)B);
        if (cond.type_mask && cond.type_mask[i]) types[i] = cond.a0[i];
    }
}

// the host struct -> the kernels' by-value form; a mask without its values is an error, values without a mask are ignored
int arreau_condition_to_dev(const arreau_sample_condition* c, SampleConditionDev* out) {
    *out = SampleConditionDev{};
    if (!c) return ARREAU_OK;
    ARREAU_REQUIRE(!(c->pos_mask && !c->x0) && !(c->type_mask && !c->a0) && !(c->len_mask && !c->l0),
                   "sample condition: a mask is given without the known values it selects");
    *out = SampleConditionDev{c->pos_mask ? c->x0 : nullptr, c->pos_mask, c->type_mask ? c->a0 : nullptr, c->type_mask,
                              c->len_mask ? c->l0 : nullptr, c->len_mask};
    return ARREAU_OK;
}

static int condition_initial_state(const char* who, const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, int32_t B,
                                   int32_t N, int32_t t_start, uint64_t seed, const arreau_sample_condition* cond, const int32_t* d_off,
                                   const uint64_t* d_crystal_seeds, void* stream) {
    ARREAU_REQUIRE(m && d_frac && d_types && d_lengths, std::string(who) + ": null pointer");
    ARREAU_REQUIRE(B >= 1 && N >= 0, std::string(who) + ": bad size");
    ARREAU_REQUIRE(t_start >= 1 && t_start <= m->T, std::string(who) + ": t_start must lie in 1..T");
    ARREAU_REQUIRE(!d_crystal_seeds || d_off, std::string(who) + ": the table of stream seeds needs the crystal offsets");
    SampleConditionDev c;
    int rc;
    if ((rc = arreau_condition_to_dev(cond, &c))) return rc;
    if (arreau_condition_empty(&c)) return ARREAU_OK;
    const int64_t n = 4 * (int64_t)N + 3 * (int64_t)B;
    ARREAU_LAUNCH(condition_initial_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_frac, d_types,
                  d_lengths, B, N, t_start + 1, seed, c, m->ve_sigmas, m->vp_alpha_bars, d_off, d_crystal_seeds);
    ARREAU_CHECK_HIP(hipGetLastError());
    return ARREAU_OK;
}

extern "C" int arreau_condition_initial_state(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths, int32_t B,
                                              int32_t N, int32_t t_start, uint64_t seed, const arreau_sample_condition* cond,
                                              void* stream) {
    return condition_initial_state("arreau_condition_initial_state", m, d_frac, d_types, d_lengths, B, N, t_start, seed, cond, nullptr,
                                   nullptr, stream);
}

// Keyed sampling (rules in include/arreau_hip.h): arreau_condition_initial_state with the crystal offsets and the table of stream
// seeds; a NULL table = arreau_condition_initial_state.
extern "C" int arreau_condition_initial_state_keyed(const arreau_model* m, float* d_frac, int32_t* d_types, float* d_lengths,
                                                    const int32_t* d_off, int32_t B, int32_t N, int32_t t_start, uint64_t seed,
                                                    const arreau_sample_condition* cond, const uint64_t* d_crystal_seeds, void* stream) {
    return condition_initial_state("arreau_condition_initial_state_keyed", m, d_frac, d_types, d_lengths, B, N, t_start, seed, cond, d_off,
                                   d_crystal_seeds, stream);
}
