// Device code of the reverse updates of one denoising step (K6), shared by the stand-alone kernel of update.hip and by the
// per-crystal tail of the sampling step (tail.hip).  Test infrastructure does not include this file.
#pragma once
#include "internal.h"
#include "philox.h"
#include "prep_dev.h"

#define D3PM_EPS 1e-6f  // d3pm.py:23

// torch.remainder(x, 1) for floats: fmod, then shift negatives up by one (can return exactly 1.0f
// for tiny negative x, like the reference's `% 1`).
__device__ __forceinline__ float remainder_one(float x) {
    float m = fmodf(x, 1.0f);
    if (m != 0.0f && m < 0.0f) m += 1.0f;
    return m;
}

// Keyed sampling (arreau_sample_loop_keyed; the rules are stated in include/arreau_hip.h): what a Philox draw of crystal b is keyed
// by.  Without the table (noise.seeds null -- a kernel argument, so the choice is a scalar one) it is the call's seed and the global
// index, exactly as before the table existed; with it the crystal's stream seed and the index counted within the crystal.
// The draws of an atom: `seed` and the atom index `atom` its elements are formed from (3 atom + d, atom S + c).
struct DrawKey {
    uint64_t seed;
    uint32_t atom;
};
__device__ __forceinline__ DrawKey atom_draw_key(const StepNoiseSrc& noise, const int32_t* __restrict__ offsets, int b, int i) {
    if (noise.seeds != nullptr) return DrawKey{noise.seeds[b], (uint32_t)(i - offsets[b])};
    return DrawKey{noise.seed, (uint32_t)i};
}
// The draws of crystal b's lengths: `seed` and the element `atom` of its first component (0 keyed, 3 b without).
__device__ __forceinline__ DrawKey length_draw_key(const StepNoiseSrc& noise, int b) {
    if (noise.seeds != nullptr) return DrawKey{noise.seeds[b], 0u};
    return DrawKey{noise.seed, 3u * (uint32_t)b};
}

// Respaced sampling (arreau_sample_loop_scheduled / arreau_reverse_step_to; rules in include/arreau_hip.h): the timestep s that
// the step leaving t (crystal b, t already clamped to 1..T) produces.  Without a schedule s = t - 1.  Valid targets are s = 0 at
// t = 1 and 1 <= s <= t - 1 above it; anything else is clamped into that range and flagged (by the caller's one thread per
// crystal: `flag`).
__device__ __forceinline__ int step_target(const StepScheduleDev* sc, int b, int t, int32_t* __restrict__ status, bool flag) {
    if (!sc) return t - 1;
    int s = sc->s_of ? sc->s_of[b] : sc->next[t];
    const int lo = t > 1 ? 1 : 0;
    if (s < lo || s > t - 1) {
        if (flag) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
        s = s < lo ? lo : t - 1;
    }
    return s;
}

// Conditioned sampling (arreau_sample_loop_conditioned; the rules are stated in include/arreau_hip.h).  The step that leaves
// timestep t produces tau (t - 1, or the scheduled s); a known component is the template forward-noised to tau with the Philox
// draw of (seed, t), and the template itself at tau = 0.  The initial state uses the same helpers with t = t_start + 1,
// tau = t_start.  word3: the counter word of the draw (0; 256 r in pass r of a resampled loop) -- no default, so that every
// call site says which.
// Rule 1, VE_pbc.forward (diffusion_helpers.py:43-47): component g = 3 i + d of a known position, drawn as element e under `seed`
// (e = g and the call's seed; keyed sampling: the component's index within its crystal and the crystal's stream seed).
__device__ __forceinline__ float known_frac_component(const SampleConditionDev* c, size_t g, uint32_t e, int t, int tau, uint64_t seed,
                                                      const float* __restrict__ ve_sigmas, uint32_t word3) {
    const float x0 = c->x0[g];
    if (tau == 0) return remainder_one(x0);
    const float z = philox_normal(seed, (uint32_t)t, ARREAU_DRAW_Z_KNOWN_FRAC, e, word3);
    return remainder_one(x0 + ve_sigmas[tau] * z);
}
// Rule 2, VP_lattice.forward (diffusion_helpers.py:156-163): component i of crystal b's known lengths, drawn as element
// key.atom + i under key.seed (length_draw_key).
__device__ __forceinline__ float known_length_component(const SampleConditionDev* c, int b, int i, int t, int tau, DrawKey key,
                                                        const float* __restrict__ alpha_bars, uint32_t word3) {
    const float l0 = c->l0[3 * b + i];
    if (tau == 0) return l0;
    const float ab = alpha_bars[tau];
    const float z = philox_normal(key.seed, (uint32_t)t, ARREAU_DRAW_Z_KNOWN_LENGTHS, key.atom + i, word3);
    return sqrtf(ab) * l0 + sqrtf(1.0f - ab) * z;
}

// DDIM-style sampling (arreau_sample_loop_eta / arreau_reverse_step_eta; the rules are stated in include/arreau_hip.h): the ETA
// instances of the length and position updates.  eta in [0, 1] scales the step's injected noise; at eta = 0 the draws (kinds 0
// and 1, or the caller's arrays, which may then be null) are not read.  The non-ETA instances do not see this code.
// The length move from t to s, float32 in the order of the rule: zz is the draw (0 for t <= 1), read only when eta > 0.
__device__ __forceinline__ float eta_length_move(float x0, float xt, float ab_t, float ab_s, float beta, float eta, float zz) {
    const float den = 1.0f - ab_t;
    const float var = (1.0f - ab_s) * beta / den;
    const float k = sqrtf(fmaxf((1.0f - ab_s) * (1.0f - eta * eta * beta / den), 0.0f) / den);
    float l = (sqrtf(ab_s) - k * sqrtf(ab_t)) * x0 + k * xt;
    if (eta > 0.0f) l += eta * var * zz;
    return l;
}
// The draw of length element e of the step at t for the eta move: none at eta = 0 (the array may be null) or for t <= 1.  The
// generator's element is pe under pseed (e and the call's seed; keyed sampling: the crystal's own).
__device__ __forceinline__ float eta_length_draw(StepNoiseSrc noise, uint32_t e, uint64_t pseed, uint32_t pe, int t, float eta, uint32_t word3) {
    if (!(eta > 0.0f) || t <= 1) return 0.0f;
    return noise.z_lattice ? noise.z_lattice[e] : philox_normal(pseed, (uint32_t)t, ARREAU_DRAW_Z_LATTICE, pe, word3);
}

// Second-order multistep sampling (arreau_sample_loop_multistep / arreau_reverse_step_multistep; the rules are stated in
// include/arreau_hip.h): the MS instances are ETA instances at eta = 0 whose position and length moves extrapolate with the previous
// step's prediction, kept per element in the caller's history buffers with the level it was made at.  Every element's history is
// read and then overwritten by the thread that owns it; a level is read by one thread of its atom / crystal, handed to the others
// in registers or LDS, and overwritten by that thread.  The other instances do not see this code.
// A history level p is usable for the step that leaves t when t < p <= T (0: empty); only a usable p indexes a table.
__device__ __forceinline__ bool ms_usable(int p, int t, int T) { return p > t && p <= T; }
// The move is second order when p is usable, the target is not level 0 and the step-size ratio lies in [1/3, 3] (a NaN fails).
__device__ __forceinline__ bool ms_second_order(bool usable, int s, float r) { return usable && s >= 1 && r >= 1.0f / 3.0f && r <= 3.0f; }
// One component of the position move (rule 1), float32 in the order of the rule: e = sig_t eps, ep the history, `first` the
// eta = 0 move (before the wrap), which a first-order step keeps.
__device__ __forceinline__ float ms_frac_move(float first, float x, float e, float ep, float sig_t, float sig_s, float sig_p, bool usable, int s) {
    const float r = logf(sig_p / sig_t) / logf(sig_t / sig_s);
    if (!ms_second_order(usable, s, r)) return first;
    const float d = e + (e - ep) / (2.0f * r);
    return x - (sig_t - sig_s) * d;
}
// Half the log-SNR of a VP level.
__device__ __forceinline__ float ms_lambda(float ab) { return 0.5f * (logf(ab) - logf(1.0f - ab)); }
// The length move (rule 2), float32 in the order of the rule: x0p the history, ab_p the history level's abar (any value when not
// usable), `first` the eta = 0 move, which a first-order step keeps.
__device__ __forceinline__ float ms_length_move(float first, float x0, float x0p, float xt, float ab_t, float ab_s, float ab_p, bool usable, int s) {
    const float lam_t = ms_lambda(ab_t);
    const float r = (lam_t - ms_lambda(ab_p)) / (ms_lambda(ab_s) - lam_t);
    if (!ms_second_order(usable, s, r)) return first;
    const float k = sqrtf(fmaxf(1.0f - ab_s, 0.0f) / (1.0f - ab_t));  // eta_length_move's k at eta = 0
    const float D = x0 + (x0 - x0p) / (2.0f * r);
    return (sqrtf(ab_s) - k * sqrtf(ab_t)) * D + k * xt;
}

// DDIM inversion (arreau_invert_loop / arreau_invert_step; the rules are stated in include/arreau_hip.h): the INVERT instances of
// the length and position updates climb from the level s a crystal is at to a higher level t, the inverse of the eta = 0 move.  In
// these instances the helpers' `t` is the level the step leaves (the lower one) and their `s` the level it produces (the higher
// one); no draw, no beta and no clip enters.  The other instances do not see this code.
// The level a crystal leaves, clamped to 1..T-1 (flagged by the caller's one thread per crystal: `flag`).
__device__ __forceinline__ int invert_level(int raw, int T, int32_t* __restrict__ status, bool flag) {
    int s = raw > T - 1 ? T - 1 : raw;
    s = s < 1 ? 1 : s;
    if (flag && s != raw) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
    return s;
}
// The level the step that leaves s (clamped) produces: the caller's per-crystal target or the loop's ascending table.  Valid
// targets are s + 1 .. T; anything else is clamped into that range and flagged.  (T caps last, so every table index stays in range.)
__device__ __forceinline__ int invert_target(const StepScheduleDev* sc, int b, int s, int T, int32_t* __restrict__ status, bool flag) {
    const int raw = sc->s_of ? sc->s_of[b] : sc->next[s];
    int t = raw < s + 1 ? s + 1 : raw;
    t = t > T ? T : t;
    if (flag && t != raw) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
    return t;
}
// The length move from level s up to t, float32 in the order of the rule.
__device__ __forceinline__ float invert_length_move(float x0, float ls, float ab_s, float ab_t) {
    const float rho = sqrtf((1.0f - ab_t) / (1.0f - ab_s));
    return sqrtf(ab_t) * x0 + rho * (ls - sqrtf(ab_s) * x0);
}
// One component of the position move from level s up to t: the unit-variance direction sig_s eps is kept and rescaled to sig_t.
__device__ __forceinline__ float invert_frac_move(float xs, float eps, float sig_s, float sig_t) {
    return remainder_one(xs + eps * sig_s * (sig_t - sig_s));
}

// One component of the length update of crystal b from timestep t to s (VP_lattice.reverse_given_x0 with t - 1 replaced by s;
// the per-atom read-out is pooled here when gs_atoms is given: the ordered sum of readout_crystals_kernel).  Writes
// lengths[3 b + i] and returns it.  A stride-1 step (always, without a schedule) takes beta from the model's betas table.
// ETA: the move is eta_length_move's (the same beta, x0 and x_t); everything around it is as without.
// INVERT: the move is invert_length_move's, from level t up to level s (same x0, same pooling; beta and the draw are not formed).
// MS (with ETA, eta = 0): the multistep move on the history `ms` with the crystal's history level hist_p; the history takes x0.
template <bool ETA = false, bool INVERT = false, bool MS = false>
__device__ __forceinline__ float reverse_length_component(int b, int i, int t, int s, const StepScheduleDev* sched, int first, int last, float* __restrict__ lengths,
                                                          const float* __restrict__ len0, StepNoiseSrc noise,
                                                          const float* __restrict__ alpha_bars, const float* __restrict__ betas,
                                                          const float* __restrict__ fixed_lengths, const float* __restrict__ gs_atoms,
                                                          float* __restrict__ len0_out, const SampleConditionDev* cond,
                                                          uint32_t word3 /* resampled loop: 256 r in pass r; else 0 */,
                                                          float eta = 0.0f /* ETA only */, const arreau_multistep& ms = {} /* MS only */,
                                                          int hist_p = 0 /* MS only */, int T = 0 /* MS only */) {
    const float* __restrict__ z = noise.z_lattice;
    const DrawKey dk = length_draw_key(noise, b);  // (keyed sampling: the crystal's stream seed, element i)
    const float n = (float)(last - first);
    const float ab_t = alpha_bars[t], ab_p = alpha_bars[s];
    const float beta = (sched == nullptr || s == t - 1) ? betas[t] : fminf(1.0f - ab_t / ab_p, sched->clipmax);
    const float denom = 1.0f - ab_t;
    const float alpha_t = 1.0f - beta;
    const float c0 = sqrtf(ab_p) * beta;
    const float c1 = sqrtf(alpha_t) * (1.0f - ab_p);
    const float variance = (1.0f - ab_p) * beta / denom;
    float pooled;
    if (gs_atoms != nullptr) {
        pooled = 0.f;  // the ordered sum of readout_crystals_kernel, four loads in flight at a time
        int a = first;
        for (; a + 3 < last; a += 4) {
            const float v0 = gs_atoms[(size_t)a * 3 + i], v1 = gs_atoms[(size_t)(a + 1) * 3 + i];
            const float v2 = gs_atoms[(size_t)(a + 2) * 3 + i], v3 = gs_atoms[(size_t)(a + 3) * 3 + i];
            pooled = (((pooled + v0) + v1) + v2) + v3;
        }
        for (; a < last; ++a) pooled += gs_atoms[(size_t)a * 3 + i];
        len0_out[3 * b + i] = pooled;
    } else {
        pooled = len0[3 * b + i];
    }
    const float x0 = pooled * n;  // pred_lengths_0 * num_atoms (diffusion_loss.py:338)
    const float xt = lengths[3 * b + i];
    float moved;
    if constexpr (INVERT) {
        moved = invert_length_move(x0, xt, ab_t, ab_p);
    } else if constexpr (ETA) {
        moved = eta_length_move(x0, xt, ab_t, ab_p, beta, eta, eta_length_draw(noise, 3u * b + i, dk.seed, dk.atom + i, t, eta, word3));
        if constexpr (MS) {
            const bool usable = ms_usable(hist_p, t, T);
            moved = ms_length_move(moved, x0, ms.hist_x0[3 * b + i], xt, ab_t, ab_p, alpha_bars[usable ? hist_p : t], usable, s);
            ms.hist_x0[3 * b + i] = x0;
        }
    } else {
        const float mean = (c0 * x0 + c1 * xt) / denom;
        const float zdraw = z ? z[3 * b + i] : philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_LATTICE, dk.atom + i, word3);
        const float zz = t > 1 ? zdraw : 0.0f;
        moved = mean + variance * zz;
    }
    // fixed-cell sampling (arreau_sample_loop, d_fixed_lengths): the given lengths are re-imposed after the update
    float mylen = fixed_lengths ? fixed_lengths[3 * b + i] : moved;
    // conditioned sampling, rule 2: a known length is replaced before the cell is formed from it
    if (cond && cond->len_mask && cond->len_mask[b]) mylen = known_length_component(cond, b, i, t, s, dk, alpha_bars, word3);
    lengths[3 * b + i] = mylen;
    return mylen;
}

// Lattice systems (arreau_sample_loop_tied; the rules are stated in include/arreau_hip.h): the tie code of crystal b -- 0 none,
// 1 a = b, 2 a = b = c.  A code outside 0..2 counts as 0 and is flagged (by the crystal's one thread: `flag`); a crystal whose
// lengths a condition knows is not tied (rule 4).
__device__ __forceinline__ int length_tie_code(const int32_t* __restrict__ tie, const uint8_t* __restrict__ len_mask, int b,
                                               int32_t* __restrict__ status, bool flag) {
    int code = tie[b];
    if (code < 0 || code > 2) {
        if (flag) atomicOr(status, ARREAU_STATUS_BAD_TIE);  // untied, but flagged
        code = 0;
    }
    return (len_mask && len_mask[b]) ? 0 : code;
}
// Axis i is in the tied group G of code `code` (G = {0 .. code} for code >= 1; axis 0 leads).
__device__ __forceinline__ bool length_tied(int code, int i) { return code > 0 && i <= code; }

// Lattice systems, the length update of crystal b in two halves around the exchange of the three components (LDS or shuffles):
// the x0 of component i (pooled from gs_atoms when given, len0_out receiving the pooled value), then the tied update.  The
// arithmetic is reverse_length_component's, operation for operation (a code-0 crystal computes the same bits); it is kept apart so
// that the untied kernel instances keep their instructions.
__device__ __forceinline__ float length_x0_component(int b, int i, int first, int last, const float* __restrict__ len0,
                                                     const float* __restrict__ gs_atoms, float* __restrict__ len0_out) {
    const float n = (float)(last - first);
    float pooled;
    if (gs_atoms != nullptr) {
        pooled = 0.f;  // the ordered sum of readout_crystals_kernel
        int a = first;
        for (; a + 3 < last; a += 4) {
            const float v0 = gs_atoms[(size_t)a * 3 + i], v1 = gs_atoms[(size_t)(a + 1) * 3 + i];
            const float v2 = gs_atoms[(size_t)(a + 2) * 3 + i], v3 = gs_atoms[(size_t)(a + 3) * 3 + i];
            pooled = (((pooled + v0) + v1) + v2) + v3;
        }
        for (; a < last; ++a) pooled += gs_atoms[(size_t)a * 3 + i];
        len0_out[3 * b + i] = pooled;
    } else {
        pooled = len0[3 * b + i];
    }
    return pooled * n;  // pred_lengths_0 * num_atoms (diffusion_loss.py:338)
}
// Component i of the tied update (rule 1): an axis of the tied group G takes the leader's x_t and draw (element 3 b) and the group's
// mean x0 (summed in axis order, divided by |G|), so every axis of G computes the same bits; the others their own.  x0s / xts: the
// crystal's three x0 and current lengths.  Writes lengths[3 b + i] and returns it.  ETA: as in reverse_length_component.
// MS: as there; x0ps the crystal's three history values (an axis of G takes the leader's), and the history takes the x0 used.
template <bool ETA = false, bool MS = false>
__device__ __forceinline__ float tied_length_component(int b, int i, int code, const float* x0s, const float* xts, int t, int s,
                                                       const StepScheduleDev* sched, float* __restrict__ lengths, StepNoiseSrc noise,
                                                       const float* __restrict__ alpha_bars, const float* __restrict__ betas,
                                                       const float* __restrict__ fixed_lengths, const SampleConditionDev* cond,
                                                       uint32_t word3, float eta = 0.0f /* ETA only */,
                                                       const arreau_multistep& ms = {} /* MS only */, const float* x0ps = nullptr /* MS only */,
                                                       int hist_p = 0 /* MS only */, int T = 0 /* MS only */) {
    const bool tied = length_tied(code, i);
    const float* __restrict__ z = noise.z_lattice;
    const float ab_t = alpha_bars[t], ab_p = alpha_bars[s];
    const float beta = (sched == nullptr || s == t - 1) ? betas[t] : fminf(1.0f - ab_t / ab_p, sched->clipmax);
    const float denom = 1.0f - ab_t;
    const float alpha_t = 1.0f - beta;
    const float c0 = sqrtf(ab_p) * beta;
    const float c1 = sqrtf(alpha_t) * (1.0f - ab_p);
    const float variance = (1.0f - ab_p) * beta / denom;
    const float x0 = !tied ? x0s[i] : (code == 1 ? (x0s[0] + x0s[1]) / 2.0f : ((x0s[0] + x0s[1]) + x0s[2]) / 3.0f);
    const float xt = tied ? xts[0] : xts[i];
    const uint32_t e = 3u * b + (tied ? 0u : (uint32_t)i);
    const DrawKey dk = length_draw_key(noise, b);  // (keyed sampling: the crystal's stream seed, the leader's element 0)
    const uint32_t pe = dk.atom + (tied ? 0u : (uint32_t)i);
    float moved;
    if constexpr (ETA) {
        moved = eta_length_move(x0, xt, ab_t, ab_p, beta, eta, eta_length_draw(noise, e, dk.seed, pe, t, eta, word3));
        if constexpr (MS) {
            const bool usable = ms_usable(hist_p, t, T);
            moved = ms_length_move(moved, x0, tied ? x0ps[0] : x0ps[i], xt, ab_t, ab_p, alpha_bars[usable ? hist_p : t], usable, s);
            ms.hist_x0[3 * b + i] = x0;
        }
    } else {
        const float mean = (c0 * x0 + c1 * xt) / denom;
        const float zdraw = z ? z[e] : philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_LATTICE, pe, word3);
        const float zz = t > 1 ? zdraw : 0.0f;
        moved = mean + variance * zz;
    }
    float mylen = fixed_lengths ? fixed_lengths[3 * b + i] : moved;  // a fixed cell: the (host-tied) given lengths
    if (cond && cond->len_mask && cond->len_mask[b]) mylen = known_length_component(cond, b, i, t, s, dk, alpha_bars, word3);
    lengths[3 * b + i] = mylen;
    return mylen;
}

// Species control (arreau_sample_loop_species / arreau_reverse_step_species; the rules are stated in include/arreau_hip.h): whether
// the classes `lane` and `lane + 64` of crystal b are admitted by the step that leaves t.  The crystal's row of four words is
// wave-uniform (a null table admits every class); an ordinary class is admitted by its bit, the mask class S - 1 by its bit or,
// above t = 1, always.
__device__ __forceinline__ void species_admitted(const arreau_species_control& sp, int b, int lane, int S, int t, bool& a0, bool& a1) {
    uint32_t w0 = ~0u, w1 = ~0u, w2 = ~0u, w3 = ~0u;
    if (sp.d_allow != nullptr) {  // (kernel argument: uniform)
        const uint32_t* __restrict__ row = sp.d_allow + 4 * (size_t)b;
        w0 = row[0]; w1 = row[1]; w2 = row[2]; w3 = row[3];
    }
    const bool bit0 = (((lane < 32 ? w0 : w1) >> (lane & 31)) & 1u) != 0u;  // class lane: word lane >> 5
    const bool bit1 = (((lane < 32 ? w2 : w3) >> (lane & 31)) & 1u) != 0u;  // class lane + 64: word 2 + (lane >> 5)
    const int mask = S - 1;
    a0 = lane < S && (bit0 || (lane == mask && t > 1));
    a1 = lane + 64 < S && (bit1 || (lane + 64 == mask && t > 1));
}

// Space-group symmetry: D3PM.reverse on the class of atom i (d3pm.py:74-110, 198-215) from given x0 logits l0 / l1 of classes
// lane / lane + 64 (-inf beyond S), from timestep t to s_to: the new class (wave-uniform), drawn with atom i's uniforms (elements
// i S + s).  The arithmetic of reverse_one_atom's species half, operation for operation; it is kept apart so that the existing
// kernel instances keep their instructions.
// SPEC: species control -- the one place its rules are written, for a single atom (reverse_one_atom's SPEC instances) and for an
// orbit alike: the x0 logits and the posterior logits of a class outside the admitted set of crystal b become -inf, the Gumbel
// term is scaled by sp.temperature (0: no uniform is read or generated), and the arg-max runs over the admitted classes.  Without
// SPEC none of this is compiled: a0 / a1 are v0 / v1 and `b` and `sp` are not read.
template <bool SPEC = false>
__device__ __forceinline__ int d3pm_reverse_class(int i, int lane, float l0, float l1, int t, int s_to, const int32_t* __restrict__ types,
                                                  StepNoiseSrc noise, const float* __restrict__ q1t, const float* __restrict__ qmats, int S,
                                                  int absorbing, int32_t* __restrict__ status, const StepScheduleDev* sched, uint32_t word3,
                                                  DrawKey dk /* atom_draw_key of atom i */,
                                                  int b = 0 /* SPEC only */, const arreau_species_control& sp = {} /* SPEC only */) {
    const float* __restrict__ u_types = noise.u_types;
    // ---- D3PM posterior logits ------------------------------------------------------------------
    const int s0 = lane, s1 = lane + 64;
    const bool v0 = s0 < S, v1 = s1 < S;
    bool a0 = v0, a1 = v1;
    if constexpr (SPEC) {
        species_admitted(sp, b, lane, S, t, a0, a1);
        l0 = a0 ? l0 : -INFINITY;  // rule 1: the softmax gives an excluded class an exact 0
        l1 = a1 ? l1 : -INFINITY;
    }
    float post0, post1;
    if (t == 1) {
        post0 = l0; post1 = l1;  // raw x0 logits at the last step (d3pm.py:106-108)
    } else {
        float mx = fmaxf(l0, l1);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        const float e0 = a0 ? expf(l0 - mx) : 0.f, e1 = a1 ? expf(l1 - mx) : 0.f;  // (a0 / a1: v0 / v1 without SPEC)
        float sum = e0 + e1;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        const float p0 = e0 / sum, p1 = e1 / sum;  // softmax of the x0 logits; lane holds classes s0, s1
        int xt = types[i];
        if ((xt < 0 || xt >= S) && lane == 0) atomicOr(status, ARREAU_STATUS_BAD_TYPE);  // clamped, but flagged
        xt = xt < 0 ? 0 : (xt >= S ? S - 1 : xt);
        const bool unit = sched == nullptr || s_to == t - 1;
        const float* q1row = q1t + ((size_t)(t - 1) * S + xt) * S;  // fact1 = Q_t^T[x_t, :] (stride 1)
        const float* qm = qmats + (size_t)(s_to - 1) * S * S;  // Qbar_s (reference index t-2 at stride 1)
        float f2a = 0.f, f2b = 0.f;
        if (absorbing) {
            // Absorbing ("mask") chain: Qbar_t is diagonal plus the mask column (checked on the host for every t at model
            // creation).  The dense loop below adds exact zeros everywhere else, so these are bit for bit its sums: for an
            // ordinary class s only the term c = s, for the mask class the whole column in class order -- without the
            // S x S read per atom.
            const int mask = S - 1;
            const float d0 = v0 ? qm[(size_t)s0 * S + s0] : 0.f, d1 = v1 ? qm[(size_t)s1 * S + s1] : 0.f;
            const float c0 = v0 ? qm[(size_t)s0 * S + mask] : 0.f, c1 = v1 ? qm[(size_t)s1 * S + mask] : 0.f;
            f2a = fmaf(p0, d0, 0.f);
            f2b = fmaf(p1, d1, 0.f);
            float fm = 0.f;
            // (c is wave-uniform: the broadcasts are v_readlane, not LDS-crossbar permutes -- round 3: the 2 S permutes per atom
            // were most of this kernel's time)
            auto lane_value = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
            for (int c = 0; c < S; ++c) {
                const float pc = c < 64 ? lane_value(p0, c) : lane_value(p1, c - 64);
                const float qc = c < 64 ? lane_value(c0, c) : lane_value(c1, c - 64);
                fm = fmaf(pc, qc, fm);
            }
            if (s0 == mask) f2a = fm;
            if (s1 == mask) f2b = fm;
        } else
        // fact2 = softmax . Qbar: rows of Qbar are fetched 16 at a time (independent loads in flight), then the
        // softmax entries are broadcast from the lanes that hold them
        for (int c0 = 0; c0 < S; c0 += 16) {
            float qa[16], qb[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = min(c0 + i, S - 1);
                qa[i] = v0 ? qm[(size_t)c * S + s0] : 0.f;
                qb[i] = v1 ? qm[(size_t)c * S + s1] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = c0 + i;  // wave-uniform
                float sc = c < 64 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), c))
                                  : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p1), c - 64));
                sc = c < S ? sc : 0.f;
                f2a = fmaf(sc, qa[i], f2a);
                f2b = fmaf(sc, qb[i], f2b);
            }
        }
        if (unit) {
            post0 = v0 ? logf(q1row[s0] + D3PM_EPS) + logf(f2a + D3PM_EPS) : -INFINITY;
            post1 = v1 ? logf(q1row[s1] + D3PM_EPS) + logf(f2b + D3PM_EPS) : -INFINITY;
        } else {
            // respaced: fact1 = Qbar_{t-s}[:, x_t], the column x_t of q_mats[t-s-1] (the mask chain is time-homogeneous, so the
            // (t-s)-step transition is the (t-s)-step product).  Absorbing chain: that column is zero off the diagonal unless
            // x_t is the mask class -- the entries skipped are exact zeros, as in the shortcut above.
            const float* qcol = qmats + (size_t)(t - s_to - 1) * S * S + xt;
            const bool all = !absorbing || xt == S - 1;
            const float fa = (v0 && (all || s0 == xt)) ? qcol[(size_t)s0 * S] : 0.f;
            const float fb = (v1 && (all || s1 == xt)) ? qcol[(size_t)s1 * S] : 0.f;
            post0 = v0 ? logf(fa + D3PM_EPS) + logf(f2a + D3PM_EPS) : -INFINITY;
            post1 = v1 ? logf(fb + D3PM_EPS) + logf(f2b + D3PM_EPS) : -INFINITY;
        }
    }
    if constexpr (SPEC) {  // rule 3: without it an excluded class keeps 2 log(1e-6) and can win a draw
        post0 = a0 ? post0 : -INFINITY;
        post1 = a1 ? post1 : -INFINITY;
    }
    // ---- Gumbel arg-max (d3pm.py:206-214) ----------------------------------------------------------
    const float scale = (t != 1) ? 1.0f : 0.2f;
    // (the array-or-generator choice is made on the kernel argument itself -- a scalar compare -- not on a per-lane pointer:
    // no per-lane 64-bit integer compares on this path)
    const bool have_u = u_types != nullptr;
    const float* un = u_types + (have_u ? (size_t)i * S : 0);
    auto draw_u = [&](int s_) {
        return have_u ? un[s_] : philox_uniform(dk.seed, (uint32_t)t, ARREAU_DRAW_U_TYPES, dk.atom * (uint32_t)S + (uint32_t)s_, word3);
    };
    float best = -INFINITY;
    int besti = 0x7fffffff;
    if constexpr (SPEC) {
        // rules 4-5: value = post + (tau scale) g over the admitted classes; only a value above -inf competes (a NaN does not)
        const float ts = sp.temperature * scale;
        float val0 = post0, val1 = post1;
        if (sp.temperature > 0.0f) {  // (kernel argument: uniform; at 0 the uniforms are not touched and u_types may be null)
            if (a0) {
                const float u = fminf(fmaxf(draw_u(s0), D3PM_EPS), 1.0f);
                val0 = post0 + (-logf(-logf(u))) * ts;
            }
            if (a1) {
                const float u = fminf(fmaxf(draw_u(s1), D3PM_EPS), 1.0f);
                val1 = post1 + (-logf(-logf(u))) * ts;
            }
        }
        if (a0 && val0 > -INFINITY) { best = val0; besti = s0; }
        if (a1 && val1 > best) { best = val1; besti = s1; }
    } else {
        if (v0) {
            const float u = fminf(fmaxf(draw_u(s0), D3PM_EPS), 1.0f);
            best = post0 + (-logf(-logf(u))) * scale;
            besti = s0;
        }
        if (v1) {
            const float u = fminf(fmaxf(draw_u(s1), D3PM_EPS), 1.0f);
            const float val = post1 + (-logf(-logf(u))) * scale;
            if (val > best) { best = val; besti = s1; }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(besti, off, 64);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }  // first index wins ties
    }
    if constexpr (SPEC) {
        if (besti == 0x7fffffff) {  // (wave-uniform) no admitted value above -inf: the lowest admitted class
            const unsigned long long m0 = __ballot(a0), m1 = __ballot(a1);
            // (a row that admits nothing at t = 1 is rejected by the caller; the mask class keeps the index in range)
            besti = m0 ? __builtin_ctzll(m0) : (m1 ? 64 + __builtin_ctzll(m1) : S - 1);
        }
    }
    return besti;
}

// One wave per atom: VE_pbc.reverse on the fractional coordinates (diffusion_helpers.py:65-81) and
// D3PM.reverse on the atom type (d3pm.py:74-110, 198-215), from timestep t to s (t - 1 without a schedule).  Lanes span the S
// classes (2 per lane).  ETA: the position update is the eta move (rules in include/arreau_hip.h); the species half is unchanged.
// MS (with ETA, eta = 0): the multistep position move on the history `ms`; lane 0 reads and then overwrites the atom's level.
// SPEC: species control -- the species half is d3pm_reverse_class<true> on the atom's own logits and its crystal's row; the
// position half is unchanged.  The other instances do not see that call.
template <bool ETA = false, bool MS = false, bool SPEC = false>
__device__ __forceinline__ void reverse_one_atom(
    int i /* atom (wave-uniform) */, int lane, float* __restrict__ frac, int32_t* __restrict__ types, const int32_t* __restrict__ tstep,
    const int32_t* __restrict__ offsets, int B, const float* __restrict__ eps,
    const float* __restrict__ logits, StepNoiseSrc noise,
    const float* __restrict__ ve_sigmas, const float* __restrict__ q1t, const float* __restrict__ qmats, int S,
    int T, const int32_t* __restrict__ const_types, int absorbing, int32_t* __restrict__ status,
    const int32_t* __restrict__ batch /* crystal of each atom, or null: searched in `offsets` */,
    const SampleConditionDev* cond /* conditioned sampling, or null */, const StepScheduleDev* sched /* respaced, or null */,
    uint32_t word3 /* resampled loop: 256 r in pass r; else 0 */, float eta = 0.0f /* ETA only */,
    const arreau_multistep& ms = {} /* MS only */, const arreau_species_control& sp = {} /* SPEC only */) {
    static_assert(!MS || ETA, "the MS instances are ETA instances (at eta = 0)");
    const float* __restrict__ z_frac = noise.z_frac;
    const float* __restrict__ u_types = noise.u_types;
    // crystal of this atom = largest b with offsets[b] <= i: a 64-ary search by the whole wave (each level one
    // load per lane + a ballot) instead of log2(B) dependent loads
    int lo = 0, hi = B;
    if (batch != nullptr) {
        lo = batch[i];  // (the sampling loop has the index from prep_kernel: two dependent loads fewer)
    } else
    while (hi - lo > 1) {
        const int span = hi - lo, step = (span + 63) >> 6;
        const int probe = lo + lane * step;
        const bool le = probe < hi && offsets[probe] <= i;       // monotone in lane: true for lanes 0..c-1
        const int c = __builtin_popcountll(__ballot(le));         // c >= 1 because offsets[lo] <= i
        lo = lo + (c - 1) * step;
        hi = min(lo + step, hi);
    }
    int t = tstep[lo];
    t = t < 1 ? 1 : (t > T ? T : t);
    const int s_to = step_target(sched, lo, t, status, false);  // (flagged by the crystal's lattice thread)
    const DrawKey dk = atom_draw_key(noise, offsets, lo, i);  // (keyed sampling: the crystal's stream seed, the atom's index in it)
    int hist_p = 0;
    if constexpr (MS) {
        if (lane == 0) hist_p = ms.hist_t_atom[i];
        hist_p = __builtin_amdgcn_readfirstlane(hist_p);  // (the whole wave is active here)
    }

    if (lane < 3) {
        const float s = ve_sigmas[t];
        const float sp = ve_sigmas[s_to];  // t >= 1 here; the reference's t == 0 branch is unreachable in sampling
        const float s2 = s * s, sp2 = sp * sp;
        const size_t g = 3 * (size_t)i + lane;
        float fv;
        if constexpr (ETA) {
            // x0 = x_t - sig_t^2 eps in the predictor's convention; the direction term keeps what the noise does not take
            const float r = sp / s;
            const float dir = sp * sqrtf((1.0f - eta * eta) + eta * eta * r * r);
            float v = frac[g] - eps[g] * s * (s - dir);
            if (eta > 0.0f) {  // (at eta = 0 the draw is not read: z_frac may be null)
                const float zf = z_frac ? z_frac[g] : philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_FRAC, 3u * dk.atom + (uint32_t)lane, word3);
                v += eta * sp * sqrtf(1.0f - r * r) * zf;
            }
            if constexpr (MS) {
                const bool usable = ms_usable(hist_p, t, T);
                const float e = eps[g] * s;
                v = ms_frac_move(v, frac[g], e, ms.hist_eps[g], s, sp, ve_sigmas[usable ? hist_p : t], usable, s_to);
                ms.hist_eps[g] = e;
            }
            fv = remainder_one(v);
        } else {
            const float mean = frac[g] - eps[g] * (s2 - sp2);
            const float stdv = sqrtf((sp2 * (s2 - sp2)) / s2);
            const float zf = z_frac ? z_frac[g] : philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_FRAC, 3u * dk.atom + (uint32_t)lane, word3);
            fv = remainder_one(mean + stdv * zf);
        }
        if (cond && cond->pos_mask && cond->pos_mask[i]) fv = known_frac_component(cond, g, 3u * dk.atom + (uint32_t)lane, t, s_to, dk.seed, ve_sigmas, word3);  // rule 1
        frac[g] = fv;
    }
    if constexpr (MS) {
        if (lane == 0) ms.hist_t_atom[i] = t;
    }

    // ---- D3PM posterior logits ------------------------------------------------------------------
    const int s0 = lane, s1 = lane + 64;
    const bool v0 = s0 < S, v1 = s1 < S;
    const float* lg = logits + (size_t)i * S;
    const float l0 = v0 ? lg[s0] : -INFINITY, l1 = v1 ? lg[s1] : -INFINITY;
    if constexpr (SPEC) {
        const int cls = d3pm_reverse_class<true>(i, lane, l0, l1, t, s_to, types, noise, q1t, qmats, S, absorbing, status, sched, word3, dk, lo, sp);
        // rule 6: held species are imposed after the draw, as below
        if (lane == 0) types[i] = (cond && cond->type_mask && cond->type_mask[i]) ? cond->a0[i] : (const_types ? const_types[i] : cls);
        return;
    }
    float post0, post1;
    if (t == 1) {
        post0 = l0; post1 = l1;  // raw x0 logits at the last step (d3pm.py:106-108)
    } else {
        float mx = fmaxf(l0, l1);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        const float e0 = v0 ? expf(l0 - mx) : 0.f, e1 = v1 ? expf(l1 - mx) : 0.f;
        float sum = e0 + e1;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        const float p0 = e0 / sum, p1 = e1 / sum;  // softmax of the x0 logits; lane holds classes s0, s1
        int xt = types[i];
        if ((xt < 0 || xt >= S) && lane == 0) atomicOr(status, ARREAU_STATUS_BAD_TYPE);  // clamped, but flagged
        xt = xt < 0 ? 0 : (xt >= S ? S - 1 : xt);
        const bool unit = sched == nullptr || s_to == t - 1;
        const float* q1row = q1t + ((size_t)(t - 1) * S + xt) * S;  // fact1 = Q_t^T[x_t, :] (stride 1)
        const float* qm = qmats + (size_t)(s_to - 1) * S * S;  // Qbar_s (reference index t-2 at stride 1)
        float f2a = 0.f, f2b = 0.f;
        if (absorbing) {
            // Absorbing ("mask") chain: Qbar_t is diagonal plus the mask column (checked on the host for every t at model
            // creation).  The dense loop below adds exact zeros everywhere else, so these are bit for bit its sums: for an
            // ordinary class s only the term c = s, for the mask class the whole column in class order -- without the
            // S x S read per atom.
            const int mask = S - 1;
            const float d0 = v0 ? qm[(size_t)s0 * S + s0] : 0.f, d1 = v1 ? qm[(size_t)s1 * S + s1] : 0.f;
            const float c0 = v0 ? qm[(size_t)s0 * S + mask] : 0.f, c1 = v1 ? qm[(size_t)s1 * S + mask] : 0.f;
            f2a = fmaf(p0, d0, 0.f);
            f2b = fmaf(p1, d1, 0.f);
            float fm = 0.f;
            // (c is wave-uniform: the broadcasts are v_readlane, not LDS-crossbar permutes -- round 3: the 2 S permutes per atom
            // were most of this kernel's time)
            auto lane_value = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
            for (int c = 0; c < S; ++c) {
                const float pc = c < 64 ? lane_value(p0, c) : lane_value(p1, c - 64);
                const float qc = c < 64 ? lane_value(c0, c) : lane_value(c1, c - 64);
                fm = fmaf(pc, qc, fm);
            }
            if (s0 == mask) f2a = fm;
            if (s1 == mask) f2b = fm;
        } else
        // fact2 = softmax . Qbar: rows of Qbar are fetched 16 at a time (independent loads in flight), then the
        // softmax entries are broadcast from the lanes that hold them
        for (int c0 = 0; c0 < S; c0 += 16) {
            float qa[16], qb[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = min(c0 + i, S - 1);
                qa[i] = v0 ? qm[(size_t)c * S + s0] : 0.f;
                qb[i] = v1 ? qm[(size_t)c * S + s1] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = c0 + i;  // wave-uniform
                float sc = c < 64 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), c))
                                  : __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p1), c - 64));
                sc = c < S ? sc : 0.f;
                f2a = fmaf(sc, qa[i], f2a);
                f2b = fmaf(sc, qb[i], f2b);
            }
        }
        if (unit) {
            post0 = v0 ? logf(q1row[s0] + D3PM_EPS) + logf(f2a + D3PM_EPS) : -INFINITY;
            post1 = v1 ? logf(q1row[s1] + D3PM_EPS) + logf(f2b + D3PM_EPS) : -INFINITY;
        } else {
            // respaced: fact1 = Qbar_{t-s}[:, x_t], the column x_t of q_mats[t-s-1] (the mask chain is time-homogeneous, so the
            // (t-s)-step transition is the (t-s)-step product).  Absorbing chain: that column is zero off the diagonal unless
            // x_t is the mask class -- the entries skipped are exact zeros, as in the shortcut above.
            const float* qcol = qmats + (size_t)(t - s_to - 1) * S * S + xt;
            const bool all = !absorbing || xt == S - 1;
            const float fa = (v0 && (all || s0 == xt)) ? qcol[(size_t)s0 * S] : 0.f;
            const float fb = (v1 && (all || s1 == xt)) ? qcol[(size_t)s1 * S] : 0.f;
            post0 = v0 ? logf(fa + D3PM_EPS) + logf(f2a + D3PM_EPS) : -INFINITY;
            post1 = v1 ? logf(fb + D3PM_EPS) + logf(f2b + D3PM_EPS) : -INFINITY;
        }
    }
    // ---- Gumbel arg-max (d3pm.py:206-214) ----------------------------------------------------------
    const float scale = (t != 1) ? 1.0f : 0.2f;
    // (the array-or-generator choice is made on the kernel argument itself -- a scalar compare -- not on a per-lane pointer:
    // no per-lane 64-bit integer compares on this path)
    const bool have_u = u_types != nullptr;
    const float* un = u_types + (have_u ? (size_t)i * S : 0);
    auto draw_u = [&](int s_) {
        return have_u ? un[s_] : philox_uniform(dk.seed, (uint32_t)t, ARREAU_DRAW_U_TYPES, dk.atom * (uint32_t)S + (uint32_t)s_, word3);
    };
    float best = -INFINITY;
    int besti = 0x7fffffff;
    if (v0) {
        const float u = fminf(fmaxf(draw_u(s0), D3PM_EPS), 1.0f);
        best = post0 + (-logf(-logf(u))) * scale;
        besti = s0;
    }
    if (v1) {
        const float u = fminf(fmaxf(draw_u(s1), D3PM_EPS), 1.0f);
        const float val = post1 + (-logf(-logf(u))) * scale;
        if (val > best) { best = val; besti = s1; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(besti, off, 64);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }  // first index wins ties
    }
    // use_constant_atomic_symbols (lightning_wrappers/diffusion.py:231-236): the fixed species are re-imposed each step
    // conditioned sampling, rule 4: a known species is re-imposed the same way, per atom
    if (lane == 0) types[i] = (cond && cond->type_mask && cond->type_mask[i]) ? cond->a0[i] : (const_types ? const_types[i] : besti);
}

// the form the stand-alone kernel uses: workgroup `blk` of four waves, one atom each
template <bool ETA, bool MS = false, bool SPEC = false>
__device__ __forceinline__ void reverse_atoms_body(
    int blk /* block of the atom part */, float* __restrict__ frac, int32_t* __restrict__ types, const int32_t* __restrict__ tstep,
    const int32_t* __restrict__ offsets, int B, int N, const float* __restrict__ eps,
    const float* __restrict__ logits, StepNoiseSrc noise,
    const float* __restrict__ ve_sigmas, const float* __restrict__ q1t, const float* __restrict__ qmats, int S,
    int T, const int32_t* __restrict__ const_types, int absorbing, int32_t* __restrict__ status, int n0,
    const int32_t* __restrict__ batch, const SampleConditionDev* cond, const StepScheduleDev* sched, uint32_t word3, float eta,
    const arreau_multistep& ms = {} /* MS only */, const arreau_species_control& sp = {} /* SPEC only */) {
    const int i = n0 + blk * 4 + (int)(threadIdx.x >> 6);  // atoms n0 .. N-1
    if (i >= N) return;  // wave-uniform; no block-level barrier below
    reverse_one_atom<ETA, MS, SPEC>(i, threadIdx.x & 63, frac, types, tstep, offsets, B, eps, logits, noise, ve_sigmas, q1t, qmats, S, T,
                                    const_types, absorbing, status, batch, cond, sched, word3, eta, ms, sp);
}

// ---- space-group symmetry (arreau_sample_loop_sym / arreau_reverse_step_sym; rules in include/arreau_hip.h) -----------------
// Crystal of atom i: the caller's index, or the 64-ary search of reverse_one_atom.  (Also the INVERT atom part's.)
__device__ __forceinline__ int sym_atom_crystal(int i, int lane, const int32_t* __restrict__ offsets, int B, const int32_t* __restrict__ batch) {
    if (batch != nullptr) return batch[i];
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int span = hi - lo, step = (span + 63) >> 6;
        const int probe = lo + lane * step;
        const bool le = probe < hi && offsets[probe] <= i;
        const int c = __builtin_popcountll(__ballot(le));
        lo = lo + (c - 1) * step;
        hi = min(lo + step, hi);
    }
    return lo;
}

// The tables of orbit o, led by atom i of the crystal [first, last), before any of them is followed: its CSR ranges in bounds
// and non-empty, every member in the crystal, naming i as its leader and with an operation row in range, i among the members,
// every stabilizer row in range.  Whole wave (o is wave-uniform); false: the orbit is rejected (the caller flags it).
__device__ __forceinline__ bool sym_orbit_ok(const arreau_symmetry& sy, int i, int o, int first, int last, int lane) {
    if (o < 0 || o >= sy.n_orbits) return false;
    const int a0 = sy.orbit_ptr[o], a1 = sy.orbit_ptr[o + 1], h0 = sy.stab_ptr[o], h1 = sy.stab_ptr[o + 1];
    if (!(a0 >= 0 && a0 < a1 && a1 <= sy.n_orbit_atoms && h0 >= 0 && h0 < h1 && h1 <= sy.n_stab_ops)) return false;
    bool bad = false, self = false;
    for (int a = a0 + lane; a < a1; a += 64) {
        const int j = sy.orbit_atoms[a];
        if (j < first || j >= last) { bad = true; continue; }
        const int k = sy.op[j];
        bad |= sy.leader[j] != i || k < 0 || k >= sy.n_ops;
        self |= j == i;
    }
    for (int h = h0 + lane; h < h1; h += 64) {
        const int k = sy.stab_ops[h];
        bad |= k < 0 || k >= sy.n_ops;
    }
    return __ballot(bad) == 0 && __ballot(self) != 0;
}

// philox_normal (philox.h) with word3 = 0, forced inline: the SYM instances hold a second copy of the position update (the
// unconstrained atoms' reverse_one_atom), past the inliner's budget for philox_normal.
__device__ __forceinline__ float sym_philox_normal(uint64_t seed, uint32_t timestep, uint32_t kind, uint32_t element) {
    const Philox4 r = philox4x32_10(element, timestep, kind, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = ((float)(r.x[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    const float u2 = (float)(r.x[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

__device__ __forceinline__ float sym_lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The SYM form of reverse_atoms_body: one wave per atom.  An unconstrained atom (leader -1) runs reverse_one_atom as the plain
// kernel does; a member leaves (its leader's wave writes it); a leader updates its whole orbit (rules 1-5).
// SPEC: species control -- the orbit's one class is drawn by d3pm_reverse_class<true> on the orbit's mean logits, the leader's
// draw and its crystal's row; an unconstrained atom runs reverse_one_atom's SPEC instance.
template <bool SPEC = false>
__device__ __forceinline__ void reverse_atoms_body_sym(
    int blk, float* __restrict__ frac, int32_t* __restrict__ types, const int32_t* __restrict__ tstep, const int32_t* __restrict__ offsets,
    int B, int N, const float* __restrict__ eps, const float* __restrict__ logits, StepNoiseSrc noise, const float* __restrict__ ve_sigmas,
    const float* __restrict__ q1t, const float* __restrict__ qmats, int S, int T, const int32_t* __restrict__ const_types, int absorbing,
    int32_t* __restrict__ status, int n0, const int32_t* __restrict__ batch, const StepScheduleDev* sched, const arreau_symmetry& sy,
    const arreau_species_control& sp = {} /* SPEC only */) {
    const int i = n0 + blk * 4 + (int)(threadIdx.x >> 6);
    if (i >= N) return;  // wave-uniform; no block-level barrier below
    const int lane = threadIdx.x & 63;
    int lead = sy.leader[i];
    if (lead != -1 && (lead < 0 || lead >= N || sy.leader[lead] != lead)) {  // a leader out of range, or one that does not lead
        if (lane == 0) atomicOr(status, ARREAU_STATUS_BAD_SYMMETRY);
        lead = -1;
    }
    if (lead >= 0 && lead != i) return;  // a member: written by its leader's wave
    int b = 0, o = -1;
    bool orbit_ok = false;
    DrawKey dk{noise.seed, (uint32_t)i};
    if (lead == i) {
        b = sym_atom_crystal(i, lane, offsets, B, batch);
        dk = atom_draw_key(noise, offsets, b, i);  // (keyed sampling: the leader's draws, keyed within its crystal)
        o = sy.orbit[i];
        orbit_ok = sym_orbit_ok(sy, i, o, offsets[b], offsets[b + 1], lane);
        if (!orbit_ok && lane == 0) atomicOr(status, ARREAU_STATUS_BAD_SYMMETRY);
    }
    if (!orbit_ok) {  // rule 7: unconstrained (or a rejected orbit's leader alone)
        if constexpr (SPEC)
            reverse_one_atom<false, false, true>(i, lane, frac, types, tstep, offsets, B, eps, logits, noise, ve_sigmas, q1t, qmats, S, T,
                                                 const_types, absorbing, status, batch, nullptr, sched, 0u, 0.0f, {}, sp);
        else
            reverse_one_atom(i, lane, frac, types, tstep, offsets, B, eps, logits, noise, ve_sigmas, q1t, qmats, S, T, const_types, absorbing,
                             status, batch, nullptr, sched, 0u);
        return;
    }
    int t = tstep[b];
    t = t < 1 ? 1 : (t > T ? T : t);
    const int s_to = step_target(sched, b, t, status, false);  // (flagged by the crystal's lattice thread)
    const int a0 = sy.orbit_ptr[o], a1 = sy.orbit_ptr[o + 1], h0 = sy.stab_ptr[o], h1 = sy.stab_ptr[o + 1];
    const float inv_o = 1.0f / (float)(a1 - a0);
    // rules 1-2, lane d < 3 owns component d: the pulled-back mean noise, then the leader's VE reverse update without the wrap
    float y = 0.f, xc = 0.f;
    if (lane < 3) {
        float acc = 0.f;
        for (int a = a0; a < a1; ++a) {
            const int j = sy.orbit_atoms[a];
            const float* Ri = sy.rot_inv + 9 * (size_t)sy.op[j] + 3 * lane;
            const float* e = eps + 3 * (size_t)j;
            acc += Ri[0] * e[0] + Ri[1] * e[1] + Ri[2] * e[2];
        }
        const float ebar = acc * inv_o;
        const float sg = ve_sigmas[t], sp = ve_sigmas[s_to];
        const float s2 = sg * sg, sp2 = sp * sp;
        const size_t g = 3 * (size_t)i + lane;
        xc = frac[g];
        const float mean = xc - ebar * (s2 - sp2);
        const float stdv = sqrtf((sp2 * (s2 - sp2)) / s2);
        const float zf = noise.z_frac ? noise.z_frac[g] : sym_philox_normal(dk.seed, (uint32_t)t, ARREAU_DRAW_Z_FRAC, 3u * dk.atom + (uint32_t)lane);
        y = mean + stdv * zf;
    }
    const float ys[3] = {sym_lane_value(y, 0), sym_lane_value(y, 1), sym_lane_value(y, 2)};
    const float xs[3] = {sym_lane_value(xc, 0), sym_lane_value(xc, 1), sym_lane_value(xc, 2)};
    // rule 3: onto the site, anchored at the current position
    float xn = 0.f;
    if (lane < 3) {
        if (h1 - h0 == 1) {
            xn = remainder_one(y);
        } else {
            float acc = 0.f;
            for (int h = h0; h < h1; ++h) {
                const int k = sy.stab_ops[h];
                const float* R = sy.rot + 9 * (size_t)k + 3 * lane;
                const float tk = sy.trans[3 * (size_t)k + lane];
                const float n = rintf(xc - (R[0] * xs[0] + R[1] * xs[1] + R[2] * xs[2]) - tk);
                acc += ((R[0] * ys[0] + R[1] * ys[1] + R[2] * ys[2]) + tk) + n;
            }
            xn = remainder_one(acc / (float)(h1 - h0));
        }
    }
    const float xl[3] = {sym_lane_value(xn, 0), sym_lane_value(xn, 1), sym_lane_value(xn, 2)};
    // rule 5 (before any write): the orbit's mean logits, the leader's draw
    const int s0 = lane, s1 = lane + 64;
    const bool v0 = s0 < S, v1 = s1 < S;
    float l0 = 0.f, l1 = 0.f;
    for (int a = a0; a < a1; ++a) {
        const float* lg = logits + (size_t)sy.orbit_atoms[a] * S;
        if (v0) l0 += lg[s0];
        if (v1) l1 += lg[s1];
    }
    l0 = v0 ? l0 * inv_o : -INFINITY;
    l1 = v1 ? l1 * inv_o : -INFINITY;
    const int cls = d3pm_reverse_class<SPEC>(i, lane, l0, l1, t, s_to, types, noise, q1t, qmats, S, absorbing, status, sched, 0u, dk, b, sp);
    const int newt = const_types ? const_types[i] : cls;
    // rule 4 and the members' species: lanes over the members
    for (int a = a0 + lane; a < a1; a += 64) {
        const int j = sy.orbit_atoms[a];
        float* fj = frac + 3 * (size_t)j;
        if (j == i) {
            fj[0] = xl[0]; fj[1] = xl[1]; fj[2] = xl[2];
        } else {
            const int k = sy.op[j];
            const float* R = sy.rot + 9 * (size_t)k;
            const float* tk = sy.trans + 3 * (size_t)k;
#pragma unroll
            for (int c = 0; c < 3; ++c) fj[c] = remainder_one((R[3 * c] * xl[0] + R[3 * c + 1] * xl[1] + R[3 * c + 2] * xl[2]) + tk[c]);
        }
        types[j] = newt;
    }
}

// The INVERT form of reverse_atoms_body: one wave per atom, the position move from the crystal's level up to its target and
// nothing else -- the species are the caller's at every level, so neither `types` nor the logits are touched and the D3PM half
// is not instantiated.  (The clamps are flagged by the crystal's lattice thread.)
__device__ __forceinline__ void invert_atoms_body(int blk, float* __restrict__ frac, const int32_t* __restrict__ tstep,
                                                  const int32_t* __restrict__ offsets, int B, int N, const float* __restrict__ eps,
                                                  const float* __restrict__ ve_sigmas, int T, int32_t* __restrict__ status, int n0,
                                                  const int32_t* __restrict__ batch, const StepScheduleDev* sched) {
    const int i = n0 + blk * 4 + (int)(threadIdx.x >> 6);  // atoms n0 .. N-1
    if (i >= N) return;  // wave-uniform; no block-level barrier below
    const int lane = threadIdx.x & 63;
    const int b = sym_atom_crystal(i, lane, offsets, B, batch);
    const int s = invert_level(tstep[b], T, status, false);
    const int t = invert_target(sched, b, s, T, status, false);
    if (lane < 3) {
        const size_t g = 3 * (size_t)i + lane;
        frac[g] = invert_frac_move(frac[g], eps[g], ve_sigmas[s], ve_sigmas[t]);
    }
}

// The LDS of an MS crystal block: the crystal's three history values and, as bits, its history level.
template <bool MS>
__device__ __forceinline__ float* ms_block_lds() {
    if constexpr (MS) {
        __shared__ float v[4];
        return v;
    } else {
        return nullptr;
    }
}

// Sampling loop (round 3): the lattice update of a crystal by ONE workgroup that then also prepares the crystal's NEXT step --
// what prep_kernel (node.hip) would compute at the top of that step from the lengths just written: the cell (into the
// caller's lattice AND the workspace copy the network reads) and the per-crystal part of the embedding for timestep t - 1 (the
// scheduled successor of t in a respaced loop).
// The step then needs no prep launch (the Cartesian positions, prep's other product, are formed by the neighbour-list waves
// from the fractional coordinates).  Same arithmetic as reverse_lattice_body + prep_kernel, thread for thread.
// TIE: the lattice-system tie of the lengths (length_tie[b]); the three x0 and current lengths are exchanged through LDS.
// ETA: the eta move of the lengths.
// INVERT: the inversion move of the lengths, from the crystal's level up to its target (not with TIE or ETA); the step prepared
// is the one at the target, the HIGHER level.
// MS: the multistep move of the lengths (with ETA, eta = 0); thread 0 reads the crystal's history level, hands it on through LDS
// and overwrites it.
template <bool TIE, bool ETA, bool INVERT = false, bool MS = false>
__device__ __forceinline__ void reverse_crystal_block(int b, float* __restrict__ lengths, const float* __restrict__ angles,
                                                      const int32_t* __restrict__ tstep, const int32_t* __restrict__ offsets,
                                                      const float* __restrict__ len0, StepNoiseSrc noise,
                                                      const float* __restrict__ alpha_bars, const float* __restrict__ betas, int T,
                                                      float* __restrict__ lattice, const float* __restrict__ fixed_lengths,
                                                      int32_t* __restrict__ status, const float* __restrict__ gs_atoms,
                                                      float* __restrict__ len0_out, float* __restrict__ lattice_ws,
                                                      float* __restrict__ cvec_next, const float* __restrict__ t_emb_w,
                                                      const float* __restrict__ embT, int S, int C, const SampleConditionDev* cond,
                                                      const StepScheduleDev* sched, uint32_t word3, const int32_t* __restrict__ length_tie,
                                                      float eta, const arreau_multistep& ms = {} /* MS only */) {
    __shared__ float newlen[3];
    __shared__ float feat[ARREAU_T_EMB_DIM + ARREAU_N_CRYSTAL_FEATS];
    const int t_raw = tstep[b];
    int t, s;
    if constexpr (INVERT) {
        static_assert(!TIE && !ETA, "the INVERT instances are untied and take no eta");
        t = invert_level(t_raw, T, status, threadIdx.x == 0);
        s = invert_target(sched, b, t, T, status, threadIdx.x == 0);
    } else {
        if (threadIdx.x == 0 && (t_raw < 1 || t_raw > T)) atomicOr(status, ARREAU_STATUS_BAD_TIMESTEP);  // clamped, but flagged
        t = t_raw < 1 ? 1 : (t_raw > T ? T : t_raw);
        s = step_target(sched, b, t, status, threadIdx.x == 0);
    }
    const int first = offsets[b], last = offsets[b + 1];
    float* const x0ps = ms_block_lds<MS>();  // (the other instances allocate nothing)
    int hist_level = 0;
    if constexpr (MS) {
        static_assert(ETA && !INVERT, "the MS instances are ETA instances (at eta = 0)");
        if (threadIdx.x < 3) x0ps[threadIdx.x] = ms.hist_x0[3 * b + threadIdx.x];
        if (threadIdx.x == 0) x0ps[3] = __int_as_float(ms.hist_t_len[b]);
        __syncthreads();
        hist_level = __float_as_int(x0ps[3]);
    }
    if constexpr (TIE) {
        __shared__ float x0s[3], xts[3];
        const int code = length_tie_code(length_tie, cond ? cond->len_mask : nullptr, b, status, threadIdx.x == 0);
        if (threadIdx.x < 3) {
            x0s[threadIdx.x] = length_x0_component(b, threadIdx.x, first, last, len0, gs_atoms, len0_out);
            xts[threadIdx.x] = lengths[3 * b + threadIdx.x];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            if constexpr (MS)
                newlen[threadIdx.x] = tied_length_component<ETA, true>(b, threadIdx.x, code, x0s, xts, t, s, sched, lengths, noise, alpha_bars,
                                                                       betas, fixed_lengths, cond, word3, eta, ms, x0ps, hist_level, T);
            else
                newlen[threadIdx.x] = tied_length_component<ETA>(b, threadIdx.x, code, x0s, xts, t, s, sched, lengths, noise, alpha_bars, betas,
                                                                 fixed_lengths, cond, word3, eta);
        }
    } else {
        if (threadIdx.x < 3) {
            if constexpr (MS)
                newlen[threadIdx.x] = reverse_length_component<ETA, false, true>(b, threadIdx.x, t, s, sched, first, last, lengths, len0, noise,
                                                                                 alpha_bars, betas, fixed_lengths, gs_atoms, len0_out, cond, word3,
                                                                                 eta, ms, hist_level, T);
            else
                newlen[threadIdx.x] = reverse_length_component<ETA, INVERT>(b, threadIdx.x, t, s, sched, first, last, lengths, len0, noise,
                                                                            alpha_bars, betas, fixed_lengths, gs_atoms, len0_out, cond, word3, eta);
        }
    }
    __syncthreads();
    if constexpr (MS) {
        if (threadIdx.x == 0) ms.hist_t_len[b] = t;
    }
    const float* ang = angles + 3 * b;
    if (threadIdx.x == 0) {
        float Lm[9];
        arreau_prep_cell(newlen, ang, Lm);  // lattice_from_params (lattice_helpers.py:55-105)
#pragma unroll
        for (int q = 0; q < 9; ++q) { lattice[9 * b + q] = Lm[q]; lattice_ws[9 * b + q] = Lm[q]; }
    }
    arreau_prep_cvec(sched ? s : t_raw - 1, last - first, newlen, ang, betas, t_emb_w, embT, S, C, T, feat, cvec_next + (size_t)b * C, status);
}

