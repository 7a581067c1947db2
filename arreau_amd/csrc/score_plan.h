// The launch plan of one evaluation of the score network: which kernel, which form of it and which operand formats every launch of
// arreau_predict_scores, arreau_ponita_forward and a step of the sampling loop uses.  The entry points build it once per call; the
// launchers execute it.  Plain C++, no HIP: tests/test_score_plan_cpu.py checks every threshold with a host compiler.
#pragma once
#include <stdint.h>
#include <stdlib.h>

// Every environment switch of the score path.  score_switches() is the one place they are read.
struct ScoreSwitches {
    // read once per process; -1 = unset where the default depends on the launch
    int basis_fp8 = -1;      // ARREAU_BASIS_FP8: 0 / 1 overrides the model's calibrated choice of the stash's residual plane
    int edge_wgs = 0;        // ARREAU_EDGE_WGS: workgroups of the persistent fp16x3 edge kernel (0: one per CU)
    int edge_split = -1;     // ARREAU_EDGE_SPLIT: 0 / 1 forces the persistent / tile-per-workgroup form
    int mlp_split = -1;      // ARREAU_MLP_SPLIT: 0 / 1 forces the tile / node-per-workgroup ConvNext form; set: no small layer
    int mlp_nb = 0;          // ARREAU_MLP_NB: 1 / 2 forces the nodes per wave of the tile form
    int mlp_slots = 3;       // ARREAU_MLP_SLOTS: 4 selects the four-slot weight ring
    int readout_split = -1;  // ARREAU_READOUT_SPLIT: 0 / 1 forces the read-out's form
    int boustrophedon = 1;   // ARREAU_CONV_PROJ_BOUSTROPHEDON: 0 = every message pass reads the stash front to back
    // read per library call (the tests change them inside one process)
    int basis_min_receivers = 2000;  // ARREAU_BASIS_MIN_RECEIVERS: the basis form takes over above this many receivers
    bool cross_fp8 = true;           // ARREAU_CROSS_FP8: 0 keeps three fp16 cross products
    bool fuse_small = true;          // ARREAU_FUSE_SMALL: 0 = two launches per layer also for small launches
    bool loop_prep = false;          // ARREAU_LOOP_PREP: 1 keeps the prep launch in every step of the sampling loop
};

inline ScoreSwitches score_switches() {
    auto env = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    static const ScoreSwitches process{
        .basis_fp8 = env("ARREAU_BASIS_FP8", -1), .edge_wgs = env("ARREAU_EDGE_WGS", 0), .edge_split = env("ARREAU_EDGE_SPLIT", -1),
        .mlp_split = env("ARREAU_MLP_SPLIT", -1), .mlp_nb = env("ARREAU_MLP_NB", 0), .mlp_slots = env("ARREAU_MLP_SLOTS", 3),
        .readout_split = env("ARREAU_READOUT_SPLIT", -1), .boustrophedon = env("ARREAU_CONV_PROJ_BOUSTROPHEDON", 1)};
    ScoreSwitches w = process;
    w.basis_min_receivers = env("ARREAU_BASIS_MIN_RECEIVERS", 2000), w.cross_fp8 = env("ARREAU_CROSS_FP8", 1) != 0;
    w.fuse_small = env("ARREAU_FUSE_SMALL", 1) != 0, w.loop_prep = env("ARREAU_LOOP_PREP", 0) != 0;
    return w;
}

// What the decision reads from the model (internal.h: arreau_model) and the machine.
struct ScorePlanInputs {
    int fused, C, D, H, L, k, S;
    int f16_ok, fp8_ok, x8_ok, calibrating;
    int edge_variant, mlp_variant, conv_variant, readout_variant;  // as requested: ARREAU_*_VARIANT, arreau_model_set_variant
    int n_cu;
};

#define ARREAU_VARIANT_GENERAL 5  // edge_variant value that selects the shape-general fp32 network for the whole evaluation

// The all-zero plan is "no evaluation yet" (a real one is general or names an edge kernel): arreau_model_create zero-fills the model.
struct ScorePlan {
    enum Edge : int32_t { EDGE_NONE, EDGE_FP32, EDGE_BF16X6, EDGE_F16X3 };
    enum EdgeForm : int32_t { EDGE_PERSISTENT, EDGE_SPLIT };
    enum Message : int32_t { MSG_REGISTER, MSG_STREAMED, MSG_BASIS_PROJ, MSG_IN_SMALL_LAYER };
    enum Mlp : int32_t { MLP_FP32, MLP_BF16X6, MLP_F16X3_TILE, MLP_F16X3_SPLIT, MLP_SMALL_LAYER };
    enum Readout : int32_t { RO_VECTOR, RO_MFMA, RO_MFMA_SPLIT };
    bool general;  // train_net.hip's fp32 kernels run everything; the other members stay zero
    Edge edge;
    EdgeForm edge_form;  // of the fp16x3 kernel
    int32_t edge_wgs;    // workgroups of its persistent form (0 otherwise)
    // basis_form: the edge kernel stores the windowed basis planes and each layer's message kernel projects them (conv_proj.hip);
    // otherwise the K pair.  basis_fp8: the basis' residual plane is rounded to fp8 e4m3, by every fp16x3 edge kernel, so that all
    // launch sizes evaluate the same numbers.  cross_fp8: the projection's two cross products on the fp8 matrix instruction.
    bool basis_form, basis_fp8, cross_fp8;
    Message message;
    bool boustrophedon;  // of the basis projection: even layers read the stash back to front
    Mlp mlp;
    int32_t mlp_nb, mlp_slots;  // of the tile form: nodes per wave, ring depth (0 otherwise)
    Readout readout;
    bool no_prep;  // sampling loop: no prep launch per step
    bool operator==(const ScorePlan&) const = default;
};

inline ScorePlan score_plan(const ScorePlanInputs& in, const ScoreSwitches& sw, int N) {
    if (!in.fused || in.edge_variant == ARREAU_VARIANT_GENERAL) return ScorePlan{.general = true};
    ScorePlan p{};
    const bool f16 = in.f16_ok != 0;
    // edge kernel: 4 = fp16x3 (edge_f16.hip; needs weights that fit fp16), 3 = bf16x6 (edge_bf16.hip), below = fp32 MFMA (edge.hip)
    p.edge = in.edge_variant == 4 && f16 ? ScorePlan::EDGE_F16X3 : in.edge_variant >= 3 ? ScorePlan::EDGE_BF16X6 : ScorePlan::EDGE_FP32;
    // Basis form (conv variant 2, the default) where it applies and the launch is large enough for it to pay.  Measured at n = 20,
    // basis form / K pair, ms per step: 960 receivers 0.436 / 0.421, 1920: 0.655 / 0.656, 2560: 0.852 / 0.870, 5120: 1.35 / 1.48,
    // so it takes over from 2,000; never below 240 (the tests set that; the calibration runs the basis form on 320 receivers).
    // (L >= 2: the stash, 96 or 128 KiB per atom, lives in the workspace region sized for L kernel buffers of 64 KiB per atom)
    const int min_receivers = sw.basis_min_receivers > 240 && !in.calibrating ? sw.basis_min_receivers : 240;
    p.basis_form = in.conv_variant == 2 && in.edge_variant == 4 && f16 && in.k == 8 && in.C == 128 && in.D == 256 && in.L >= 2 &&
                   N > min_receivers;
    // (the environment overrides the model's calibration either way, except while that calibration runs)
    p.basis_fp8 = sw.basis_fp8 >= 0 && !in.calibrating ? sw.basis_fp8 != 0 : in.fp8_ok != 0;
    p.cross_fp8 = (sw.cross_fp8 || in.calibrating) && in.x8_ok && p.basis_fp8;
    if (p.edge == ScorePlan::EDGE_F16X3) {
        // small launches: one tile per workgroup (bit-identical K tiles; the persistent form is one wave's latency, 62 us at 1 x 8)
        const bool split = in.L >= 2 && in.L <= 6 && !p.basis_form && (sw.edge_split >= 0 ? sw.edge_split != 0 : N <= 240);
        p.edge_form = split ? ScorePlan::EDGE_SPLIT : ScorePlan::EDGE_PERSISTENT;
        const int pairs = (N + 1) / 2, most = sw.edge_wgs > 0 ? sw.edge_wgs : in.n_cu;
        if (!split) p.edge_wgs = pairs < most ? pairs : most;
    }
    const bool streamed = (in.conv_variant == 1 || in.conv_variant == 2) && in.k == 8;  // (2 without the basis form = the streamed K pair)
    p.message = p.basis_form ? ScorePlan::MSG_BASIS_PROJ : streamed ? ScorePlan::MSG_STREAMED : ScorePlan::MSG_REGISTER;
    p.boustrophedon = sw.boustrophedon != 0;
    // ConvNext block: 3 = fp16x3 (node_f16m.hip), 4 = always its node-per-workgroup form, 1 and 2 = bf16x6, 0 = fp32 MFMA.  Variant 3
    // picks the form by size: one node per workgroup takes 10.7 us per layer at 8 nodes against 22.5, and loses past two rounds of the chip.
    const bool mlp_split = sw.mlp_split >= 0 ? sw.mlp_split != 0 : N <= 512;
    if (sw.fuse_small && sw.mlp_split < 0 && N <= 512 && in.mlp_variant == 3 && f16 && streamed && in.C == 128 && in.H == 512 &&
        !p.basis_form) {
        // small launch on the K pair: the streamed message kernel and the split ConvNext form in one launch (bit-identical)
        p.mlp = ScorePlan::MLP_SMALL_LAYER;
        p.message = ScorePlan::MSG_IN_SMALL_LAYER;
    } else if ((in.mlp_variant == 4 && f16) || (in.mlp_variant == 3 && f16 && mlp_split)) {
        p.mlp = ScorePlan::MLP_F16X3_SPLIT;
    } else if (in.mlp_variant == 3 && f16) {
        // one wave = 2 nodes, or 1 node (twice the tiles, 0.6 of the time each): whichever takes cheaper rounds over the chip's wave
        // slots (2 workgroups x 4 waves per CU).  The four-slot ring measured no gain (256 x 20: 1.77 vs 1.77 ms per step).
        const long long slots = 8LL * in.n_cu;
        const long long rounds1 = (N + slots - 1) / slots, rounds2 = ((N + 1LL) / 2 + slots - 1) / slots;
        p.mlp = ScorePlan::MLP_F16X3_TILE;
        p.mlp_nb = sw.mlp_nb == 1 || sw.mlp_nb == 2 ? sw.mlp_nb : 6 * rounds1 < 10 * rounds2 ? 1 : 2;
        p.mlp_slots = sw.mlp_slots == 4 ? 4 : 3;
    } else {
        p.mlp = in.mlp_variant >= 1 ? ScorePlan::MLP_BF16X6 : ScorePlan::MLP_FP32;
    }
    // Read-out on the fp32 matrix pipe (variant 1) where its tiles fit, one workgroup per output tile while the launch has fewer
    // workgroups than the chip has CUs (160 workgroups: 18.7 us split against 21.6; 640: 75 against 65); else the vector kernel.
    if (in.readout_variant == 1 && in.S + 4 <= 96 && in.L <= 8 && in.C == 128)
        p.readout = (sw.readout_split >= 0 ? sw.readout_split != 0 : (N + 31) / 32 < 256) ? ScorePlan::RO_MFMA_SPLIT : ScorePlan::RO_MFMA;
    p.no_prep = !sw.loop_prep;  // (api.hip: enqueue_sample_step)
    return p;
}

// What arreau_model_status reports of a plan (include/arreau_hip.h: arreau_status); -1 / 0 before the first evaluation.
struct ScorePlanCodes { int edge_kernel, mlp_kernel, conv_kernel, readout_kernel, basis_row_bytes, conv_cross_fp8; };
inline ScorePlanCodes score_plan_codes(const ScorePlan& p) {
    if (p.general) return {ARREAU_VARIANT_GENERAL, ARREAU_VARIANT_GENERAL, ARREAU_VARIANT_GENERAL, ARREAU_VARIANT_GENERAL, 0, 0};
    if (p.edge == ScorePlan::EDGE_NONE) return {-1, -1, -1, -1, 0, 0};
    const bool proj = p.message == ScorePlan::MSG_BASIS_PROJ;
    return {p.edge == ScorePlan::EDGE_F16X3 ? 4 : p.edge == ScorePlan::EDGE_BF16X6 ? 3 : 0,
            p.mlp >= ScorePlan::MLP_F16X3_TILE ? 3 : p.mlp == ScorePlan::MLP_BF16X6 ? 1 : 0, proj ? 2 : p.message == ScorePlan::MSG_REGISTER ? 0 : 1,
            p.readout == ScorePlan::RO_VECTOR ? 0 : 1, proj ? (p.basis_fp8 ? 768 : 1024) : 0, proj && p.cross_fp8 ? 1 : 0};
}
