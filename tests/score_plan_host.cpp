// Host driver of csrc/score_plan.h for tests/test_score_plan_cpu.py: no HIP, no device.  Reads one row per line from stdin,
// "key=value" tokens that override the defaults below (inputs of the flagship model on a 256-CU chip, every switch unset, N = 100),
// and prints the plan of each row, the codes arreau_model_status would report for it, and whether it equals the previous row's plan.
// The token "none" prints the all-zero plan (no evaluation yet) instead.
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../arreau_amd/csrc/score_plan.h"

int main() {
    static const char* edge[] = {"none", "fp32", "bf16x6", "f16x3"};
    static const char* form[] = {"persistent", "split"};
    static const char* message[] = {"register", "streamed", "basis_proj", "small_layer"};
    static const char* mlp[] = {"fp32", "bf16x6", "f16x3_tile", "f16x3_split", "small_layer"};
    static const char* readout[] = {"vector", "mfma", "mfma_split"};
    ScorePlan prev{};
    std::string line;
    while (std::getline(std::cin, line)) {
        ScorePlanInputs in{1, 128, 256, 512, 2, 8, 90, 1, 1, 1, 0, 4, 3, 2, 1, 256};
        ScoreSwitches sw;
        int N = 100, none = 0;
        const std::map<std::string, int*> ints = {
            {"fused", &in.fused}, {"C", &in.C}, {"D", &in.D}, {"H", &in.H}, {"L", &in.L}, {"k", &in.k}, {"S", &in.S},
            {"f16_ok", &in.f16_ok}, {"fp8_ok", &in.fp8_ok}, {"x8_ok", &in.x8_ok}, {"calibrating", &in.calibrating},
            {"edge_variant", &in.edge_variant}, {"mlp_variant", &in.mlp_variant}, {"conv_variant", &in.conv_variant},
            {"readout_variant", &in.readout_variant}, {"n_cu", &in.n_cu}, {"N", &N},
            {"BASIS_FP8", &sw.basis_fp8}, {"EDGE_WGS", &sw.edge_wgs}, {"EDGE_SPLIT", &sw.edge_split}, {"MLP_SPLIT", &sw.mlp_split},
            {"MLP_NB", &sw.mlp_nb}, {"MLP_SLOTS", &sw.mlp_slots}, {"READOUT_SPLIT", &sw.readout_split},
            {"CONV_PROJ_BOUSTROPHEDON", &sw.boustrophedon}, {"BASIS_MIN_RECEIVERS", &sw.basis_min_receivers}};
        const std::map<std::string, bool*> bools = {{"CROSS_FP8", &sw.cross_fp8}, {"FUSE_SMALL", &sw.fuse_small}, {"LOOP_PREP", &sw.loop_prep}};
        std::istringstream tokens(line);
        std::string tok;
        while (tokens >> tok) {
            const size_t eq = tok.find('=');
            const std::string key = tok.substr(0, eq);
            const int value = eq == std::string::npos ? 1 : atoi(tok.c_str() + eq + 1);
            if (key == "none") none = 1;
            else if (ints.count(key)) *ints.at(key) = value;
            else if (bools.count(key)) *bools.at(key) = value != 0;
            else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        const ScorePlan p = none ? ScorePlan{} : score_plan(in, sw, N);
        const ScorePlanCodes c = score_plan_codes(p);
        printf("general=%d edge=%s form=%s wgs=%d basis_form=%d basis_fp8=%d cross_fp8=%d message=%s boustrophedon=%d mlp=%s nb=%d slots=%d "
               "readout=%s no_prep=%d codes=%d/%d/%d/%d/%d/%d same_as_previous=%d\n",
               p.general, edge[p.edge], form[p.edge_form], p.edge_wgs, p.basis_form, p.basis_fp8, p.cross_fp8, message[p.message],
               p.boustrophedon, mlp[p.mlp], p.mlp_nb, p.mlp_slots, readout[p.readout], p.no_prep, c.edge_kernel, c.mlp_kernel,
               c.conv_kernel, c.readout_kernel, c.basis_row_bytes, c.conv_cross_fp8, p == prev);
        prev = p;
    }
    return 0;
}
