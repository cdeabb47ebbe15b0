// tools/stage_plan_sweep.cpp -- the stage planner (cat_amd/csrc/stage_plan.cpp) under a host sanitizer: a stand-alone program, no GPU, no HIP call.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D_GLIBCXX_ASSERTIONS -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/stage_plan_sweep.cpp cat_amd/csrc/stage_plan.cpp cat_amd/csrc/crf_opts.cpp -o stage_plan_sweep && ./stage_plan_sweep
// (-D_GLIBCXX_ASSERTIONS: std::array's operator[] checks its index, so a write past one array INSIDE a plan is caught too.)
// Sweeps T = 1 .. 4096 and B in {1, 80, 96} under every switch setting of tests/test_stage_plan.py's CASES plus segments = 1 and
// gd_stage_launches = 1, plans the way plan_schedule and launch_grad_den do, and checks: nstage <= kMaxStages - 1, bound strictly
// increasing from 0 to T, poff non-decreasing.  tests/test_stage_plan_sanitized.py builds and runs it.  Exit status 0 and one line: all held.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../cat_amd/csrc/stage_plan.h"
#include "../include/ctc_crf_hip.h"

using Case = std::vector<std::pair<const char *, int>>;

static void fail(const char *what, const Case &c, long T, long B) {
    fprintf(stderr, "stage_plan_sweep: %s at T = %ld, B = %ld under", what, T, B);
    for (const auto &kv : c) fprintf(stderr, " %s=%d", kv.first, kv.second);
    fprintf(stderr, "\n");
    exit(1);
}

int main() {
    using namespace crf;
    const std::vector<Case> cases = {
        {}, {{"piece", 48}}, {{"piece", 64}}, {{"piece", 96}}, {{"piece", 128}, {"taper", 0}}, {{"taper", 16}}, {{"taper", 64}}, {{"piece", 112}, {"taper", 48}},
        {{"gd_sub", 8}}, {{"gd_sub", 4}, {"piece", 64}}, {{"gd_sub", 2}, {"taper", 16}}, {{"first_shift", 3}}, {{"stages", 5}},
        {{"segments", 1}}, {{"gd_stage_launches", 1}}};
    long plans = 0;
    for (const Case &c : cases) {
        bool segmode = false, per_stage = false;
        int stages_env = 0;
        for (const auto &kv : c) {
            if (crf_debug_set(kv.first, kv.second) != CRF_OK) fail("unknown switch", c, 0, 0);
            if (std::string(kv.first) == "segments") segmode = kv.second != 0;
            if (std::string(kv.first) == "stages") stages_env = kv.second;
            if (std::string(kv.first) == "gd_stage_launches") per_stage = kv.second != 0;
        }
        const int pieces = stages_env > 0 ? stages_env : (segmode ? 4 : 12);
        for (long T = 1; T <= 4096; ++T) {
            for (const int sl : {-1, per_stage ? 1 : 0}) {   // as crf_debug_stage_plan asks, and as plan_schedule does
                const StagePlan sp = plan_grad_stages(T, segmode, stages_env, pieces, sl);
                if (sp.nstage < 1 || sp.nstage > kMaxStages - 1) fail("nstage out of range", c, T, 0);
                if (sp.bound[0] != 0 || sp.bound[sp.nstage] != T) fail("bounds do not run from 0 to T", c, T, 0);
                for (int k = 1; k <= sp.nstage; ++k)
                    if (sp.bound[k - 1] >= sp.bound[k]) fail("bounds not strictly increasing", c, T, 0);
                for (const long B : {1L, 80L, 96L}) {
                    for (int stage = 1; stage <= 2 && stage <= sp.nstage; ++stage) {
                        const GradGrid g = plan_grad_grid(sp, stage, B);
                        for (int k = stage; k <= sp.nstage; ++k)
                            if (g.poff[k] > g.poff[k + 1] || g.fpb[k] < 1) fail("poff decreasing", c, T, B);
                        if (g.workgroups != g.poff[sp.nstage + 1]) fail("workgroups", c, T, B);
                        ++plans;
                    }
                }
            }
            for (const long B : {1L, 80L, 96L}) {   // the export writes 4 + 4 * (kMaxStages + 2) ints: a heap block of exactly that size
                std::vector<int32_t> out(4 + 4 * (kMaxStages + 2));
                if (crf_debug_stage_plan(T, B, out.data(), (int)out.size()) != CRF_OK) fail("crf_debug_stage_plan", c, T, B);
            }
        }
        for (const auto &kv : c) crf_debug_unset(kv.first);
    }
    printf("stage_plan_sweep: %zu switch settings x T = 1 .. 4096 x B in {1, 80, 96}: %ld plans, every check held\n", cases.size(), plans);
    return 0;
}
