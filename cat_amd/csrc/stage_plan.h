// cat_amd/csrc/stage_plan.h -- the plan of the staged grad pass (stage_plan.cpp: host C++ only, no kernels): the stage bounds the factored
// recursions publish, and the grid of the one-launch grad pass that follows them.  Every array has its capacity in its type; the capacities
// are those of the kernels' parameter blocks (LossParams::gd_bound / gd_poff / gd_fpb, FacParams::bound: crf_host.hip asserts it).
#pragma once
#include <stdint.h>

#include <array>

namespace crf {

constexpr int kMaxStages = 16;   // stage counters of a context; a plan has at most kMaxStages - 1 stages
constexpr int kStageFill = 75;   // staged schedule (and the numerator chains beside the recursions) for den grids of up to this percent of the CUs
#ifndef CRF_GD_FRAMES
#define CRF_GD_FRAMES 16
#endif
constexpr int kStageFrames = CRF_GD_FRAMES;   // frames per block of the grad pass (kGDFrames of crf_kernels_decl.h)

// bound[0] = 0 < bound[1] < ... < bound[nstage] = T: stage k = the recursions' iterations [bound[k-1], bound[k]); piece = the length of the equal pieces
struct StagePlan {
    int nstage = 1, piece = 0;
    std::array<int, kMaxStages> bound{};
};
// the one-launch grad pass's grid: the candidates of stage k start at workgroup poff[k] (poff[nstage + 1] = workgroups), fpb[k] frames per workgroup
struct GradGrid {
    int64_t workgroups = 0;
    std::array<int, kMaxStages + 1> poff{};
    std::array<int, kMaxStages> fpb{};
};
// stage_launches: 1 = one grad launch per stage, 0 = one launch for all, -1 = as the switch gd_stage_launches says
StagePlan plan_grad_stages(int64_t T, bool segmode, int stages_env, int pieces, int stage_launches = -1);
GradGrid plan_grad_grid(const StagePlan &sp, int stage, int64_t B);

}  // namespace crf
