// cat_amd/csrc/stage_plan.cpp -- the plan of the staged grad pass (stage_plan.h): plain host C++, so that the CPU suite
// (crf_debug_stage_plan, tests/test_stage_plan.py) and a host sanitizer (tools/stage_plan_sweep.cpp) reach it without a GPU.
#include "stage_plan.h"

#include <algorithm>
#include <cstdlib>

#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"

namespace crf {

constexpr int kGDFrames = kStageFrames;

// Stage bounds of the staged grad pass (crf_loss_fwd_bwd; crf_debug_stage_plan shows them to the tests).
StagePlan plan_grad_stages(int64_t T, bool segmode, int stages_env, int pieces, int stage_launches) {
    // stage_launches: one grad launch per stage (round 4's schedule) -- the switch gd_stage_launches, or a context whose one-launch grad pass has
    // timed out once (DevCtx::gd_fallback)
    const bool per_stage = stage_launches >= 0 ? stage_launches != 0 : opt_on(kOpt_gd_stage_launches);
    StagePlan sp;
    auto &bound = sp.bound;
    int nstage = 1, gd_piece = 0;
    bound[0] = 0;
    bound[1] = (int)T;
    if (T >= 256) {
        const int half = (int)((T / 2 + kGDFrames - 1) / kGDFrames * kGDFrames);
        int piece, first = half;
        if (stages_env > 0 || segmode) {
            const int nshort = std::max(1, std::min(std::min(pieces, kMaxStages - 2), (int)(T - half) / 32));
            piece = ((int)T - half + nshort - 1) / nshort;
            piece = (piece + kGDFrames - 1) / kGDFrames * kGDFrames;
        } else {
            // (round 5, one grad launch for all stages: a stage costs the grad pass nothing any more and the recursions one drain + barrier;
            // pieces of 48 .. 96 iterations all give 2.71 ms where 128 gives 2.75 and round 4's per-stage launches 2.82: profiles/round5_ab_grad_one_launch.txt)
            piece = per_stage ? 128 : 80;
            while ((kMaxStages - 4) * piece < (int)T - half && piece < (int)T) piece += per_stage ? 128 : 16;   // the stage counters cover T - half
            const int piece_env = opt(kOpt_piece, 0);
            if (piece_env > 0) piece = (piece_env + kGDFrames - 1) / kGDFrames * kGDFrames;
            const int body = std::min((int)T - half, (kMaxStages - 2) * piece);   // (a CRF_PIECE too small for the counters)
            first = std::max(half, ((int)T - body + kGDFrames - 1) / kGDFrames * kGDFrames);
            const int fs = opt(kOpt_first_shift, 0);
            if (fs > 0) first = std::min((int)T - kGDFrames, first + fs * kGDFrames);
        }
        nstage = 1;
        gd_piece = piece;
        bound[1] = first;
        while (bound[nstage] < T && nstage < kMaxStages - 1) { bound[nstage + 1] = std::min((int)T, bound[nstage] + piece); ++nstage; }
        bound[nstage] = (int)T;
        // taper: the last stage is what is left to do when the recursions have ended; with one grad launch for all stages (its workgroups
        // wait themselves) a stage costs the grad pass nothing and the recursions one drain + barrier, so the last pieces are halved down
        // to `taper` iterations: ..., piece, piece / 2, piece / 4, ..., taper
        const int taper = stages_env > 0 || segmode || per_stage ? 0 : (opt(kOpt_taper, 32) + kGDFrames - 1) / kGDFrames * kGDFrames;
        if (taper > 0 && taper < piece && nstage >= 3) {
            std::array<int, kMaxStages + 8> desc{};                    // stage ends from the last one backwards
            int n = 0, pos = (int)T;
            desc[n++] = pos;
            for (int q = taper; q < piece && n < 8; q *= 2) { pos -= q; desc[n++] = pos; }
            while (pos - piece > first + kGDFrames && n < kMaxStages + 6) { pos -= piece; desc[n++] = pos; }
            if (pos > first && n + 1 <= kMaxStages - 1) {               // (the piece behind `first` takes what is left: 16 .. piece + 16 iterations)
                nstage = n + 1;
                bound[1] = first;
                for (int k = 0; k < n; ++k) bound[2 + k] = desc[n - 1 - k];
            }
        }
    }
    if (nstage > kMaxStages - 1) abort();   // (the stage counters, and every array of the plan)
    sp.nstage = nstage;
    sp.piece = gd_piece;
    return sp;
}

// The one-launch grad pass's grid (crf_grad_den_kernel, gd_persist): first block of the candidates of the stages `stage` .. nstage, frames per
// workgroup in each
GradGrid plan_grad_grid(const StagePlan &sp, int stage, int64_t B) {
    GradGrid g;
    int64_t tot = 0;
    const int sub_env = opt(kOpt_gd_sub, 16);              // frames per workgroup in a last stage shorter than `piece` (16: whole blocks)
    const int fsub = sub_env == 8 ? 8 : sub_env == 4 ? 4 : sub_env == 2 ? 2 : kGDFrames;
    for (int k = stage; k <= sp.nstage; ++k) {
        g.poff[k] = (int)tot;
        g.fpb[k] = (k == sp.nstage && sp.bound[k] - sp.bound[k - 1] < sp.piece) ? fsub : kGDFrames;   // (the LAST stage only)
        tot += 2 * (int64_t)((sp.bound[k] - sp.bound[k - 1] + kGDFrames - 1) / kGDFrames + 3) * (kGDFrames / g.fpb[k]) * B;
    }
    g.poff[sp.nstage + 1] = (int)tot;
    g.workgroups = tot;
    return g;
}

}  // namespace crf

using namespace crf;

extern "C" int crf_debug_stage_plan(int64_t T, int64_t B, int32_t *out, int n_out) {
    constexpr int n = kMaxStages + 2;
    if (!out || n_out < 4 + 4 * n || T < 1 || B < 1) { set_error("crf_debug_stage_plan: out needs 4 + 4 * 18 ints"); return CRF_ERR_ARG; }
    const bool segmode = opt_on(kOpt_segments);
    const int stages_env = opt(kOpt_stages, 0);
    const StagePlan sp = plan_grad_stages(T, segmode, stages_env, stages_env > 0 ? stages_env : (segmode ? 4 : 12));
    const bool one = !segmode && sp.nstage >= 3 && !opt_on(kOpt_gd_stage_launches);
    const GradGrid g = one ? plan_grad_grid(sp, 2, B) : GradGrid{};
    out[0] = sp.nstage; out[1] = sp.piece; out[2] = one ? 1 : 0; out[3] = (int32_t)g.workgroups;
    for (int k = 0; k < n; ++k) {
        out[4 + k] = k < (int)sp.bound.size() ? sp.bound[k] : 0;
        out[4 + n + k] = k < (int)g.poff.size() ? g.poff[k] : 0;
        out[4 + 2 * n + k] = k < (int)g.fpb.size() ? g.fpb[k] : 0;
        out[4 + 3 * n + k] = k >= 1 && k <= sp.nstage ? (sp.bound[k] - sp.bound[k - 1] + kGDFrames - 1) / kGDFrames + 3 : 0;   // candidates per run (nfc)
    }
    return CRF_OK;
}
