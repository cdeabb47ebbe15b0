// cat_amd/csrc/k_ngram_common.h -- the look-up in the compiled n-gram tables (include/ctc_crf_hip.h crf_ngram_tables, "Lookup") that the
// fused beam search (k_beam_lm.hip) and the scoring of complete rows (k_ngram.hip) share.  One copy for both translation units (and for
// crf_unity.hip).
#pragma once
#include "crf_device.h"
#include "crf_kernels_decl.h"

namespace crf {

// (state s, class c) -> lp = log P(c | s) along the back-off chain (fp32: the back-off weights in order, then the arc's value -- sums
// only, nothing a compiler could contract), the next state and, with AT, *at = the state in whose row c was found (0: the root's dense
// row).  The fused search calls ngram_lookup<false> itself: through a wrapper its kernel compiles to other code (profiles/).
// At most min(order, kNgramMaxOrder) sparse rows, then the root's dense row -- with tables that pass crf_ngram_tables_check a state lies
// at most order - 1 back-offs above the root, so the walk ends by itself.  Every state and arc index is clamped into the tables and both
// loops are bounded: no access out of bounds and no hang whatever the tables hold.
template <bool AT>
__device__ __forceinline__ void ngram_lookup(const NgramDev &lm, int s, int c, float &lp, int &nx, int *at = nullptr) {
    const int S1 = max(lm.S, 1) - 1, A = max(lm.A, 0);
    c = min(max(c, 0), lm.V - 1);
    s = min(max(s, 0), S1);
    float acc = 0.f;
    const int steps = min(lm.order, kNgramMaxOrder);
    for (int i = 0; i < steps && s > 0; ++i) {
        int lo = min(max(lm.row_off[s], 0), A);
        const int end = min(max(lm.row_off[s + 1], 0), A);
        int hi = end;
        for (int it = 0; it < kNgramRowSteps && lo < hi; ++it) {       // (lo <= mid < hi <= A: inside arc_label)
            const int mid = (lo + hi) >> 1;
            if (lm.arc_label[mid] < c) lo = mid + 1; else hi = mid;
        }
        if (lo < end && lm.arc_label[lo] == c) {
            lp = acc + lm.arc_logp[lo];
            nx = lm.arc_next[lo];
            if (AT) *at = s;
            return;
        }
        acc += lm.bo_weight[s];
        s = min(max(lm.bo_state[s], 0), S1);
    }
    lp = acc + lm.uni_logp[c];
    nx = lm.uni_next[c];
    if (AT) *at = 0;
}

}  // namespace crf
