// cat_amd/csrc/k_ngram.hip -- n-gram LM scores of complete hypothesis rows (include/ctc_crf_hip.h crf_ngram_score; host side:
// crf_host_ctc.hip): per hypothesis the sum of log P(t_i | t_0 .. t_{i-1}) over the compiled tables of cat_amd/ngram_lm.py, with the
// end-of-sentence value where asked, and per position the value and the length of the n-gram that matched.
//
// The walk of the search carries a prefix' LM state through the frames.  For a complete row the state in front of token i is the longest
// suffix of (<s>,) t_0 .. t_{i-1} of at most order - 1 tokens that is a state of the tables -- a function of the last order - 1 tokens
// alone (every look-up leads to the longest suffix of what has been read that is a state, and no state is longer than order - 1 tokens).
// So every (hypothesis, position) pair is resolved on its own: for i >= order - 1 from the root over t_{i-order+1} .. t_{i-1}, for
// i < order - 1 from `start` (or the root) over t_0 .. t_{i-1}, then the one look-up that counts.  No sentence-long chain of loads.
//
// crf_ngram_score_kernel<TOK>: one wave per hypothesis, kNgramScoreWaves of them per workgroup, the grid over H in x alone.  Lane l takes
// positions l, l + 64, ...: a chunk's 64 tokens come in one coalesced load; the context tokens are re-read from the row (the cache has
// them), each one look-up ahead of its use.  The look-up is ngram_lookup of k_ngram_common.h, the fused search's: chains of dependent
// loads that the 64 lanes and the waves of a SIMD overlap; the tables' pointers stay in scalar registers (no spill: DESIGN.md 7 (f13)).
// Per chunk the values are summed in fp64 by a butterfly over the wave (idle lanes add 0; a + b = b + a, so every lane holds the same
// bits), the chunks in ascending order: the order of the sum depends on the length alone.  Lane 0 adds eos[state behind the last token]
// -- that state is the `next` of position L - 1's look-up, in the lane that owns it -- and stores.
// The matched length is 1 + the history length of the state in whose row the token was found.  The tables carry no length per state;
// the states are sorted by history length and, inside one length, in the order of the arcs that lead to them (ngram_lm.py: states by
// (length, tokens), rows by label), so length d + 1 begins at arc_next[row_off[first state of length d]]: order - 2 pairs of scalar loads
// per wave give the first state of every length, a state's length is the number of those it has reached.
// An invalid row (length outside [0, stride], a token outside [0, V) among the first L, found by a vote of the wave per chunk): -inf,
// the flag, zeros over its per-token rows; a length out of range reads nothing of the row.
// Every state and arc index is clamped and every loop bounded: no access outside the tables whatever they hold.  No LDS, no barrier,
// vector stores only.
#include "k_ngram_common.h"

namespace crf {

template <bool TOK>
__global__ __launch_bounds__(64 * kNgramScoreWaves) void crf_ngram_score_kernel(NgramScoreParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t h = (int64_t)blockIdx.x * kNgramScoreWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (h >= p.H) return;                       // (no barrier in this kernel: waves leave on their own)
    const NgramDev &lm = p.lm;
    const int W = p.stride, V = lm.V;
    const int S1 = max(lm.S, 1) - 1, A = max(lm.A, 0);
    const int Lr = __builtin_amdgcn_readfirstlane(p.hyp_len[h]);
    bool ok = Lr >= 0 && Lr <= W;
    const int L = ok ? Lr : 0;
    const int *row = p.hyps + h * W;
    float *tlp = TOK && p.tok_logp ? p.tok_logp + h * W : nullptr;
    int *tor = TOK && p.tok_order ? p.tok_order + h * W : nullptr;
    const int ctx = min(max(lm.order, 1), kNgramMaxOrder) - 1;       // context tokens of a look-up
    const int s0 = p.use_start ? min(max(lm.start, 0), S1) : 0;

    // the first state of every history length 2 .. 7 (INT_MAX: the tables hold none that long); length 1 begins at state 1
    int lv[kNgramMaxOrder];
#pragma unroll
    for (int d = 0; d < kNgramMaxOrder; ++d) lv[d] = 0x7fffffff;
    if (TOK) {
        int first = 1;
        bool more = true;
#pragma unroll
        for (int d = 2; d < kNgramMaxOrder; ++d) {
            more = more && d <= ctx && first <= S1;
            if (more) {
                const int a = __builtin_amdgcn_readfirstlane(min(max(lm.row_off[first], 0), A));
                more = a < A;
                if (more) { first = __builtin_amdgcn_readfirstlane(lm.arc_next[a]); lv[d] = first; more = first > 0; }
            }
        }
    }

    double total = 0.0;
    int last = s0;                              // the state behind the last token
    for (int i0 = 0; i0 < L; i0 += 64) {
        const int i = i0 + lane;
        const bool act = i < L;
        const int t = act ? row[i] : 0;
        if (__ballot(act && (unsigned)t >= (unsigned)V)) { ok = false; break; }     // (uniform)
        float lp = 0.f;
        int nx = 0, mo = 0;
        if (act) {
            const int k = min(i, ctx);
            int s = i < ctx ? s0 : 0;
            int c = row[i - k];                 // (k = 0: t itself)
            for (int j = 0; j < k; ++j) {
                const int cn = row[i - k + j + 1];                  // the next token, a look-up ahead (the last one is t)
                float x;
                int n;
                ngram_lookup<false>(lm, s, c, x, n);
                s = n;
                c = cn;
            }
            int at = 0;
            ngram_lookup<TOK>(lm, s, c, lp, nx, &at);
            if (TOK) {
                mo = at > 0 ? 2 : 1;
#pragma unroll
                for (int d = 2; d < kNgramMaxOrder; ++d) mo += at >= lv[d];
            }
        }
        if (TOK && i < W) {
            if (tlp) tlp[i] = lp;
            if (tor) tor[i] = mo;
        }
        double v = act ? (double)lp : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        total += v;
        if (i0 + 64 >= L) last = __shfl(nx, (L - 1) & 63);
    }

    if (!ok) {
        if (lane == 0) {
            p.score[h] = -INFINITY;
            if (p.invalid) p.invalid[h] = 1;
        }
        if (TOK)
            for (int i = lane; i < W; i += 64) {
                if (tlp) tlp[i] = 0.f;
                if (tor) tor[i] = 0;
            }
        return;
    }
    if (TOK)
        for (int i = ((L + 63) & ~63) + lane; i < W; i += 64) {
            if (tlp) tlp[i] = 0.f;
            if (tor) tor[i] = 0;
        }
    if (lane == 0) {
        if (p.add_eos) total += (double)p.eos[min(max(last, 0), S1)];
        p.score[h] = (float)total;
        if (p.invalid) p.invalid[h] = 0;
    }
}

template __global__ void crf_ngram_score_kernel<false>(NgramScoreParams);
template __global__ void crf_ngram_score_kernel<true>(NgramScoreParams);

}  // namespace crf
