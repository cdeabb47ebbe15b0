// cat_amd/csrc/k_beam_lm_body.h -- THE frame step of the prefix beam search with the n-gram LM, as two device functions: called per frame
// by crf_beamlm_search_kernel (k_beam_lm.hip, the whole utterance) and by crf_beamlm_chunk_kernel (k_beam_chunk.hip, a chunk of frames
// with the beam carried across calls).  The caller owns the LDS (lm_w, lm_n: [64][kBeamLmStride]; st_lds: the slots' LM states; na_lds:
// live slots), the barriers between the parts and the fetch of the next frame's words.
//
// The beam lives in the registers of wave 0 as in k_beam_body.h (slot k in lane k: a BeamSlot) plus the prefix' LM state and lm = alpha
// * log P_lm(prefix) + beta * len in fp64.  The LM-free selection does not carry over: there the extensions of one parent are sorted by
// x[c], here alpha * log P(c | history) + beta is added per (slot, class) and the order differs from slot to slot.  Per frame:
//   A. beamlm_frame_lookups: ALL waves resolve the W_alive x C lookups (slot's LM state, class of place j in E_t) into two LDS matrices
//      [slot][place], rows kBeamLmStride = 65 words apart (lane k walking its row and lane j reading entry j of one row are both free of
//      bank conflicts): lm_w = lmw = alpha * lp + beta (fp32, product and sum rounded separately) and lm_n = the next LM state.  One pair
//      per thread and step: a lookup is a chain of dependent loads (row bounds, at most kNgramRowSteps probes of the sorted row, the
//      back-off weight and state, at most `order` times, ending in the root's dense row), so the pairs are spread over the lanes and the
//      chains overlap.  Every state and arc index is clamped into the tables, both loops are bounded: no fault and no hang whatever the
//      tables hold.  The slots' LM states come through LDS (st_lds, na_lds = the number of live slots: they are slots 0 .. na - 1).
//      Barrier.
//   B. beamlm_frame_step: wave 0 runs steps 1 and 2 of k_beam_body.h (beam_frame_merges: a merge moves acoustic mass only) and steps 3
//      and 4 with a head per slot: every lane finds the arg-max of x[c] + lmw over the unstruck places of its row (fp64 sum of the two
//      fp32 values; ties to the lower place), the W rounds take the wave maximum of the FUSED scores (acoustic + lm, stay before
//      extension, then the lowest slot), and a slot that wins with its head gets its next head from the whole wave: lane j reads entry j
//      of the winner's row, one wave maximum, the lowest lane that holds it.  Slot r notes the winner's lane, kind, class and place;
//      behind the rounds it gathers the parent's fields, the place's x, lmw and next state, and forms pnb' and lm' from them -- the same
//      operands in the same operations as in the winner's lane.  Barrier.
// With alpha == 0 and beta == 0 every lmw is +0 and every lm is 0: the keys are the x[c], the fused scores are the acoustic ones, and
// every output equals the LM-free search's bit for bit.
#pragma once
#include "k_beam_body.h"
#include "k_ngram_common.h"   // ngram_lookup: the look-up in the tables, shared with k_ngram.hip

namespace crf {

// A. pair i = (slot i / C, place i % C), one per thread and step; ct: the C classes of the frame's E_t; NT threads
template <int NT>
__device__ __forceinline__ void beamlm_frame_lookups(const NgramDev &lmt, const float alpha, const float beta, const int *ct, const int na,
                                                     const int W, const int C, const int tid, const int *st_lds, float *lm_w, int *lm_n) {
    const int np = min(na, W) * C;
    for (int i = tid; i < np; i += NT) {
        const int k = i / C, j = i - k * C;
        const int c = ct[j];
        float w = 0.f;
        int nx = 0;
        if (c >= 0) {                   // (a filler pair (-1, -inf) is no candidate: nothing to look up)
            float lp;
            ngram_lookup<false>(lmt, st_lds[k], c, lp, nx);
            w = __fadd_rn(__fmul_rn(alpha, lp), beta);
        }
        lm_w[k * kBeamLmStride + j] = w;
        lm_n[k * kBeamLmStride + j] = nx;
    }
}

// B. wave 0.  lm, lms: the slot's alpha log P_lm + beta len and its LM state; S1: the highest state; the new states and the number of
// live slots go to st_lds / na_lds
__device__ __forceinline__ void beamlm_frame_step(BeamSlot &b, double &lm, int &lms, const float vj, const int cj, const float xb,
                                                  const int lane, const int W, const int C, const int S1, int *tr_row, const float *lm_w,
                                                  const int *lm_n, int *st_lds, int *na_lds) {
    const double kNegInf = -__builtin_huge_val();
    const float *my_w = lm_w + lane * kBeamLmStride;
    const BeamFrame f = beam_frame_merges(b, vj, cj, xb, lane, W, C);
    const int pos = f.pos;
    const double s_stay = b.alive ? beam_lse2(f.spb, f.spnb) + lm : kNegInf;
    const float ew = my_w[max(pos, 0)];                     // the repeat's lmw
    const double ek = (double)f.ve + (double)ew;
    const double s_rep = f.rep_ok ? ((double)f.ve + b.pb) + (lm + (double)ew) : kNegInf;
    bool stay_ok = b.alive != 0, rep_ok = f.rep_ok;
    beam_u64 mask = f.mask;                                 // struck places of the slot's row
    // 3. the head of every slot's row: the arg-max of x[c] + lmw over its unstruck places, ties to the lower place
    double hk = kNegInf;
    int h = 64;
    for (int j = 0; j < C; ++j) {
        const double key = (double)beam_bcast(vj, j) + (double)my_w[j];
        if (!((mask >> j) & 1) && key > hk) { hk = key; h = j; }   // (-inf and NaN never win)
    }
    int hc = __shfl(cj, h & 63);
    float hv = __shfl(vj, h & 63), hw = my_w[h & 63];
    // W rounds of the best candidate; slot r keeps where it came from, the fields follow in one gather behind the rounds
    int src = -1, n_kind = 0, n_c = -1, n_pl = 0;
    for (int r = 0; r < W; ++r) {
        const double s_list = (b.alive && h < 64) ? ((double)hv + f.tot) + (lm + (double)hw) : kNegInf;
        const double rr = rep_ok ? s_rep : kNegInf;
        const bool rep_first = rr > s_list || (rr == s_list && (ek > hk || (ek == hk && pos < h)));
        const double sx = rep_first ? rr : s_list;
        double s = stay_ok ? s_stay : kNegInf;
        int kind = 0;                                       // 0 stay, 1 extension by e, 2 head of the row
        if (sx > s) { s = sx; kind = rep_first ? 1 : 2; }
        const double mx = beam_wave_max(s);
        if (!(mx > kNegInf)) break;                         // (uniform; NaN ends the frame too)
        const bool top = s == mx;
        const beam_u64 bs = __ballot(top && kind == 0);
        const beam_u64 bal = bs ? bs : __ballot(top);
        if (!bal) break;
        const int m = __ffsll((long long)bal) - 1;
        const int c = kind == 0 ? -1 : kind == 1 ? b.e : hc;
        const int pl = kind == 1 ? pos : h;
        const int b_kind = beam_bcast(kind, m), b_c = beam_bcast(c, m), b_pl = beam_bcast(pl, m) & 63;
        if (lane == r) { src = m; n_kind = b_kind; n_c = b_c; n_pl = b_pl; }
        if (b_kind == 2) {
            // the winner's next head, by the whole wave: lane j looks at place j of its row
            const beam_u64 nmask = beam_bcast(mask, m) | (1ull << b_pl);
            const float w2 = lm_w[m * kBeamLmStride + lane];
            double key = (double)vj + (double)w2;
            if (((nmask >> lane) & 1) || !(key > kNegInf)) key = kNegInf;
            const double kmax = beam_wave_max(key);
            const beam_u64 kb = __ballot(key == kmax);
            const int nh = (kmax > kNegInf && kb) ? __ffsll((long long)kb) - 1 : 64;
            const int c2 = beam_bcast(cj, nh & 63);
            const float v2 = beam_bcast(vj, nh & 63), hw2 = beam_bcast(w2, nh & 63);
            if (lane == m) { mask = nmask; h = nh; hk = kmax; hc = c2; hv = v2; hw = hw2; }
        } else if (lane == m) {
            if (kind == 0) stay_ok = false; else rep_ok = false;
        }
    }
    // 4. the trace row, the new beam: slot r's fields from its parent's lane, the place's x, lmw and next state
    if (lane < W) tr_row[lane] = src >= 0 ? src + 64 * (n_c + 1) : -1;
    {
        const int sl = src >= 0 ? src : lane;
        const double g_spb = __shfl(f.spb, sl), g_spnb = __shfl(f.spnb, sl), g_pb = __shfl(b.pb, sl), g_tot = __shfl(f.tot, sl), g_lm = __shfl(lm, sl);
        const beam_u64 g_id = __shfl(b.id, sl), g_pid = __shfl(b.pid, sl);
        const int g_e = __shfl(b.e, sl), g_len = __shfl(b.len, sl), g_lms = __shfl(lms, sl);
        const float g_x = __shfl(vj, n_pl), g_w = lm_w[sl * kBeamLmStride + n_pl];
        const int g_n = lm_n[sl * kBeamLmStride + n_pl];
        const bool st = n_kind == 0;
        const int alive = src >= 0;
        b.alive = alive;
        b.pb = alive && st ? g_spb : kNegInf;
        b.pnb = !alive ? kNegInf : st ? g_spnb : (double)g_x + (n_kind == 1 ? g_pb : g_tot);   // (an extension's pnb' is its acoustic score)
        lm = !alive ? 0.0 : st ? g_lm : g_lm + (double)g_w;
        lms = !alive ? 0 : st ? g_lms : min(max(g_n, 0), S1);
        b.id = !alive ? 0ull : st ? g_id : beam_mix(g_id, n_c);
        b.pid = !alive ? 0ull : st ? g_pid : g_id;
        b.e = !alive ? -2 : st ? g_e : n_c;
        b.len = !alive ? 0 : g_len + (st ? 0 : 1);
    }
    st_lds[lane] = lms;
    const beam_u64 live = __ballot(b.alive != 0);
    if (lane == 0) *na_lds = __popcll(live);
}

}  // namespace crf
