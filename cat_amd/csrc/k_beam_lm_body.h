// cat_amd/csrc/k_beam_lm_body.h -- one frame of the prefix beam search with the n-gram LM as two device functions: part A (all waves: the
// frame's LM lookups into the two LDS matrices) and part B (wave 0: steps 1 to 4 with a head per slot) of k_beam_lm.hip's
// crf_beamlm_search_kernel, operation for operation, for the kernels that carry a beam across calls (k_beam_chunk.hip).  A COPY, as
// k_beam_body.h is and for the same reason: called from crf_beamlm_search_kernel these functions changed that kernel's register
// allocation from its first block on (profiles/beam_chunk_resource_usage.txt).  tests/test_gpu_ctc_beam_stream_lm.py holds the copy to
// the original bit for bit.  The caller owns the LDS (lm_w, lm_n: [64][kBeamLmStride]; st_lds: the slots' LM states; na_lds: live
// slots) and the barriers between the parts.
#pragma once
#include "k_beam_body.h"
#include "k_ngram_common.h"

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
__device__ __forceinline__ void beamlm_frame_step(BeamSlot &b, double &lm_io, int &lms_io, const float vj, const int cj, const float xb,
                                                  const int lane, const int W, const int C, const int S1, int *tr_row, const float *lm_w,
                                                  const int *lm_n, int *st_lds, int *na_lds) {
    const double kNegInf = -__builtin_huge_val();
    const float *my_w = lm_w + lane * kBeamLmStride;
    int alive = b.alive;
    double pb = b.pb, pnb = b.pnb, lm = lm_io;
    beam_u64 id = b.id, pid = b.pid;
    int e = b.e, len = b.len, lms = lms_io;
    // 1. the last label among the frame's classes
    int pos = -1;
    float ve = -INFINITY;
    for (int j = 0; j < C; ++j) {
        const int c = beam_bcast(cj, j);
        const float v = beam_bcast(vj, j);
        if (c == e) { pos = j; ve = v; }
    }
    const double tot = beam_lse2(pb, pnb);
    const double spb = alive ? (double)xb + tot : kNegInf;
    double spnb = (alive && pos >= 0) ? (double)ve + pnb : kNegInf;
    beam_u64 mask = C >= 64 ? 0ull : ~0ull << C;           // struck places of the slot's row
    if (pos >= 0) mask |= 1ull << pos;
    bool rep_ok = alive && pos >= 0;                        // the extension by e itself: base pb
    // 2. merges into the slots whose parent is in the beam (acoustic mass only)
    double madd = kNegInf;
    for (int k = 0; k < W; ++k) {
        const int kpos = beam_bcast(pos, k);
        if (!beam_bcast(alive, k) || beam_bcast(len, k) == 0 || kpos < 0) continue;    // (uniform)
        const beam_u64 kp = beam_bcast(pid, k);
        const int ke = beam_bcast(e, k);
        const float kv = beam_bcast(ve, k);
        const bool match = alive && id == kp;
        const beam_u64 bal = __ballot(match);
        if (!bal) continue;
        double contrib = kNegInf;
        if (match) {
            if (ke == e) { contrib = (double)kv + pb; rep_ok = false; }
            else { contrib = (double)kv + tot; mask |= 1ull << kpos; }
        }
        const double cb = beam_bcast(contrib, __ffsll((long long)bal) - 1);
        if (lane == k) madd = cb;
    }
    spnb = beam_lse2(spnb, madd);
    const double s_stay = alive ? beam_lse2(spb, spnb) + lm : kNegInf;
    const float ew = my_w[max(pos, 0)];                     // the repeat's lmw
    const double ek = (double)ve + (double)ew;
    const double s_rep = rep_ok ? ((double)ve + pb) + (lm + (double)ew) : kNegInf;
    bool stay_ok = alive != 0;
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
        const double s_list = (alive && h < 64) ? ((double)hv + tot) + (lm + (double)hw) : kNegInf;
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
        const int c = kind == 0 ? -1 : kind == 1 ? e : hc;
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
        const double g_spb = __shfl(spb, sl), g_spnb = __shfl(spnb, sl), g_pb = __shfl(pb, sl), g_tot = __shfl(tot, sl), g_lm = __shfl(lm, sl);
        const beam_u64 g_id = __shfl(id, sl), g_pid = __shfl(pid, sl);
        const int g_e = __shfl(e, sl), g_len = __shfl(len, sl), g_lms = __shfl(lms, sl);
        const float g_x = __shfl(vj, n_pl), g_w = lm_w[sl * kBeamLmStride + n_pl];
        const int g_n = lm_n[sl * kBeamLmStride + n_pl];
        const bool st = n_kind == 0;
        alive = src >= 0;
        pb = alive && st ? g_spb : kNegInf;
        pnb = !alive ? kNegInf : st ? g_spnb : (double)g_x + (n_kind == 1 ? g_pb : g_tot);   // (an extension's pnb' is its acoustic score)
        lm = !alive ? 0.0 : st ? g_lm : g_lm + (double)g_w;
        lms = !alive ? 0 : st ? g_lms : min(max(g_n, 0), S1);
        id = !alive ? 0ull : st ? g_id : beam_mix(g_id, n_c);
        pid = !alive ? 0ull : st ? g_pid : g_id;
        e = !alive ? -2 : st ? g_e : n_c;
        len = !alive ? 0 : g_len + (st ? 0 : 1);
    }
    st_lds[lane] = lms;
    const beam_u64 live = __ballot(alive != 0);
    if (lane == 0) *na_lds = __popcll(live);
    b.alive = alive; b.pb = pb; b.pnb = pnb; b.id = id; b.pid = pid; b.e = e; b.len = len;
    lm_io = lm; lms_io = lms;
}

}  // namespace crf
