// cat_amd/csrc/k_beam_lm.hip -- CTC prefix beam search with shallow fusion of a token-level n-gram LM (include/ctc_crf_hip.h
// crf_ctc_beam_lm; host side: crf_host_ctc.hip).  The row stage is k_beam.hip's crf_beam_row_kernel<E>, unchanged, with its workspace
// records (val / cls, [B T][C + 1]); this file holds the fused search, which cannot take crf_beam_search_kernel's selection: there the
// extensions of one parent are sorted by x[c], here alpha * log P(c | history) + beta is added per (slot, class) and the order differs
// from slot to slot.
//
// crf_beamlm_search_kernel: ONE workgroup of kBeamLmWaves waves per utterance.  The beam lives in the registers of wave 0 as in
// crf_beam_search_kernel (slot k in lane k: pb, pnb in fp64, the prefix' id, its parent's id, last label, length) plus the prefix' LM
// state and lm = alpha * log P_lm(prefix) + beta * len in fp64.  Per frame:
//   A. ALL waves resolve the W_alive x C lookups (slot's LM state, class of place j in E_t) into two LDS matrices [slot][place], rows
//      kBeamLmStride = 65 words apart (lane k walking its row and lane j reading entry j of one row are both free of bank conflicts):
//      lm_w = lmw = alpha * lp + beta (fp32, product and sum rounded separately) and lm_n = the next LM state.  One pair per thread and
//      step: a lookup is a chain of dependent loads (row bounds, at most kNgramRowSteps probes of the sorted row, the back-off weight
//      and state, at most `order` times, ending in the root's dense row), so the pairs are spread over the lanes and the chains overlap.
//      Every state and arc index is clamped into the tables, both loops are bounded: no fault and no hang whatever the tables hold.
//      The slots' LM states come through LDS (st_lds, na_lds = the number of live slots: they are slots 0 .. na - 1).  Barrier.
//   B. wave 0 runs steps 1, 2 and 4 of crf_beam_search_kernel unchanged (a merge moves acoustic mass only: prefixes are label
//      sequences, so both sides of a merge carry the same lm) and step 3 with a head per slot: every lane finds the arg-max of
//      x[c] + lmw over the unstruck places of its row (fp64 sum of the two fp32 values; ties to the lower place), the W rounds take the
//      wave maximum of the FUSED scores (acoustic + lm, stay before extension, then the lowest slot), and a slot that wins with its head
//      gets its next head from the whole wave: lane j reads entry j of the winner's row, one wave maximum, the lowest lane that holds it.
//      Slot r notes the winner's lane, kind, class and place; behind the rounds it gathers the parent's fields, the place's x, lmw and
//      next state, and forms pnb' and lm' from them -- the same operands in the same operations as in the winner's lane.  Barrier.
// Waits per frame: two barriers, the lookups' vector-memory waits in A (what bounds the frame: DESIGN.md 7 (f11)), the prefetched row of
// the next frame in B (issued a frame ahead), LDS waits on the matrix reads.
// Back-trace as in crf_beam_search_kernel; the trace rows come back through lm_n's LDS (all waves copy, wave 0 follows the ranks).
// With alpha == 0 and beta == 0 every lmw is +0 and every lm is 0: the keys are the x[c], the fused scores are the acoustic ones, and
// every output equals crf_ctc_beam's bit for bit.
#include "k_beam_common.h"
#include "k_ngram_common.h"   // ngram_lookup: the look-up in the tables, shared with k_ngram.hip

namespace crf {

__global__ __launch_bounds__(64 * kBeamLmWaves) void crf_beamlm_search_kernel(BeamLmParams q) {
    __shared__ float lm_w[64 * kBeamLmStride];  // [slot][place] lmw of the slot's extension by the class at that place of E_t
    __shared__ int lm_n[64 * kBeamLmStride];    // ... and its next LM state; behind the frames: 64 frames of the trace for the back-trace
    __shared__ int st_lds[kBeamMaxW];           // the slots' LM states
    __shared__ int na_lds;                      // live slots: 0 .. na - 1
    __shared__ NgramDev lm_lds;                 // the tables' pointers and sizes: read per lookup from LDS into vector registers -- held in
                                                // scalar registers across the frame loop they would not fit beside the search's (spills)
    const BeamParams &p = q.b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int T = p.T, W = p.W, C = p.C, RS = C + 1;
    const int lx = max(0, min(p.lx[b], T));
    const int S1 = max(q.lm.S, 1) - 1;
    const double kNegInf = -__builtin_huge_val();
    const float *val = p.val + (int64_t)b * T * RS;
    const int *cls = p.cls + (int64_t)b * T * RS;
    int *tr = p.trace + (int64_t)b * T * W;
    int *tr_lds = lm_n;
    const int jl = C > 0 ? 1 + min(lane, C - 1) : 0;   // this lane's word of a row (lanes >= C: clamped, not used)
    float *my_w = lm_w + lane * kBeamLmStride;          // wave 0: this slot's row

    for (int i = tid; i < 64 * kBeamLmStride; i += 64 * kBeamLmWaves) { lm_w[i] = 0.f; lm_n[i] = 0; }
    if (tid < kBeamMaxW) st_lds[tid] = tid == 0 ? min(max(q.lm.start, 0), S1) : 0;
    if (tid == 0) { na_lds = 1; lm_lds = q.lm; }
    __syncthreads();

    // the beam (wave 0): the empty prefix in slot 0
    int alive = lane == 0;
    double pb = lane == 0 ? 0.0 : kNegInf, pnb = kNegInf, lm = 0.0;
    beam_u64 id = 0x243F6A8885A308D3ull, pid = 0;
    int e = -2, len = 0;                        // (no last label: -2 matches neither a class nor a filler pair)
    int lms = lane == 0 ? min(max(q.lm.start, 0), S1) : 0;

    float nv = 0.f, nxb = 0.f;
    int nc = -1;
    if (wave == 0 && lx > 0) { nv = val[jl]; nc = cls[jl]; nxb = val[0]; }
    for (int t = 0; t < lx; ++t) {
        // A. the frame's lookups, all waves: pair i = (slot i / C, place i % C)
        {
            const int np = min(na_lds, W) * C;
            const int *ct = cls + (int64_t)t * RS + 1;
            const NgramDev lmt = lm_lds;
            const float alpha = q.alpha, beta = q.beta;
            for (int i = tid; i < np; i += 64 * kBeamLmWaves) {
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
        __syncthreads();
        if (wave == 0) {
            const float vj = lane < C ? nv : -INFINITY, xb = nxb;
            const int cj = lane < C ? nc : -1;
            {
                const int64_t o = (int64_t)min(t + 1, lx - 1) * RS;
                nv = val[o + jl]; nc = cls[o + jl]; nxb = val[o];
            }
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
            if (lane < W) tr[(int64_t)t * W + lane] = src >= 0 ? src + 64 * (n_c + 1) : -1;
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
            if (lane == 0) na_lds = __popcll(live);
        }
        __syncthreads();
    }

    // results of the ranks, back-trace
    const bool out = wave == 0 && lane < p.nbest;
    const int olen = alive ? len : 0;
    const int64_t h0 = (int64_t)b * p.nbest;
    if (out) {
        p.score[h0 + lane] = alive ? (float)(beam_lse2(pb, pnb) + lm) : -INFINITY;
        p.hyp_len[h0 + lane] = olen;
        if (q.lm_score) q.lm_score[h0 + lane] = alive ? (float)lm : 0.f;
    }
    int *hyp = p.hyps + (h0 + (out ? lane : 0)) * T;
    int slot = lane, at = olen;
    for (int t1 = lx; t1 > 0; t1 -= 64) {
        const int t0 = max(0, t1 - 64), nw = (t1 - t0) * W;
        __syncthreads();                        // (the trace rows are wave 0's stores; the chunk before has been read)
        for (int i = tid; i < nw; i += 64 * kBeamLmWaves) tr_lds[i] = tr[(int64_t)t0 * W + i];
        __syncthreads();
        if (out && alive) {
            for (int t = t1 - 1; t >= t0; --t) {
                const int wd = tr_lds[(t - t0) * W + slot];
                const int c = (wd >> 6) - 1;
                slot = min(wd & 63, W - 1);     // (a live slot's word is never -1; the clamp keeps any word inside the row)
                if (c >= 0 && at > 0) hyp[--at] = c;
            }
        }
    }
    if (wave == 0) {
        for (int r = 0; r < p.nbest; ++r) {
            const int L = beam_bcast(olen, r);
            int *row = p.hyps + (h0 + r) * T;
            for (int j = L + lane; j < T; j += 64) row[j] = p.blank;
        }
        if (p.fill_trace)
            for (int64_t i = (int64_t)lx * W + lane; i < (int64_t)T * W; i += 64) tr[i] = -1;
    }
}

}  // namespace crf
