// cat_amd/csrc/k_beam_lm.hip -- CTC prefix beam search with shallow fusion of a token-level n-gram LM (include/ctc_crf_hip.h
// crf_ctc_beam_lm; host side: crf_host_ctc.hip).  The row stage is k_beam.hip's crf_beam_row_kernel<E>, unchanged, with its workspace
// records (val / cls, [B T][C + 1]); this file holds the fused search of the whole utterance.
//
// crf_beamlm_search_kernel: ONE workgroup of kBeamLmWaves waves per utterance.  The beam lives in the registers of wave 0 (a BeamSlot,
// the prefix' LM state and lm = alpha * log P_lm(prefix) + beta * len).  Per frame, parts A (all waves: the frame's LM lookups into the
// two LDS matrices, beamlm_frame_lookups) and B (wave 0: steps 1 to 4 with a head per slot, beamlm_frame_step) as k_beam_lm_body.h
// describes them (the streaming search of k_beam_chunk.hip calls the same functions), a barrier behind each.
// Waits per frame: two barriers, the lookups' vector-memory waits in A (what bounds the frame: DESIGN.md 7 (f11)), the prefetched row of
// the next frame in B (issued a frame ahead), LDS waits on the matrix reads.
// Back-trace as in crf_beam_search_kernel; the trace rows come back through lm_n's LDS (all waves copy, wave 0 follows the ranks).
#include "k_beam_lm_body.h"   // the frame step, shared with k_beam_chunk.hip

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
    const float *val = p.val + (int64_t)b * T * RS;
    const int *cls = p.cls + (int64_t)b * T * RS;
    int *tr = p.trace + (int64_t)b * T * W;
    int *tr_lds = lm_n;
    const int jl = C > 0 ? 1 + min(lane, C - 1) : 0;   // this lane's word of a row (lanes >= C: clamped, not used)

    for (int i = tid; i < 64 * kBeamLmStride; i += 64 * kBeamLmWaves) { lm_w[i] = 0.f; lm_n[i] = 0; }
    if (tid < kBeamMaxW) st_lds[tid] = tid == 0 ? min(max(q.lm.start, 0), S1) : 0;
    if (tid == 0) { na_lds = 1; lm_lds = q.lm; }
    __syncthreads();

    // the beam (wave 0): the empty prefix in slot 0
    BeamSlot s;
    beam_slot_fresh(s, lane);
    double lm = 0.0;
    int lms = lane == 0 ? min(max(q.lm.start, 0), S1) : 0;

    float nv = 0.f, nxb = 0.f;
    int nc = -1;
    if (wave == 0 && lx > 0) { nv = val[jl]; nc = cls[jl]; nxb = val[0]; }
    for (int t = 0; t < lx; ++t) {
        {
            const NgramDev lmt = lm_lds;
            beamlm_frame_lookups<64 * kBeamLmWaves>(lmt, q.alpha, q.beta, cls + (int64_t)t * RS + 1, na_lds, W, C, tid, st_lds, lm_w, lm_n);
        }
        __syncthreads();
        if (wave == 0) {
            const float vj = lane < C ? nv : -INFINITY, xb = nxb;
            const int cj = lane < C ? nc : -1;
            {
                const int64_t o = (int64_t)min(t + 1, lx - 1) * RS;
                nv = val[o + jl]; nc = cls[o + jl]; nxb = val[o];
            }
            beamlm_frame_step(s, lm, lms, vj, cj, xb, lane, W, C, S1, tr + (int64_t)t * W, lm_w, lm_n, st_lds, &na_lds);
        }
        __syncthreads();
    }

    // results of the ranks, back-trace
    const bool out = wave == 0 && lane < p.nbest;
    const int olen = s.alive ? s.len : 0;
    const int64_t h0 = (int64_t)b * p.nbest;
    if (out) {
        p.score[h0 + lane] = s.alive ? (float)(beam_lse2(s.pb, s.pnb) + lm) : -INFINITY;
        p.hyp_len[h0 + lane] = olen;
        if (q.lm_score) q.lm_score[h0 + lane] = s.alive ? (float)lm : 0.f;
    }
    int *hyp = p.hyps + (h0 + (out ? lane : 0)) * T;
    int slot = lane, at = olen;
    for (int t1 = lx; t1 > 0; t1 -= 64) {
        const int t0 = max(0, t1 - 64), nw = (t1 - t0) * W;
        __syncthreads();                        // (the trace rows are wave 0's stores; the chunk before has been read)
        for (int i = tid; i < nw; i += 64 * kBeamLmWaves) tr_lds[i] = tr[(int64_t)t0 * W + i];
        __syncthreads();
        if (out && s.alive) {
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
