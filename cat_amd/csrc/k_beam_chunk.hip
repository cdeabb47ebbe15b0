// cat_amd/csrc/k_beam_chunk.hip -- streaming CTC prefix beam search: the searches of k_beam.hip and k_beam_lm.hip on a CHUNK of frames, with the
// beam loaded from a record at the start and stored to another at the end (include/ctc_crf_hip.h crf_ctc_beam_chunk; host side:
// crf_host_ctc.hip).  The row stage is k_beam.hip's crf_beam_row_kernel<E> on the chunk's rows, unchanged.  The frame steps are the
// device functions of k_beam_body.h / k_beam_lm_body.h, the ones crf_beam_search_kernel / crf_beamlm_search_kernel call (the steps are
// described there), so any split of an utterance's frames into chunks gives the bits of the whole call.
//
// crf_beam_chunk_kernel (one wave per utterance) and crf_beamlm_chunk_kernel (kBeamLmWaves waves, wave 0 searches):
//   Load.    Slot k's fields of the input record (crf_kernels_decl.h: beam_state_bytes) into lane k; a fresh utterance (no input state, or
//            its reset word set) takes the searches' start instead and its record is never read.  With the LM, st_lds / na_lds are
//            rebuilt from the loaded slots (the live slots are 0 .. na - 1).  Whatever a record holds, no access leaves the buffers: the
//            LM state is clamped, lengths are clamped where they index.
//   Frames.  The frame step for t < lx_chunk, the chunk's trace rows as in the whole call.
//   Trace.   Back-trace of the chunk for ALL W slots, 64 frames at a time through LDS: lane k follows slot k down to the chunk's first
//            frame and stores every appended label at its final place `--at` (at = len at the start) of row k of the output record --
//            places >= cap are skipped, the search itself never looks at a row -- and ends in the slot s0(k) of the INPUT beam it
//            descends from, with at = that slot's length.
//   Gather.  Row k of the output record takes the first min(at, cap) words of input row s0(k): a uniform loop over k, the whole
//            workgroup copying consecutive words (coalesced), places from min(len, cap) on take the blank.  The words between were the
//            back-trace's: every word of a row is written once.  Rows k < nbest go to hyps as well.
//   Store.   The slots' fields, the ranks' lengths and scores, the record's padding (zero).
// Only plain vector loads and stores.
#include "k_beam_lm_body.h"

namespace crf {

// slot `lane`'s fields: the start of the searches (fresh), or the input record's; lanes >= W hold nothing
__device__ __forceinline__ void beam_state_load(const char *rin, const bool fresh, const int lane, const int W, const int lm_start,
                                                const int S1, BeamSlot &s, double &lm, int &lms) {
    beam_slot_fresh(s, lane);
    lm = 0.0;
    lms = lane == 0 ? lm_start : 0;
    if (fresh) return;
    if (lane < W) {
        const int64_t w = W;
        s.pb = ((const double *)rin)[lane];
        s.pnb = ((const double *)(rin + 8 * w))[lane];
        lm = ((const double *)(rin + 16 * w))[lane];
        s.id = ((const beam_u64 *)(rin + 24 * w))[lane];
        s.pid = ((const beam_u64 *)(rin + 32 * w))[lane];
        s.alive = ((const int *)(rin + 40 * w))[lane] != 0;
        s.e = ((const int *)(rin + 44 * w))[lane];
        s.len = ((const int *)(rin + 48 * w))[lane];
        lms = min(max(((const int *)(rin + 52 * w))[lane], 0), S1);
    } else {
        lms = 0;
    }
}

// everything behind the frames, by all NT threads of the workgroup; the beam is wave 0's (lane = tid there)
template <int NT>
__device__ __forceinline__ void beam_chunk_finish(const BeamChunkParams &cp, const int b, const int lxc, const bool fresh, const int tid,
                                                  const BeamSlot &s, const double lm, const int lms, const bool with_lm, int *tr,
                                                  int *tr_lds, int *s0_lds, int *n_lds, int *len_lds) {
    const BeamParams &p = cp.q.b;
    const int T = p.T, W = p.W, cap = cp.cap, lane = tid;
    const bool wave0 = tid < 64, mine = wave0 && lane < W, out = wave0 && lane < p.nbest;
    char *rout = cp.state_out + (int64_t)b * cp.rec;
    const char *rin = cp.state_in ? cp.state_in + (int64_t)b * cp.rec : rout;    // (without an input state: any address, never read)
    int *orows = (int *)(rout + beam_state_rows_off(W));
    const int *irows = (const int *)(rin + beam_state_rows_off(W));    // (never read where fresh: no words are taken from it)
    const int64_t h0 = (int64_t)b * p.nbest;
    // the slots' fields and the ranks' results
    if (mine) {
        const int64_t w = W;
        ((double *)rout)[lane] = s.pb;
        ((double *)(rout + 8 * w))[lane] = s.pnb;
        ((double *)(rout + 16 * w))[lane] = lm;
        ((beam_u64 *)(rout + 24 * w))[lane] = s.id;
        ((beam_u64 *)(rout + 32 * w))[lane] = s.pid;
        ((int *)(rout + 40 * w))[lane] = s.alive;
        ((int *)(rout + 44 * w))[lane] = s.e;
        ((int *)(rout + 48 * w))[lane] = s.len;
        ((int *)(rout + 52 * w))[lane] = lms;
    }
    {
        const int64_t used = beam_state_rows_off(W) + 4 * (int64_t)W * cap;
        if (tid < (int)((cp.rec - used) >> 2)) ((int *)(rout + used))[tid] = 0;    // the record's padding: at most 3 words
    }
    if (out) {
        const double ac = beam_lse2(s.pb, s.pnb);
        p.score[h0 + lane] = !s.alive ? -INFINITY : with_lm ? (float)(ac + lm) : (float)ac;
        p.hyp_len[h0 + lane] = s.alive ? s.len : 0;
        if (with_lm && cp.q.lm_score) cp.q.lm_score[h0 + lane] = s.alive ? (float)lm : 0.f;
    }
    // the chunk's back-trace, every slot
    const bool follow = mine && s.alive;
    int *orow = orows + (int64_t)(mine ? lane : 0) * cap;
    int *hyp = p.hyps + (h0 + (out ? lane : 0)) * cap;
    int slot = mine ? lane : 0, at = follow ? s.len : 0;
    for (int t1 = lxc; t1 > 0; t1 -= 64) {
        const int t0 = max(0, t1 - 64), nw = (t1 - t0) * W;
        __syncthreads();                        // (the trace rows are wave 0's own stores; the window before has been read)
        for (int i = tid; i < nw; i += NT) tr_lds[i] = tr[(int64_t)t0 * W + i];
        __syncthreads();
        if (follow) {
            for (int t = t1 - 1; t >= t0; --t) {
                const int wd = tr_lds[(t - t0) * W + slot];
                const int c = (wd >> 6) - 1;
                slot = min(wd & 63, W - 1);     // (a live slot's word is never -1; the clamp keeps any word inside the row)
                if (c >= 0 && at > 0) {
                    --at;
                    if (at < cap) {
                        orow[at] = c;
                        if (out) hyp[at] = c;
                    }
                }
            }
        }
    }
    // the rows' heads from the input beam, their tails the blank
    __syncthreads();
    if (wave0) {
        s0_lds[lane] = slot;
        n_lds[lane] = fresh ? 0 : min(max(at, 0), cap);
        len_lds[lane] = follow ? min(max(s.len, 0), cap) : 0;
    }
    __syncthreads();
    for (int k = 0; k < W; ++k) {
        const int n = n_lds[k], L = max(len_lds[k], n);
        const int *src = irows + (int64_t)s0_lds[k] * cap;
        int *dst = orows + (int64_t)k * cap;
        int *hdst = p.hyps + (h0 + k) * cap;
        const bool to_hyp = k < p.nbest;
#pragma unroll 4
        for (int j = tid; j < cap; j += NT) {
            if (j >= n && j < L) continue;      // (the back-trace's words)
            const int v = j < n ? src[j] : p.blank;
            dst[j] = v;
            if (to_hyp) hdst[j] = v;
        }
    }
    if (wave0 && p.fill_trace)
        for (int64_t i = (int64_t)lxc * W + lane; i < (int64_t)T * W; i += 64) tr[i] = -1;
}

__global__ __launch_bounds__(64) void crf_beam_chunk_kernel(BeamChunkParams cp) {
    __shared__ int tr_lds[64 * kBeamMaxW];     // 64 frames of the trace for the back-trace
    __shared__ int s0_lds[64], n_lds[64], len_lds[64];
    const BeamParams &p = cp.q.b;
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = p.T, W = p.W, C = p.C, RS = C + 1;
    const int lxc = max(0, min(p.lx[b], T));
    const float *val = p.val + (int64_t)b * T * RS;
    const int *cls = p.cls + (int64_t)b * T * RS;
    int *tr = p.trace + (int64_t)b * T * W;
    const int jl = C > 0 ? 1 + min(lane, C - 1) : 0;   // this lane's word of a row (lanes >= C: clamped, not used)
    const bool fresh = !cp.state_in || (cp.reset && cp.reset[b] != 0);

    BeamSlot s;
    double lm;
    int lms;
    beam_state_load(fresh ? nullptr : cp.state_in + (int64_t)b * cp.rec, fresh, lane, W, 0, 0, s, lm, lms);

    float nv = 0.f, nxb = 0.f;
    int nc = -1;
    if (lxc > 0) { nv = val[jl]; nc = cls[jl]; nxb = val[0]; }
    for (int t = 0; t < lxc; ++t) {
        const float vj = lane < C ? nv : -INFINITY, xb = nxb;
        const int cj = lane < C ? nc : -1;
        {
            const int64_t o = (int64_t)min(t + 1, lxc - 1) * RS;
            nv = val[o + jl]; nc = cls[o + jl]; nxb = val[o];
        }
        beam_frame_step(s, vj, cj, xb, lane, W, C, tr + (int64_t)t * W);
    }
    beam_chunk_finish<64>(cp, b, lxc, fresh, lane, s, lm, lms, false, tr, tr_lds, s0_lds, n_lds, len_lds);
}

__global__ __launch_bounds__(64 * kBeamLmWaves) void crf_beamlm_chunk_kernel(BeamChunkParams cp) {
    __shared__ float lm_w[64 * kBeamLmStride];  // [slot][place] lmw of the slot's extension by the class at that place of E_t
    __shared__ int lm_n[64 * kBeamLmStride];    // ... and its next LM state; behind the frames: 64 frames of the trace for the back-trace
    __shared__ int st_lds[kBeamMaxW];           // the slots' LM states
    __shared__ int na_lds;                      // live slots: 0 .. na - 1
    __shared__ NgramDev lm_lds;                 // the tables' pointers and sizes (k_beam_lm.hip: read per lookup from LDS)
    __shared__ BeamChunkParams cp_lds;          // the arguments for behind the frames, for the same reason: held in scalar registers
                                                // across the frame loop they do not fit beside the search's (spills)
    __shared__ int s0_lds[64], n_lds[64], len_lds[64];
    const BeamLmParams &q = cp.q;
    const BeamParams &p = q.b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int T = p.T, W = p.W, C = p.C, RS = C + 1;
    const int lxc = max(0, min(p.lx[b], T));
    const int S1 = max(q.lm.S, 1) - 1;
    const float *val = p.val + (int64_t)b * T * RS;
    const int *cls = p.cls + (int64_t)b * T * RS;
    int *tr = p.trace + (int64_t)b * T * W;
    const int jl = C > 0 ? 1 + min(lane, C - 1) : 0;   // this lane's word of a row (lanes >= C: clamped, not used)
    const bool fresh = !cp.state_in || (cp.reset && cp.reset[b] != 0);

    // the beam (wave 0; the other waves hold a copy they never use)
    BeamSlot s;
    double lm;
    int lms;
    beam_state_load(fresh ? nullptr : cp.state_in + (int64_t)b * cp.rec, fresh, lane, W, min(max(q.lm.start, 0), S1), S1, s, lm, lms);

    for (int i = tid; i < 64 * kBeamLmStride; i += 64 * kBeamLmWaves) { lm_w[i] = 0.f; lm_n[i] = 0; }
    if (wave == 0) {
        st_lds[lane] = lms;
        const beam_u64 live = __ballot(s.alive != 0);
        if (lane == 0) { na_lds = __popcll(live); lm_lds = q.lm; cp_lds = cp; }
    }
    __syncthreads();

    float nv = 0.f, nxb = 0.f;
    int nc = -1;
    if (wave == 0 && lxc > 0) { nv = val[jl]; nc = cls[jl]; nxb = val[0]; }
    for (int t = 0; t < lxc; ++t) {
        {
            const NgramDev lmt = lm_lds;
            beamlm_frame_lookups<64 * kBeamLmWaves>(lmt, q.alpha, q.beta, cls + (int64_t)t * RS + 1, na_lds, W, C, tid, st_lds, lm_w, lm_n);
        }
        __syncthreads();
        if (wave == 0) {
            const float vj = lane < C ? nv : -INFINITY, xb = nxb;
            const int cj = lane < C ? nc : -1;
            {
                const int64_t o = (int64_t)min(t + 1, lxc - 1) * RS;
                nv = val[o + jl]; nc = cls[o + jl]; nxb = val[o];
            }
            beamlm_frame_step(s, lm, lms, vj, cj, xb, lane, W, C, S1, tr + (int64_t)t * W, lm_w, lm_n, st_lds, &na_lds);
        }
        __syncthreads();
    }
    beam_chunk_finish<64 * kBeamLmWaves>(cp_lds, b, lxc, fresh, tid, s, lm, lms, true, tr, lm_n, s0_lds, n_lds, len_lds);
}

}  // namespace crf
