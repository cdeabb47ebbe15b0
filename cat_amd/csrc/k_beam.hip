// cat_amd/csrc/k_beam.hip -- CTC prefix beam search on the GPU (LM-free): the W best label sequences of every utterance under the prefix
// recursion of include/ctc_crf_hip.h (crf_ctc_beam), with the trace that spells them.  Host side: crf_ctc_beam (crf_host_ctc.hip).
//
// Row stage (crf_beam_row_kernel<E>): one wave per row (n, t), t < lx[n]; 4 rows per workgroup up to kBeamRowsV classes, beyond one.  The
// row is read ONCE into LDS (V words per wave; lane l owns the entries v = l, l + 64, ...; one wave, whose LDS operations complete in
// order: no barrier), with normalize its lse = m + log sum exp(x^ - m) (fp32, each lane its own entries in order, the lanes' sums in
// a butterfly) is taken; then every lane finds the best of its entries once (ascending v: the lowest index of its maximum) and keeps it as a
// key (the value's order-preserving integer image, ~index), and C rounds take the wave maximum of the keys (DPP, no LDS round trip) --
// the largest value at its lowest index: equal values to the lower index -- strike the winner's entry (-inf) and find that lane's next
// best with the whole wave (lane i reads the entries own + 64 i, + 4096, ..: one LDS read per lane instead of a walk over the column by
// one lane; the first version walked every column in every round: 9.8 ms at N = 64, V = 5 000).  Round j gives pair j of E_t;
// where nothing above -inf is left (or only NaN) the pair is (class -1, -inf): an extension at -inf is no candidate, so it changes nothing.
// Workspace: val[n T + t][0] = x^[blank] - lse, val[..][1 + j] = x^[c_j] - lse, cls[..][1 + j] = c_j (cls[..][0] = blank), C + 1 words a row.
//
// Beam stage (crf_beam_search_kernel): ONE wave per utterance, slot k of the beam in lane k, all state in registers (a BeamSlot).  Lane j
// holds pair j of the frame (C <= 64); the next frame's C + 1 words are fetched while this frame is worked on (unconditional loads, frame
// and lane clamped).  Per frame: beam_frame_step, steps 1 to 4 as k_beam_body.h describes them (the streaming search of
// k_beam_chunk.hip calls the same function).
// Back-trace, same launch behind a barrier: the trace rows come back through LDS 64 frames at a time, lane r < nbest follows rank r from
// frame lx - 1 down and stores a label wherever a class was appended (its length is known: the labels land at their final places), then
// the tails take the blank, and with a caller's trace buffer the rows t >= lx take -1.  Every output word is written by one plain store.
#include "k_beam_body.h"   // the frame step, shared with k_beam_chunk.hip; the wave helpers (k_beam_common.h) come with it

namespace crf {

template <typename E>
__global__ __launch_bounds__(256) void crf_beam_row_kernel(BeamParams p) {
    extern __shared__ float beam_rows[];       // [waves of the workgroup][V]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, R = blockDim.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * R + w;
    if (f >= (int64_t)p.B * p.T) return;       // (no barrier in this kernel: waves leave on their own)
    const int n = (int)(f / p.T), t = (int)(f % p.T);
    if (t >= p.lx[n]) return;
    const int V = p.V, C = p.C, RS = C + 1;
    const E *row = (const E *)p.x + ((int64_t)n * p.xs_b + (int64_t)t * p.xs_t);
    float *xr = beam_rows + (size_t)w * V;
    float m = -INFINITY;
#pragma unroll 4
    for (int v = lane; v < V; v += 64) {
        const float x = lat_ld<E>((const char *)(row + v));
        xr[v] = x;
        m = fmaxf(m, x);
    }
    const float xb = lat_ld<E>((const char *)(row + p.blank));
    float lse = 0.f;
    if (p.normalize) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (m == -INFINITY) m = 0.f;
        float s = 0.f;
        for (int v = lane; v < V; v += 64) s += expf(xr[v] - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        lse = m + logf(s);
    }
    if (lane == (p.blank & 63)) xr[p.blank] = -INFINITY;   // the blank is no class of E_t
    // every lane's best entry as a key (value image, ~index): the wave maximum of the keys is the largest value at its lowest index
    unsigned kh, kl;
    {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = lane; v < V; v += 64) {
            const float x = xr[v];
            if (x > bv) { bv = x; bi = v; }    // (ascending v: the lowest index of the lane's maximum; NaN never wins)
        }
        kh = beam_ord(bv); kl = ~(unsigned)bi;
    }
    float myv = -INFINITY;
    int myc = -1;
    for (int j = 0; j < C; ++j) {
        const unsigned mh = beam_wave_umax(kh);
        if (mh <= kBeamOrdNegInf) break;       // (uniform) nothing above -inf is left: the remaining pairs stay (-inf, -1)
        const int bi = (int)~beam_wave_umax(kh == mh ? kl : 0u);
        if (lane == j) { myv = beam_unord(mh) - lse; myc = bi; }
        // the winner's entry is struck, and its lane's next best found by the whole wave: lane i looks at the entries own + 64 i
        // (+ 4096, ..) of that lane's column -- one conflicted LDS read instead of a walk over the column by one lane
        const int own = bi & 63;
        if (lane == own) xr[bi] = -INFINITY;
        float cv = -INFINITY;
        int ci = 0x7fffffff;
        for (int v = own + 64 * lane; v < V; v += 4096) {
            const float x = xr[v];
            if (v != bi && x > cv) { cv = x; ci = v; }
        }
        const unsigned ch = beam_ord(cv), cl = ~(unsigned)ci;
        const unsigned nh = beam_wave_umax(ch);
        const unsigned nl = beam_wave_umax(ch == nh ? cl : 0u);
        if (lane == own) { kh = nh; kl = nl; }
    }
    float *val = p.val + f * RS;
    int *cls = p.cls + f * RS;
    if (lane < C) { val[1 + lane] = myv; cls[1 + lane] = myc; }
    if (lane == 63) { val[0] = xb - lse; cls[0] = p.blank; }
}

__global__ __launch_bounds__(64) void crf_beam_search_kernel(BeamParams p) {
    __shared__ int tr_lds[64 * kBeamMaxW];     // 64 frames of the trace for the back-trace
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = p.T, W = p.W, C = p.C, RS = C + 1;
    const int lx = max(0, min(p.lx[b], T));
    const float *val = p.val + (int64_t)b * T * RS;
    const int *cls = p.cls + (int64_t)b * T * RS;
    int *tr = p.trace + (int64_t)b * T * W;
    const int jl = C > 0 ? 1 + min(lane, C - 1) : 0;   // this lane's word of a row (lanes >= C: clamped, not used)

    BeamSlot s;                                 // the beam: the empty prefix in slot 0
    beam_slot_fresh(s, lane);

    float nv = 0.f, nxb = 0.f;
    int nc = -1;
    if (lx > 0) { nv = val[jl]; nc = cls[jl]; nxb = val[0]; }
    for (int t = 0; t < lx; ++t) {
        const float vj = lane < C ? nv : -INFINITY, xb = nxb;
        const int cj = lane < C ? nc : -1;
        {
            const int64_t o = (int64_t)min(t + 1, lx - 1) * RS;
            nv = val[o + jl]; nc = cls[o + jl]; nxb = val[o];
        }
        beam_frame_step(s, vj, cj, xb, lane, W, C, tr + (int64_t)t * W);
    }

    // results of the ranks, back-trace
    const bool out = lane < p.nbest;
    const int olen = s.alive ? s.len : 0;
    const int64_t h0 = (int64_t)b * p.nbest;
    if (out) {
        p.score[h0 + lane] = s.alive ? (float)beam_lse2(s.pb, s.pnb) : -INFINITY;
        p.hyp_len[h0 + lane] = olen;
    }
    int *hyp = p.hyps + (h0 + (out ? lane : 0)) * T;
    int slot = lane, at = olen;
    for (int t1 = lx; t1 > 0; t1 -= 64) {
        const int t0 = max(0, t1 - 64), nw = (t1 - t0) * W;
        __syncthreads();                        // (the trace rows are this wave's own stores; the chunk before has been read)
        for (int i = lane; i < nw; i += 64) tr_lds[i] = tr[(int64_t)t0 * W + i];
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
    for (int r = 0; r < p.nbest; ++r) {
        const int L = beam_bcast(olen, r);
        int *row = p.hyps + (h0 + r) * T;
        for (int j = L + lane; j < T; j += 64) row[j] = p.blank;
    }
    if (p.fill_trace)
        for (int64_t i = (int64_t)lx * W + lane; i < (int64_t)T * W; i += 64) tr[i] = -1;
}

template __global__ void crf_beam_row_kernel<float>(BeamParams);
template __global__ void crf_beam_row_kernel<AlnBf16>(BeamParams);
template __global__ void crf_beam_row_kernel<AlnF16>(BeamParams);

}  // namespace crf
