// cat_amd/csrc/k_align.hip -- CTC forced alignment: the best path through the numerator's 2L+1 states (the max-plus twin of the forward
// chain in k_chain.hip), with back-pointers and the back-trace in the same launch.  Host side: crf_ctc_align (crf_host_ctc.hip).
//
//   v_t[s] = x[b][t][lab(s)] + max(v_{t-1}[s], v_{t-1}[s-1], v_{t-1}[s-2] if s is odd and lab(s) != lab(s-2))      log domain, fp32
//
// One workgroup of kCtcThreads per utterance, state s = tid + i * kCtcThreads in register set i < NR (the chains' geometry).  Ties go to the
// smallest move (stay, advance, skip; at the end state 2L before 2L-1): the comparisons below are strict, in that order.
// Frame 0 is an ordinary frame on the virtual vector v_{-1} = (0, -inf, -inf, ...): x + 0 is exact, and it yields v_0[0] = x[blank],
// v_0[1] = x[lab(1)], -inf elsewhere.  States s >= 2L+1 of the last register set run along on the blank's column: values only move UP the
// state axis, so nothing they hold reaches a real state, and they are never stored.
//
// Back-pointers: 2 bits per (frame, state), the move taken into the state.  A thread keeps the moves of 16 consecutive frames of its state
// in one register and stores the word once per 16 frames:  bp[b][t / 16][s], bits 2 (t % 16) ..  -- coalesced along s, and every word of
// the blocks [0, ceil(lx / 16)) x [0, 2L+1) is written before the back-trace starts (the workspace may hold anything).
// Back-trace: the state falls by at most 2 per frame, so the words of the next kAlnG blocks (64 frames) for the 32 kAlnG states below the
// current one are ONE word per thread: the workgroup fetches that tile into LDS in one pass (one dependent global round trip per 64 frames
// instead of one per frame), and wave 0 walks it -- per block of 16 frames 32 lanes take their state's word from LDS, the walk itself is
// v_readlane + scalar arithmetic, and the 16 positions of the block leave as one store of 16 lanes.
//
// Raw network output (crf_ctc_align_logits): the kernel is instantiated on the element type E -- float, or 2-byte bf16 / fp16 elements
// upcast in registers -- and runs the SAME recursion on the upcast values: every alignment takes one entry of each of its lx frames, so
// log_softmax's normaliser sum_t lse_t is common to all of them and the best path is the same.  crf_align_lse_kernel writes lse[b][t]
// in front of it; with LSE the workgroup sums its utterance's lse values in fp64 in a fixed order at the end (k_lattice_common.h: the
// order is part of the contract) and the score is float(double(raw best sum) - that sum).
#include "k_lattice_common.h"

namespace crf {

// lse[b][t] = m + log sum_v exp(x[b][t][v] - m), m = max_v x[b][t][v], fp32, for the frames t < lx[b] (the others are never written, and
// never read).  G lanes per frame: a lane adds its entries v = sub, sub + G, ... in that order, the lanes' sums meet in a butterfly -- the
// same arithmetic in either layout.  expf / logf, not the fast intrinsics: this kernel is memory-bound and not on the chain.
template <int G, typename E>
__global__ __launch_bounds__(256) void crf_align_lse_kernel(AlignParams p) {
    const int sub = threadIdx.x & (G - 1);
    const int64_t f = (int64_t)blockIdx.x * (256 / G) + (threadIdx.x / G);
    if (f >= (int64_t)p.B * p.T) return;
    const int b = (int)(f / p.T), t = (int)(f % p.T);
    if (t >= p.lx[b]) return;                     // (whole groups of G lanes leave together)
    const E *row = (const E *)p.x + ((int64_t)b * p.xs_b + (int64_t)t * p.xs_t);
    float m = -INFINITY, s = 0.f;
    constexpr int NX = 16;                        // row entries a lane keeps between the two passes
    if (p.V <= NX * G) {
        float x[NX];
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            const int v = sub + k * G;
            x[k] = v < p.V ? lat_ld<E>((const char *)(row + v)) : -INFINITY;
            m = fmaxf(m, x[k]);
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, G));
        if (m == -INFINITY) m = 0.f;
#pragma unroll
        for (int k = 0; k < NX; ++k)
            if (sub + k * G < p.V) s += expf(x[k] - m);
    } else {
        for (int v = sub; v < p.V; v += G) m = fmaxf(m, lat_ld<E>((const char *)(row + v)));
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, G));
        if (m == -INFINITY) m = 0.f;
        for (int v = sub; v < p.V; v += G) s += expf(lat_ld<E>((const char *)(row + v)) - m);
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, G);
    if (sub == 0) p.lse[f] = m + logf(s);
}

template <int NR, typename E, bool LSE>
__global__ __launch_bounds__(kCtcThreads) void crf_ctc_align_kernel(AlignParams p) {
    constexpr int S = NR * kCtcThreads;       // states this instantiation holds
    constexpr int PF = NR == 1 ? 8 : 4;      // frames per emission prefetch batch (two register sets in flight)
    static_assert((2 * PF) <= kAlnFrames && kAlnFrames % (2 * PF) == 0, "a back-pointer word is closed at the end of a loop iteration");
    static_assert(kAlnG * 2 * kAlnFrames * kAlnG == kCtcThreads, "the back-trace tile is one word per thread");
    __shared__ float A[2][S + 2];             // v of the previous / this frame, two -inf entries in front of state 0
    __shared__ int lab[S];
    __shared__ unsigned tile[kCtcThreads];
    __shared__ int red[kCtcWaves];
    __shared__ int ctl[2];                    // [0] the back-trace's current state, [1] 1 = a path exists

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int lx = min(p.lx[b], p.T), L = p.ly[b];
    const bool fits = L >= 0 && 2 * L + 1 <= S;
    const int Sx = fits ? 2 * L + 1 : 1;
    int *prow = p.pos + (int64_t)b * p.T;

    const bool valid = lat_valid(fits, lx, L, lat_wg_labels(p.labels + p.lab_off[b], L, fits, p.blank, p.V, lab, red, A, tid, lane, wave));
    for (int t = tid; t < p.T; t += kCtcThreads)
        if (!valid || t >= lx) prow[t] = -2;
    if (!valid) {
        if (tid == 0) { p.score[b] = -INFINITY; if (p.invalid) p.invalid[b] = 1; }
        return;
    }

    unsigned labo[NR];                        // the state's column as a byte offset into a row
    bool skip[NR];
    unsigned bpw[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        lat_wg_state<E>(lab, Sx, tid + i * kCtcThreads, labo[i], skip[i], A);
        bpw[i] = 0u;
    }
    __syncthreads();

    const E *xb = (const E *)p.x + (int64_t)b * p.xs_b;
    unsigned *bpb = p.bp + (int64_t)b * p.NB * p.Sc;
    auto fetch = [&](float (&e)[PF][NR], int t) __attribute__((always_inline)) { lat_fetch<PF, NR, E>(e, xb, p.xs_t, lx, labo, t); };
    // One frame; a frame at or past lx copies the vector (the loop runs in whole batches).
    auto frame = [&](const float (&e)[NR], int t) __attribute__((always_inline)) {
        const float *Ac = &A[t & 1][2];
        float *An = &A[(t + 1) & 1][2];
        const bool live = t < lx;
        const int sh = 2 * (t & (kAlnFrames - 1));
        float a0[NR], a1[NR], a2[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int s = tid + i * kCtcThreads;
            a0[i] = Ac[s]; a1[i] = Ac[s - 1]; a2[i] = Ac[s - 2];
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int s = tid + i * kCtcThreads;
            const float c2 = skip[i] ? a2[i] : -INFINITY;
            float best = a0[i];
            unsigned mv = 0u;
            if (a1[i] > best) { best = a1[i]; mv = 1u; }
            if (c2 > best) { best = c2; mv = 2u; }
            An[s] = live ? e[i] + best : a0[i];
            bpw[i] |= mv << sh;
        }
        sync_lds();
    };

    float ea[PF][NR], eb[PF][NR];
    fetch(ea, 0);
    int t0 = 0;
    for (; t0 < lx; t0 += 2 * PF) {
        fetch(eb, t0 + PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) frame(ea[f], t0 + f);
        fetch(ea, t0 + 2 * PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) frame(eb[f], t0 + PF + f);
        if (((t0 + 2 * PF) & (kAlnFrames - 1)) == 0 || t0 + 2 * PF >= lx) {    // the block of 16 frames is complete, or the utterance is
            unsigned *w = bpb + (int64_t)(t0 / kAlnFrames) * p.Sc;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int s = tid + i * kCtcThreads;
                if (s < Sx) w[s] = bpw[i];
                bpw[i] = 0u;
            }
        }
    }
    __syncthreads();                          // the back-pointer words are in memory, the last vector in LDS
    [[maybe_unused]] float raw = 0.f;         // (thread 0: the best sum of raw entries)
    if (tid == 0) {
        const float *Af = &A[t0 & 1][2];      // t0 frames have run
        float best = Af[Sx - 1];
        int s = Sx - 1;
        if (Sx > 1 && Af[Sx - 2] > best) { best = Af[Sx - 2]; s = Sx - 2; }
        const bool alive = best > -INFINITY;  // (false for NaN as well)
        ctl[0] = s; ctl[1] = alive ? 1 : 0;
        p.score[b] = alive ? best : -INFINITY;
        if (p.invalid) p.invalid[b] = 0;
        raw = best;
    }
    __syncthreads();
    if (!ctl[1]) {                            // a valid label sequence, no alignment of non-zero probability
        for (int t = tid; t < lx; t += kCtcThreads) prow[t] = -2;
        return;
    }
    if constexpr (LSE) {
        // score = raw best sum - sum_{t < lx} lse_t in fp64, in the fixed order of k_lattice_common.h
        __shared__ double lred[kCtcWaves];
        const double sum = lat_lse_sum_wg(p.lse + (int64_t)b * p.T, lx, lred, tid, lane, wave);
        if (tid == 0) p.score[b] = (float)((double)raw - sum);
    }

    constexpr int kTileStates = 2 * kAlnFrames * kAlnG;   // 128 states below the current one
    for (int blk = (lx - 1) / kAlnFrames; blk >= 0; blk -= kAlnG) {
        const int s_top = __builtin_amdgcn_readfirstlane(ctl[0]);
        {
            const int bj = blk - tid / kTileStates, st = s_top - (tid & (kTileStates - 1));
            tile[tid] = (bj >= 0 && st >= 0) ? bpb[(int64_t)bj * p.Sc + st] : 0u;
        }
        __syncthreads();
        if (wave == 0) {
            int cur = s_top;
            for (int j = 0; j < kAlnG && blk - j >= 0; ++j) {
                const int bj = blk - j, tb = bj * kAlnFrames;
                const int c0 = cur;           // s_top - c0 <= 32 j: lanes 0 .. 31 hold the words of the states c0, c0 - 1, ...
                const int w = lane < 2 * kAlnFrames ? (int)tile[j * kTileStates + (s_top - c0) + lane] : 0;
                int val = -2;
                for (int t = min(lx - 1, tb + kAlnFrames - 1); t >= tb; --t) {
                    const int k = t & (kAlnFrames - 1);
                    val = lane == k ? ((cur & 1) ? (cur >> 1) : -1) : val;
                    const unsigned word = (unsigned)__builtin_amdgcn_readlane(w, c0 - cur);   // c0 - cur <= 30 inside a block
                    cur -= (int)((word >> (2 * k)) & 3u);
                }
                if (lane < kAlnFrames && tb + lane < lx) prow[tb + lane] = val;
            }
            if (lane == 0) ctl[0] = cur;
        }
        __syncthreads();
    }
}

#define CRF_ALN_INST(E, LSE)                                                    \
    template __global__ void crf_ctc_align_kernel<1, E, LSE>(AlignParams);        \
    template __global__ void crf_ctc_align_kernel<2, E, LSE>(AlignParams);        \
    template __global__ void crf_ctc_align_kernel<4, E, LSE>(AlignParams);        \
    template __global__ void crf_ctc_align_kernel<kCtcRegs, E, LSE>(AlignParams);
CRF_ALN_INST(float, false)      // crf_ctc_align: log-probs
CRF_ALN_INST(float, true)       // crf_ctc_align_logits
CRF_ALN_INST(AlnBf16, true)
CRF_ALN_INST(AlnF16, true)
#undef CRF_ALN_INST
#define CRF_LSE_INST(E)                                                      \
    template __global__ void crf_align_lse_kernel<16, E>(AlignParams);       \
    template __global__ void crf_align_lse_kernel<64, E>(AlignParams);
CRF_LSE_INST(float)
CRF_LSE_INST(AlnBf16)
CRF_LSE_INST(AlnF16)
#undef CRF_LSE_INST

}  // namespace crf
