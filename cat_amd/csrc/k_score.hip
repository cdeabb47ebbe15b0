// cat_amd/csrc/k_score.hip -- forward-only CTC log-likelihoods of H hypotheses over B utterances: the sum-product twin of k_align.hip, with
// no backward chain, no gradient and no back-pointers.  Host side: crf_ctc_score / crf_ctc_score_logits (crf_host_ctc.hip).
//
//   v_t[s] = x[u][t][lab(s)] + log(exp(v_{t-1}[s]) + exp(v_{t-1}[s-1]) + [s odd and lab(s) != lab(s-2)] exp(v_{t-1}[s-2]))     u = hyp_utt[h]
//   score[h] = logaddexp(v[2L], v[2L-1])  after the lx[u] frames of the utterance
//
// Log domain, fp32, the largest term subtracted, ONE operand order (score_lse3 / score_lse2, k_lattice_common.h: stay, advance, skip; at the end 2L,
// 2L-1): a hypothesis's score depends on its own labels and its utterance's rows only -- not on its place in the list, on its
// neighbours or on the layout -- and is the same bits in every call that takes the same instantiation.  -inf flows through: an
// all -inf triple stays -inf (the maximum is raised to -FLT_MAX before it is subtracted), -inf + anything finite is -inf, and there is no +inf.
// Frame 0 is an ordinary frame on the virtual vector v_{-1} = (0, -inf, -inf, ...), as in k_align.hip.  The activations are read in
// place, never replicated: the hypotheses of one utterance reread its rows out of L2.
//
// Wave geometry (crf_ctc_score_wave_kernel, 2 max_hyp_len + 1 <= 64 NR, NR in 1, 2, 4, 8): one wave per hypothesis, kScoreWaves waves per
// workgroup, state s = lane * NR + i in register i.  The vector lives in registers; what crosses lanes is the last state of the lane
// below (NR >= 2: states 0 and 1 of a lane take it, and s is odd exactly when i is, so state 0 never skips) or the states of the two lanes
// below (NR = 1) -- DPP full-wave shifts, no LDS, no barrier, no wait on anything but the emissions.  Those are gathered straight from the
// caller's tensor two batches of PF frames ahead, unconditionally (frame clamped to lx - 1, idle states on the blank's column).
// Workgroup geometry (crf_ctc_score_wg_kernel, up to kMaxCtcLabelLen): kCtcThreads x NR, state s = tid + i * kCtcThreads, the vector in
// LDS twice and one LDS-only barrier per frame, exactly as k_align.hip lays it out.
//
// Raw network output (crf_ctc_score_logits): the SAME recursion on the upcast values -- every alignment takes one entry of each of
// the lx frames, so log_softmax's normaliser sum_t lse_t is common to all of them -- and score = float(double(raw) - sum_t double(lse[u][t])),
// the lse values written by crf_align_lse_kernel in front, their sum taken in fp64 in the fixed order of k_lattice_common.h.
// A hypothesis is valid by the alignment's rule (lat_valid, k_lattice_common.h).
#include "k_lattice_common.h"

namespace crf {

template <int NR, typename E, bool LSE>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_ctc_score_wave_kernel(ScoreParams p) {
    constexpr int S = NR * 64;                // states this instantiation holds
    constexpr int PF = NR >= 8 ? 2 : NR == 4 ? 4 : 8;   // frames per emission prefetch batch (two register sets in flight)
    const int lane = threadIdx.x & 63;
    const int64_t hw = (int64_t)blockIdx.x * kScoreWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (hw >= p.H) return;                    // (no barrier in this kernel: waves leave on their own)
    const int h = (int)hw;
    const int u = p.hyp_utt[h], L = p.hyp_len[h];
    const bool fits = (unsigned)u < (unsigned)p.B && L >= 0 && 2 * L + 1 <= S;
    const int lx = fits ? min(p.lx[u], p.T) : 0;
    const int Sx = fits ? 2 * L + 1 : 1;
    const int *ul = p.labels + p.hyp_off[h];

    unsigned labo[NR];                        // the state's column as a byte offset into a row
    bool skip[NR];
    int cnt = 0;                              // repeats | out-of-range labels << 12  (each <= 255)
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int s = lane * NR + i;
        int l = p.blank;
        skip[i] = false;
        if (s < Sx && (s & 1)) {
            l = ul[s >> 1];
            const int lp = s >= 2 ? ul[(s >> 1) - 1] : -1;
            if ((unsigned)l >= (unsigned)p.V) { cnt += 1 << 12; l = p.blank; }
            else if (s >= 2 && l == lp) cnt += 1;
            else skip[i] = s >= 2;
        }
        labo[i] = (unsigned)l * (unsigned)sizeof(E);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (!lat_valid(fits, lx, L, cnt)) {
        if (lane == 0) { p.score[h] = -INFINITY; if (p.invalid) p.invalid[h] = 1; }
        return;
    }

    const E *xb = (const E *)p.x + (int64_t)u * p.xs_b;
    auto fetch = [&](float (&e)[PF][NR], int t) __attribute__((always_inline)) { lat_fetch<PF, NR, E>(e, xb, p.xs_t, lx, labo, t); };
    float v[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) v[i] = (lane == 0 && i == 0) ? 0.f : -INFINITY;
    // One frame; a frame at or past lx keeps the vector (the loop runs in whole batches).
    auto frame = [&](const float (&e)[NR], int t) __attribute__((always_inline)) {
        const bool live = t < lx;
        float n[NR];
        if constexpr (NR == 1) {
            const float a1 = score_shift_up(v[0]);
            const float a2 = score_shift_up(a1);
            n[0] = e[0] + score_lse3(v[0], a1, skip[0] ? a2 : -INFINITY);
        } else {
            const float below = score_shift_up(v[NR - 1]);
            n[0] = e[0] + score_lse2(v[0], below);
            n[1] = e[1] + score_lse3(v[1], v[0], skip[1] ? below : -INFINITY);
#pragma unroll
            for (int i = 2; i < NR; ++i)
                n[i] = (i & 1) ? e[i] + score_lse3(v[i], v[i - 1], skip[i] ? v[i - 2] : -INFINITY) : e[i] + score_lse2(v[i], v[i - 1]);
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) v[i] = live ? n[i] : v[i];
    };

    float ea[PF][NR], eb[PF][NR];
    fetch(ea, 0);
    for (int t0 = 0; t0 < lx; t0 += 2 * PF) {
        fetch(eb, t0 + PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) frame(ea[f], t0 + f);
        fetch(ea, t0 + 2 * PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) frame(eb[f], t0 + PF + f);
    }

    // states 2L and 2L-1: each in one register of one lane
    float mine0 = -INFINITY, mine1 = -INFINITY;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int s = lane * NR + i;
        mine0 = s == Sx - 1 ? v[i] : mine0;
        mine1 = s == Sx - 2 ? v[i] : mine1;
    }
    const float last = __shfl(mine0, (Sx - 1) / NR);
    const float prev = Sx > 1 ? __shfl(mine1, (Sx - 2) / NR) : -INFINITY;
    const float raw = score_lse2(last, prev);
    float out = raw;
    if constexpr (LSE) {
        const double sum = lat_lse_sum_wave(p.lse + (int64_t)u * p.T, lx, lane);
        out = raw > -INFINITY ? (float)((double)raw - sum) : -INFINITY;
    }
    if (lane == 0) { p.score[h] = out; if (p.invalid) p.invalid[h] = 0; }
}

template <int NR, typename E, bool LSE>
__global__ __launch_bounds__(kCtcThreads) void crf_ctc_score_wg_kernel(ScoreParams p) {
    constexpr int S = NR * kCtcThreads;       // states this instantiation holds
    constexpr int PF = 4;                     // frames per emission prefetch batch (two register sets in flight)
    __shared__ float A[2][S + 2];             // v of the previous / this frame, two -inf entries in front of state 0
    __shared__ int lab[S];
    __shared__ int red[kCtcWaves];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x;
    const int u = p.hyp_utt[h], L = p.hyp_len[h];
    const bool fits = (unsigned)u < (unsigned)p.B && L >= 0 && 2 * L + 1 <= S;
    const int lx = fits ? min(p.lx[u], p.T) : 0;
    const int Sx = fits ? 2 * L + 1 : 1;

    if (!lat_valid(fits, lx, L, lat_wg_labels(p.labels + p.hyp_off[h], L, fits, p.blank, p.V, lab, red, A, tid, lane, wave))) {   // (the whole workgroup: nothing below is reached)
        if (tid == 0) { p.score[h] = -INFINITY; if (p.invalid) p.invalid[h] = 1; }
        return;
    }

    unsigned labo[NR];
    bool skip[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) lat_wg_state<E>(lab, Sx, tid + i * kCtcThreads, labo[i], skip[i], A);
    __syncthreads();

    const E *xb = (const E *)p.x + (int64_t)u * p.xs_b;
    auto fetch = [&](float (&e)[PF][NR], int t) __attribute__((always_inline)) { lat_fetch<PF, NR, E>(e, xb, p.xs_t, lx, labo, t); };
    auto frame = [&](const float (&e)[NR], int t) __attribute__((always_inline)) {
        const float *Ac = &A[t & 1][2];
        float *An = &A[(t + 1) & 1][2];
        const bool live = t < lx;
        float a0[NR], a1[NR], a2[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int s = tid + i * kCtcThreads;
            a0[i] = Ac[s]; a1[i] = Ac[s - 1]; a2[i] = Ac[s - 2];
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int s = tid + i * kCtcThreads;
            An[s] = live ? e[i] + score_lse3(a0[i], a1[i], skip[i] ? a2[i] : -INFINITY) : a0[i];
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
    }
    const float *Af = &A[t0 & 1][2];          // t0 frames have run (the last frame's barrier has passed)
    const float raw = score_lse2(Af[Sx - 1], Sx > 1 ? Af[Sx - 2] : -INFINITY);
    if constexpr (LSE) {
        __shared__ double lred[kCtcWaves];
        const double sum = lat_lse_sum_wg(p.lse + (int64_t)u * p.T, lx, lred, tid, lane, wave);
        if (tid == 0) {
            p.score[h] = raw > -INFINITY ? (float)((double)raw - sum) : -INFINITY;
            if (p.invalid) p.invalid[h] = 0;
        }
    } else {
        if (tid == 0) { p.score[h] = raw; if (p.invalid) p.invalid[h] = 0; }
    }
}

#define CRF_SCORE_INST(E, LSE)                                                          \
    template __global__ void crf_ctc_score_wave_kernel<1, E, LSE>(ScoreParams);         \
    template __global__ void crf_ctc_score_wave_kernel<2, E, LSE>(ScoreParams);         \
    template __global__ void crf_ctc_score_wave_kernel<4, E, LSE>(ScoreParams);         \
    template __global__ void crf_ctc_score_wave_kernel<8, E, LSE>(ScoreParams);         \
    template __global__ void crf_ctc_score_wg_kernel<2, E, LSE>(ScoreParams);           \
    template __global__ void crf_ctc_score_wg_kernel<4, E, LSE>(ScoreParams);           \
    template __global__ void crf_ctc_score_wg_kernel<kCtcRegs, E, LSE>(ScoreParams);
CRF_SCORE_INST(float, false)    // crf_ctc_score: log-probs
CRF_SCORE_INST(float, true)     // crf_ctc_score_logits
CRF_SCORE_INST(AlnBf16, true)
CRF_SCORE_INST(AlnF16, true)
#undef CRF_SCORE_INST

}  // namespace crf
