// cat_amd/csrc/k_score_grad_body.h -- the bodies of stages 1 (alpha) and 2 (beta) of the score gradient, as k_score_grad.hip describes
// them, for its kernels and for the device-rows entry points of k_rows.hip.  ROWS = false: the rows of occ are the instantiation's own
// 64 NR doubles apart (crf_ctc_score_grad*: one instantiation per call).  ROWS = true: they are p.S doubles apart, the stride of the
// call's widest class, so that the instantiations of several classes write into ONE occ section (crf_ctc_score_grad_rows).
#pragma once
#include "k_lattice_common.h"

namespace crf {

// log(exp(a0) + exp(a1) + exp(a2)) on fp64 operands: the maximum and the result in fp64, the three differences to it, their exponentials
// and the logarithm of the sum (in [1, 3]) in fp32, k_score's operand order.  All -inf: the maximum is raised to -DBL_MAX, the result -inf.
__device__ __forceinline__ double acc_lse3(double a0, double a1, double a2) {
    const double m = fmax(fmax(fmax(a0, a1), a2), -1.7976931348623157e308);
    return m + (double)score_log((score_exp((float)(a0 - m)) + score_exp((float)(a1 - m))) + score_exp((float)(a2 - m)));
}
__device__ __forceinline__ double acc_lse2(double a0, double a1) {
    const double m = fmax(fmax(a0, a1), -1.7976931348623157e308);
    return m + (double)score_log(score_exp((float)(a0 - m)) + score_exp((float)(a1 - m)));
}
// DPP full-wave shifts of an fp64 value, a lane without a source takes -inf: UP = lane l takes lane l - 1's (wave_shr:1), else lane l + 1's
template <bool UP> __device__ __forceinline__ double acc_shift(double v) {
    constexpr int ctrl = UP ? 0x138 : 0x130;
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, ctrl, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)0xfff00000u, (int)(unsigned)(b >> 32), ctrl, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// the lane's NR consecutive doubles at a (a multiple of 8 NR bytes): vector stores / loads of 8 or 16 bytes
template <int NR> __device__ __forceinline__ void alpha_store(double *a, const double (&v)[NR]) {
    if constexpr (NR == 1) a[0] = v[0];
    else {
#pragma unroll
        for (int i = 0; i < NR; i += 2) *(double2 *)(a + i) = make_double2(v[i], v[i + 1]);
    }
}
template <int NR> __device__ __forceinline__ void alpha_load(double (&v)[NR], const double *a) {
    if constexpr (NR == 1) v[0] = a[0];
    else {
#pragma unroll
        for (int i = 0; i < NR; i += 2) { const double2 q = *(const double2 *)(a + i); v[i] = q.x; v[i + 1] = q.y; }
    }
}
// the lane's NR consecutive floats at a (a multiple of 4 NR bytes): one vector store of 4, 8 or 16 bytes, two for NR = 8
template <int NR> __device__ __forceinline__ void occ_store(float *a, const float (&v)[NR]) {
    if constexpr (NR == 1) a[0] = v[0];
    else if constexpr (NR == 2) *(float2 *)a = make_float2(v[0], v[1]);
    else {
#pragma unroll
        for (int i = 0; i < NR; i += 4) *(float4 *)(a + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    }
}

// What stages 1 and 2 share: the wave's hypothesis, whether it is live, its utterance's rows and its rows of occ.
template <typename E> struct ScoreGradHyp {
    int h, lx, Sx;
    float score;

    const int *ul;
    const E *xb;
    double *ab;                 // the lane's alphas of frame 0: frame t's are S doubles further per frame
    float *ob;                  // the lane's occupancies of frame 0, at the start of the same rows: 2 S floats further per frame
};
// false: the wave has nothing to do (no hypothesis, or one that is invalid, scores -inf or weighs exactly 0: stage 3 skips it by the same
// rule).  A live hypothesis is a valid one: u in [0, B), every label in [0, V), 0 < lx, 2 L + 1 <= S.  COPY: the score goes to the caller.
template <int NR, bool COPY, bool ROWS = false, typename E>
__device__ __forceinline__ bool score_grad_hyp(const ScoreGradParams &p, int lane, ScoreGradHyp<E> &y) {
    const int rs = ROWS ? p.S : NR * 64;      // doubles per row of occ
    const int64_t hw = (int64_t)blockIdx.x * kScoreWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (hw >= p.H) return false;
    y.h = (int)hw;
    const float score = p.hscore[y.h];
    if (COPY && lane == 0 && p.score) p.score[y.h] = score;
    const float w = p.weight ? p.weight[y.h] : 1.f;
    if (!(score > -INFINITY) || w == 0.f) return false;
    const int u = p.hyp_utt[y.h];
    y.lx = min(p.lx[u], p.T);
    y.score = score;
    y.Sx = 2 * p.hyp_len[y.h] + 1;
    y.ul = p.labels + p.hyp_off[y.h];
    y.xb = (const E *)p.x + (int64_t)u * p.xs_b;
    y.ab = (double *)p.occ + ((int64_t)y.h * p.T) * rs + lane * NR;
    y.ob = p.occ + ((int64_t)y.h * p.T) * (2 * rs) + lane * NR;
    return true;
}

// Stage 1 on the element type E (float: log-probs or raw output; AlnBf16 / AlnF16: raw output, upcast in registers by lat_ld).
template <int NR, typename E, bool ROWS = false>
__device__ __forceinline__ void score_grad_alpha_body(const ScoreGradParams p) {
    constexpr int S = NR * 64;                // states this instantiation holds
    constexpr int PF = NR >= 8 ? 2 : NR == 4 ? 4 : 8;   // frames per emission prefetch batch (two register sets in flight)
    const int rs = ROWS ? p.S : S;            // doubles per row of occ
    const int lane = threadIdx.x & 63;
    ScoreGradHyp<E> y;
    if (!score_grad_hyp<NR, true, ROWS>(p, lane, y)) return;   // (no barrier in this kernel: waves leave on their own)
    const int lx = y.lx, Sx = y.Sx;

    unsigned labo[NR];                        // the state's column as a byte offset into a row
    bool skip[NR];
    double v[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int s = lane * NR + i;
        const int l = (s < Sx && (s & 1)) ? y.ul[s >> 1] : p.blank;
        labo[i] = (unsigned)l * (unsigned)sizeof(E);
        skip[i] = (s & 1) && s >= 2 && s < Sx && y.ul[(s >> 1) - 1] != l;
        v[i] = s == 0 ? 0.0 : -__builtin_huge_val();
    }
    auto fetch = [&](float (&e)[PF][NR], int t) __attribute__((always_inline)) { lat_fetch<PF, NR, E>(e, y.xb, p.xs_t, lx, labo, t); };
    const double kNegInf = -__builtin_huge_val();
    // One frame, crf_ctc_score_wave_kernel's on the fp64 vector; a frame at or past lx does nothing (the loop runs in whole batches).
    auto frame = [&](const float (&e)[NR], int t) __attribute__((always_inline)) {
        if (t >= lx) return;                  // (the whole wave)
        double n[NR];
        if constexpr (NR == 1) {
            const double a1 = acc_shift<true>(v[0]);
            const double a2 = acc_shift<true>(a1);
            n[0] = (double)e[0] + acc_lse3(v[0], a1, skip[0] ? a2 : kNegInf);
        } else {
            const double below = acc_shift<true>(v[NR - 1]);
            n[0] = (double)e[0] + acc_lse2(v[0], below);
            n[1] = (double)e[1] + acc_lse3(v[1], v[0], skip[1] ? below : kNegInf);
#pragma unroll
            for (int i = 2; i < NR; ++i)
                n[i] = (i & 1) ? (double)e[i] + acc_lse3(v[i], v[i - 1], skip[i] ? v[i - 2] : kNegInf) : (double)e[i] + acc_lse2(v[i], v[i - 1]);
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) v[i] = n[i];
        alpha_store<NR>(y.ab + (int64_t)t * rs, v);
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
}

// Stage 2 on the element type E.  LSE (raw output): y.score is the NORMALISED score, float(double(raw) - sum_t lse_t), while alpha and
// beta are those of the upcast values themselves; the raw sum-product the exponent needs is double(score) + sum_t lse_t, the sum taken
// as the score kernel took it (lat_lse_sum_wave).  What is left of the score's fp32 rounding is common to a frame: stage 3 normalises.
template <int NR, typename E, bool LSE, bool ROWS = false>
__device__ __forceinline__ void score_grad_beta_body(const ScoreGradParams p, const float *lse) {
    constexpr int S = NR * 64;
    constexpr int PF = NR >= 8 ? 2 : NR == 4 ? 4 : 8;   // frames per prefetch batch of emissions and stored alphas (two register sets in flight)
    const int rs = ROWS ? p.S : S;            // doubles per row of occ
    const int lane = threadIdx.x & 63;
    ScoreGradHyp<E> y;
    if (!score_grad_hyp<NR, false, ROWS>(p, lane, y)) return;
    const int lx = y.lx, Sx = y.Sx;
    double lsum = 0.0;
    if constexpr (LSE) lsum = lat_lse_sum_wave(lse + (int64_t)p.hyp_utt[y.h] * p.T, lx, lane);

    unsigned labo[NR];
    bool skipn[NR];                           // state s + 2 exists and may be entered from s
    double b[NR];                             // beta_t
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int s = lane * NR + i;
        const int l = (s < Sx && (s & 1)) ? y.ul[s >> 1] : p.blank;
        labo[i] = (unsigned)l * (unsigned)sizeof(E);
        skipn[i] = (s & 1) && s + 2 < Sx && y.ul[(s >> 1) + 1] != l;
        b[i] = (s == Sx - 1 || s == Sx - 2) ? 0.0 : -__builtin_huge_val();
    }
    const double kNegInf = -__builtin_huge_val();
    // frames t, t - 1, ..., t - PF + 1, clamped to frame 0: unconditional loads, as lat_fetch's
    auto fetch = [&](float (&e)[PF][NR], double (&a)[PF][NR], int t) __attribute__((always_inline)) {
#pragma unroll
        for (int f = 0; f < PF; ++f) {
            const int tt = max(t - f, 0);
            const char *row = (const char *)(y.xb + (int64_t)tt * p.xs_t);
#pragma unroll
            for (int i = 0; i < NR; ++i) e[f][i] = lat_ld<E>(row + labo[i]);
            alpha_load<NR>(a[f], y.ab + (int64_t)tt * rs);
        }
    };
    // One frame: the occupancies of frame t over its alphas, then beta_{t-1}; a frame below 0 does neither.
    auto frame = [&](const float (&e)[NR], const double (&a)[NR], int t) __attribute__((always_inline)) {
        if (t < 0) return;                    // (the whole wave)
        double c[NR], n[NR];
        float o[NR];
        const double score = LSE ? (double)y.score + lsum : (double)y.score;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            o[i] = score_exp((float)((a[i] + b[i]) - score));
            c[i] = b[i] + (double)e[i];
        }
        occ_store<NR>(y.ob + (int64_t)t * (2 * rs), o);
        if constexpr (NR == 1) {
            const double a1 = acc_shift<false>(c[0]);
            const double a2 = acc_shift<false>(a1);
            n[0] = acc_lse3(c[0], a1, skipn[0] ? a2 : kNegInf);
        } else {
            const double up0 = acc_shift<false>(c[0]), up1 = acc_shift<false>(c[1]);
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const double c1 = i + 1 < NR ? c[(i + 1) % NR] : up0;
                const double c2 = i + 2 < NR ? c[(i + 2) % NR] : i + 2 == NR ? up0 : up1;
                n[i] = (i & 1) ? acc_lse3(c[i], c1, skipn[i] ? c2 : kNegInf) : acc_lse2(c[i], c1);
            }
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) b[i] = n[i];
    };

    float ea[PF][NR], eb[PF][NR];
    double aa[PF][NR], ab[PF][NR];
    fetch(ea, aa, lx - 1);
    for (int t0 = lx - 1; t0 >= 0; t0 -= 2 * PF) {
        fetch(eb, ab, t0 - PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) frame(ea[f], aa[f], t0 - f);
        fetch(ea, aa, t0 - 2 * PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) frame(eb[f], ab[f], t0 - PF - f);
    }
}

}  // namespace crf
