// cat_amd/csrc/k_score_grad.hip -- the weighted gradient of H hypothesis scores over B utterances, written as ONE [B][T][V] tensor: the
// backward half of k_score.hip.  Host side: crf_ctc_score_grad / crf_ctc_score_grad_logits (crf_host_ctc.hip).
//
//   grad[u][t][v] = sum over h with hyp_utt[h] = u of  w_h * gamma_h[t][v]
//   gamma_h[t][v] = sum over s with lab_h(s) = v of  exp(alpha_t[s] + beta_t[s] - score_h)
//
// Four launches on one stream, the activations read in place and never replicated; what is per hypothesis lives in the workspace
// (occ[h][t]: a row of 64 NR doubles, and the H scores), never in an [H][T][V] tensor.
//   0. crf_ctc_score_wave_kernel<NR> ITSELF (k_score.hip), the instantiation crf_ctc_score takes for max_hyp_len: it writes invalid and,
//      into the workspace, the scores -- the bits crf_ctc_score writes because the same code writes them.
//   1. crf_ctc_score_grad_alpha_kernel<NR>: copies the score out, then for a live hypothesis (valid, score > -inf, weight != 0) the same
//      recursion in the same geometry (one wave per hypothesis, state s = lane * NR + i, DPP wave_shr:1, emissions prefetched two batches
//      ahead) with the state vector CARRIED IN FP64 (acc_lse3 below), and per frame t < lx one vector store of the lane's NR states into
//      occ[h][t] AS THEY ARE, in fp64.  The stored vector is as exact as the carried one whatever the input: no offset is taken off, so
//      none has to be found (a cross-lane step) and none can be wrong.  An fp32 store relative to the ramp (t + 1) score_h / lx was tried
//      first: it is accurate only while the cost per frame is even.  A confident half followed by a costly one leaves the vector
//      |score| / 2 off the ramp at mid-utterance -- 3 000 nats at T = 1 500 -- where one fp32 rounding is 1.2e-4, different from state to
//      state: measured 1.7e-4 .. 2.2e-4 entry-wise on the posteriors (profiles/score_grad_uneven.txt), against the project's 1e-4.
//   2. crf_ctc_score_grad_beta_kernel<NR>: the same backward in time with the mirror-image shift (wave_shl:1, the top lane takes -inf),
//        beta_{lx-1}[s] = 0 for s in {2L, 2L-1}, else -inf
//        beta_t[s] = lse3(c_{t+1}[s], c_{t+1}[s+1], [s+2 may be skipped to] c_{t+1}[s+2]),   c_t[s] = beta_t[s] + x_t[lab(s)]
//      Per frame it reads the stored alpha and writes exp(alpha_t[s] + beta_t[s] - score_h), the sum in fp64, as 64 NR floats over the
//      first half of the same row: every lane holds the row's alphas in registers by then (they were loaded a batch ahead).
//      Neither recursion has a reduction across the wave: with one wave per SIMD whatever a frame waits for delays the next frame.
//   3. crf_ctc_score_grad_reduce_kernel: one workgroup per (utterance, block of FB frames).  It zeroes an LDS row of V floats per frame,
//      lists the live hypotheses of its utterance in ascending h, and per hypothesis and frame sums the 2L+1 occupancies (1 in exact
//      arithmetic: their own sum is the normaliser, which takes out whatever is common to a frame's states -- the fp32 score's own
//      rounding first of all), scales them by w_h / sum and scatters them with LDS float adds onto lab(s) -- as the numerator's grad
//      pass does (k_grad.hip: crf_grad_ctc_kernel), so the gradient is not bit for bit -- and stores the rows.  Frames t >= lx and
//      utterances without a hypothesis keep their zero rows: every entry of grad is written here, nothing is zeroed in front, there is
//      no global atomic.
// Why fp64 carries the vectors of stages 1 and 2: an fp32 log-domain value of magnitude 2^k has an ulp of 2^(k-23), and the vectors grow
// by a few units per frame -- 6e-5 per rounding after 250 frames, two roundings per frame, not common to a frame's states.  Measured with
// fp32 vectors (and a per-frame normaliser): entry-wise error of the posteriors 1e-5 at T = 48, 1e-4 at T = 150, 2.5e-4 at T = 300, against
// the project's 1e-4.  Here only the DIFFERENCES to the frame's maximum go through fp32 (exp and log on the hardware's instructions, sums
// in [1, 3]); the accumulation is fp64, so a frame adds about 1e-7 whatever the magnitude.  The scores stay k_score's fp32 bits.
// -inf flows through: a state at -inf gives exp(-inf) = 0, and there is no +inf to meet it.
//
// Raw network output (crf_ctc_score_grad_logits): the stage bodies are templates on the element type E -- float, or 2-byte bf16 / fp16
// elements upcast in registers by lat_ld -- and the *_raw_kernel<NR, E> instantiations run them behind crf_align_lse_kernel and
// crf_ctc_score_wave_kernel<NR, E, true> (crf_ctc_score_logits' own two launches: the same score bits).  Both recursions run on the upcast
// values THEMSELVES: sum_t lse_t is common to all alignments of a hypothesis, so alpha_t[s] + beta_t[s] exceeds its log_softmax value by
// exactly that sum, and stage 2 takes the RAW sum-product for the exponent, double(score) + sum_t double(lse_t) with the sum in the score
// kernel's order -- the normalised fp32 score is what the workspace holds; half an ulp of it remains, common to a frame, for stage 3's
// normaliser.  Stage 3 adds log_softmax's own term: d / d x of -lse_t is -softmax, once per unit of live weight,
//   grad[u][t][v] = sum_{live h of u} w_h gamma_h[t][v] - W_u exp(x^[u][t][v] - lse_t),   W_u = sum_{live h of u} w_h  (ascending h).
// The kernels under the old names are the float instantiations of the same bodies without any of this (LSE / RAW = false).
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
template <int NR, bool COPY, typename E>
__device__ __forceinline__ bool score_grad_hyp(const ScoreGradParams &p, int lane, ScoreGradHyp<E> &y) {
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
    y.ab = (double *)p.occ + ((int64_t)y.h * p.T) * (NR * 64) + lane * NR;
    y.ob = p.occ + ((int64_t)y.h * p.T) * (2 * NR * 64) + lane * NR;
    return true;
}

// Stage 1 on the element type E (float: log-probs or raw output; AlnBf16 / AlnF16: raw output, upcast in registers by lat_ld).
template <int NR, typename E>
__device__ __forceinline__ void score_grad_alpha_body(const ScoreGradParams p) {
    constexpr int S = NR * 64;                // states this instantiation holds
    constexpr int PF = NR >= 8 ? 2 : NR == 4 ? 4 : 8;   // frames per emission prefetch batch (two register sets in flight)
    const int lane = threadIdx.x & 63;
    ScoreGradHyp<E> y;
    if (!score_grad_hyp<NR, true>(p, lane, y)) return;   // (no barrier in this kernel: waves leave on their own)
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
        alpha_store<NR>(y.ab + (int64_t)t * S, v);
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
template <int NR>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_ctc_score_grad_alpha_kernel(ScoreGradParams p) { score_grad_alpha_body<NR, float>(p); }
template <int NR, typename E>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_ctc_score_grad_alpha_raw_kernel(ScoreGradRawParams p) { score_grad_alpha_body<NR, E>(p); }

// Stage 2 on the element type E.  LSE (raw output): y.score is the NORMALISED score, float(double(raw) - sum_t lse_t), while alpha and
// beta are those of the upcast values themselves; the raw sum-product the exponent needs is double(score) + sum_t lse_t, the sum taken
// as the score kernel took it (lat_lse_sum_wave).  What is left of the score's fp32 rounding is common to a frame: stage 3 normalises.
template <int NR, typename E, bool LSE>
__device__ __forceinline__ void score_grad_beta_body(const ScoreGradParams p, const float *lse) {
    constexpr int S = NR * 64;
    constexpr int PF = NR >= 8 ? 2 : NR == 4 ? 4 : 8;   // frames per prefetch batch of emissions and stored alphas (two register sets in flight)
    const int lane = threadIdx.x & 63;
    ScoreGradHyp<E> y;
    if (!score_grad_hyp<NR, false>(p, lane, y)) return;
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
            alpha_load<NR>(a[f], y.ab + (int64_t)tt * S);
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
        occ_store<NR>(y.ob + (int64_t)t * (2 * S), o);
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
template <int NR>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_ctc_score_grad_beta_kernel(ScoreGradParams p) { score_grad_beta_body<NR, float, false>(p, nullptr); }
template <int NR, typename E>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_ctc_score_grad_beta_raw_kernel(ScoreGradRawParams p) { score_grad_beta_body<NR, E, true>(p, p.lse); }

// Stage 3.  rows: the dynamic LDS, FB rows of V floats; list: the live hypotheses of this utterance among one chunk of h, ascending.
// RAW (raw output of element type E): the gradient with respect to the raw output has log_softmax's term as well,
//   - W_u * exp(x^[u][t][v] - lse_t),   W_u = the sum of the live weights in ascending h (every live hypothesis's occupancies sum to 1 per frame),
// taken off the frames below lx as the rows are stored: thread tid holds the entries v = tid, tid + 256, ... of a row there, the input row is
// read beside them, one element per thread and step, and nothing more goes through LDS.  W_u = 0 (no live hypothesis): the rows stay exact 0.
template <typename E, bool RAW>
__device__ __forceinline__ void score_grad_reduce_body(const ScoreGradParams p, const float *lse, float *rows, int *list, int *wcnt) {
    constexpr int NW = kScoreGradReduceThreads / 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int V = p.V, FB = p.FB, NBT = (p.T + FB - 1) / FB;
    const int u = (int)(blockIdx.x / (unsigned)NBT);
    const int t0 = (int)(blockIdx.x % (unsigned)NBT) * FB;
    const int nf = min(FB, p.T - t0);                              // frames of this block (>= 1)
    const int nl = min(nf, max(min(p.lx[u], p.T) - t0, 0));        // ... below lx: the ones that take occupancies
    const int S = p.S;
    float W = 0.f;                                                 // RAW: the live weights of this utterance (the same value in every thread)

    for (int i = tid; i < nf * V; i += kScoreGradReduceThreads) rows[i] = 0.f;
    __syncthreads();
    for (int h0 = 0; h0 < p.H && nl > 0; h0 += kScoreGradReduceThreads) {
        const int h = h0 + tid;
        bool mine = false;
        if (h < p.H && p.hyp_utt[h] == u) mine = p.hscore[h] > -INFINITY && (p.weight ? p.weight[h] : 1.f) != 0.f;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int base = 0, n = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { base += k < wave ? wcnt[k] : 0; n += wcnt[k]; }
        if (mine) list[base + __popcll(m & ((1ull << lane) - 1ull))] = h;
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const int hk = list[k];
            const int Sx = 2 * p.hyp_len[hk] + 1;
            const int *ul = p.labels + p.hyp_off[hk];
            const float w = p.weight ? p.weight[hk] : 1.f;
            if constexpr (RAW) W += w;
            for (int f = wave; f < nl; f += NW) {
                const float *o = p.occ + ((int64_t)hk * p.T + (t0 + f)) * (2 * S);   // (the floats at the start of a row of S doubles)
                float *row = rows + f * V;
                float z = 0.f;                                     // the frame's occupancies sum to 1: their own sum is the normaliser
                for (int s = lane; s < Sx; s += 64) z += o[s];
#pragma unroll
                for (int j = 32; j > 0; j >>= 1) z += __shfl_xor(z, j);
                const float scale = z > 0.f ? w / z : 0.f;
                for (int s = lane; s < Sx; s += 64) {
                    const float g = o[s] * scale;
                    const int l = (s & 1) ? ul[s >> 1] : p.blank;
                    if (g != 0.f) atomicAdd(row + l, g);           // (an LDS float add; most states of a frame hold an exact 0)
                }
            }
        }
        __syncthreads();                                           // list and wcnt are free again; after the last chunk: the rows are complete
    }
    float *gb = p.grad + (int64_t)u * p.xs_b + (int64_t)t0 * p.xs_t;
    for (int f = 0; f < nf; ++f) {
        float *g = gb + (int64_t)f * p.xs_t;
        const float *row = rows + f * V;
        if constexpr (RAW) {
            if (f < nl && W != 0.f) {                              // (the whole workgroup)
                const char *xr = (const char *)((const E *)p.x + (int64_t)u * p.xs_b + (int64_t)(t0 + f) * p.xs_t);
                const float l = lse[(int64_t)u * p.T + (t0 + f)];
                for (int v = tid; v < V; v += kScoreGradReduceThreads) g[v] = row[v] - W * score_exp(lat_ld<E>(xr + (size_t)v * sizeof(E)) - l);
                continue;
            }
        }
        for (int v = tid; v < V; v += kScoreGradReduceThreads) g[v] = row[v];
    }
}
// Dynamic LDS: FB rows of V floats.  Grid: B * ceil(T / FB) workgroups of kScoreGradReduceThreads.
__global__ __launch_bounds__(kScoreGradReduceThreads) void crf_ctc_score_grad_reduce_kernel(ScoreGradParams p) {
    extern __shared__ __attribute__((aligned(16))) float rows[];   // [FB][V]
    __shared__ int list[kScoreGradReduceThreads];
    __shared__ int wcnt[kScoreGradReduceThreads / 64];
    score_grad_reduce_body<float, false>(p, nullptr, rows, list, wcnt);
}
template <typename E>
__global__ __launch_bounds__(kScoreGradReduceThreads) void crf_ctc_score_grad_reduce_raw_kernel(ScoreGradRawParams p) {
    extern __shared__ __attribute__((aligned(16))) float rows[];   // [FB][V]
    __shared__ int list[kScoreGradReduceThreads];
    __shared__ int wcnt[kScoreGradReduceThreads / 64];
    score_grad_reduce_body<E, true>(p, p.lse, rows, list, wcnt);
}

template __global__ void crf_ctc_score_grad_alpha_kernel<1>(ScoreGradParams);
template __global__ void crf_ctc_score_grad_alpha_kernel<2>(ScoreGradParams);
template __global__ void crf_ctc_score_grad_alpha_kernel<4>(ScoreGradParams);
template __global__ void crf_ctc_score_grad_alpha_kernel<8>(ScoreGradParams);
template __global__ void crf_ctc_score_grad_beta_kernel<1>(ScoreGradParams);
template __global__ void crf_ctc_score_grad_beta_kernel<2>(ScoreGradParams);
template __global__ void crf_ctc_score_grad_beta_kernel<4>(ScoreGradParams);
template __global__ void crf_ctc_score_grad_beta_kernel<8>(ScoreGradParams);
#define CRF_SCORE_GRAD_RAW_INST(E)                                                              \
    template __global__ void crf_ctc_score_grad_alpha_raw_kernel<1, E>(ScoreGradRawParams);     \
    template __global__ void crf_ctc_score_grad_alpha_raw_kernel<2, E>(ScoreGradRawParams);     \
    template __global__ void crf_ctc_score_grad_alpha_raw_kernel<4, E>(ScoreGradRawParams);     \
    template __global__ void crf_ctc_score_grad_alpha_raw_kernel<8, E>(ScoreGradRawParams);     \
    template __global__ void crf_ctc_score_grad_beta_raw_kernel<1, E>(ScoreGradRawParams);      \
    template __global__ void crf_ctc_score_grad_beta_raw_kernel<2, E>(ScoreGradRawParams);      \
    template __global__ void crf_ctc_score_grad_beta_raw_kernel<4, E>(ScoreGradRawParams);      \
    template __global__ void crf_ctc_score_grad_beta_raw_kernel<8, E>(ScoreGradRawParams);      \
    template __global__ void crf_ctc_score_grad_reduce_raw_kernel<E>(ScoreGradRawParams);
CRF_SCORE_GRAD_RAW_INST(float)      // crf_ctc_score_grad_logits
CRF_SCORE_GRAD_RAW_INST(AlnBf16)
CRF_SCORE_GRAD_RAW_INST(AlnF16)
#undef CRF_SCORE_GRAD_RAW_INST

}  // namespace crf
