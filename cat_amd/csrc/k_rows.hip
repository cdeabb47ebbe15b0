// cat_amd/csrc/k_rows.hip -- hypotheses that lie on the device as padded rows (what crf_ctc_sample and crf_ctc_beam write): the kernel
// choice of the score and score-gradient calls made PER HYPOTHESIS on the device, since the host cannot know the longest hypothesis
// without a synchronisation.  Host side: crf_ctc_score_rows / crf_ctc_score_grad_rows (crf_host_ctc.hip).
//
// The length classes are the seven instantiations the score call chooses from (rows_class below): one wave per hypothesis with 1, 2, 4,
// 8 states per lane (L <= 31, 63, 127, 255), one workgroup with 2, 4, 8 states per thread (L <= 511, 1023, 2047).  The host knows a bound
// len_cap on the lengths and launches the classes 0 .. rows_class(len_cap), each one the EXISTING kernel of k_score.hip on all H
// hypotheses with a masked length row:
//   crf_rows_plan_kernel   one pass over hyp_len: hyp_off[h] = h * stride, cls[h] = the class of L = hyp_len[h] (kRowsNoClass for L < 0,
//                          L > len_cap or L > stride), and per launched class c the row len_c[h] = L where cls[h] = c, else -1.  A length
//                          of -1 fails the score kernels' `fits` test: the wave (workgroup) loads no label and no emission and leaves after
//                          one store, -inf / invalid = 1 into its class's rows.
//   crf_rows_merge_kernel  score[h] = score_{cls[h]}[h], invalid[h] = invalid_{cls[h]}[h]; without a class -inf and 1.
// Every hypothesis is thus scored by the instantiation of its own class: the bits crf_ctc_score writes for a list whose longest
// hypothesis lies in that class, whatever else the list holds.
//
// The gradient (the four wave classes): per class the score kernel, then stages 1 and 2 of k_score_grad.hip on len_c and the class's own
// scores -- a masked-out hypothesis scores -inf there, so both stages leave its rows of occ alone -- through the entry points below,
// which differ from crf_ctc_score_grad_alpha / beta_kernel in ONE thing: the rows of occ are p.S doubles apart, the stride of len_cap's
// class, not the instantiation's own 64 NR, so that all classes write into one occ section and the one reduce launch
// (crf_ctc_score_grad_reduce*_kernel as it is: it has always indexed by p.S) reads the merged scores and the true lengths behind them.
#include "k_score_grad_body.h"

namespace crf {

__global__ __launch_bounds__(kRowsThreads) void crf_rows_plan_kernel(RowsPlanParams p) {
    const int h = blockIdx.x * kRowsThreads + threadIdx.x;
    if (h >= p.H) return;
    const int L = p.hyp_len[h];
    const int c = (L < 0 || L > p.len_cap || L > p.stride) ? kRowsNoClass : rows_class(L);
    p.hyp_off[h] = h * p.stride;              // (H * stride <= INT32_MAX: the host has checked)
    p.cls[h] = c;
    for (int k = 0; k < p.ncls; ++k) p.len_c[(int64_t)k * p.H + h] = k == c ? L : -1;
}

__global__ __launch_bounds__(kRowsThreads) void crf_rows_merge_kernel(RowsMergeParams p) {
    const int h = blockIdx.x * kRowsThreads + threadIdx.x;
    if (h >= p.H) return;
    const int c = p.cls[h];
    const bool has = (unsigned)c < (unsigned)p.ncls;
    const float s = has ? p.cscore[(int64_t)c * p.H + h] : -INFINITY;
    const int inv = has ? p.cinvalid[(int64_t)c * p.H + h] : 1;
    if (p.score) p.score[h] = s;
    if (p.hscore) p.hscore[h] = s;
    if (p.invalid) p.invalid[h] = inv;
}

template <int NR>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_rows_grad_alpha_kernel(ScoreGradParams p) { score_grad_alpha_body<NR, float, true>(p); }
template <int NR, typename E>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_rows_grad_alpha_raw_kernel(ScoreGradRawParams p) { score_grad_alpha_body<NR, E, true>(p); }
template <int NR>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_rows_grad_beta_kernel(ScoreGradParams p) { score_grad_beta_body<NR, float, false, true>(p, nullptr); }
template <int NR, typename E>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_rows_grad_beta_raw_kernel(ScoreGradRawParams p) { score_grad_beta_body<NR, E, true, true>(p, p.lse); }

template __global__ void crf_rows_grad_alpha_kernel<1>(ScoreGradParams);
template __global__ void crf_rows_grad_alpha_kernel<2>(ScoreGradParams);
template __global__ void crf_rows_grad_alpha_kernel<4>(ScoreGradParams);
template __global__ void crf_rows_grad_alpha_kernel<8>(ScoreGradParams);
template __global__ void crf_rows_grad_beta_kernel<1>(ScoreGradParams);
template __global__ void crf_rows_grad_beta_kernel<2>(ScoreGradParams);
template __global__ void crf_rows_grad_beta_kernel<4>(ScoreGradParams);
template __global__ void crf_rows_grad_beta_kernel<8>(ScoreGradParams);
#define CRF_ROWS_GRAD_RAW_INST(E)                                                          \
    template __global__ void crf_rows_grad_alpha_raw_kernel<1, E>(ScoreGradRawParams);     \
    template __global__ void crf_rows_grad_alpha_raw_kernel<2, E>(ScoreGradRawParams);     \
    template __global__ void crf_rows_grad_alpha_raw_kernel<4, E>(ScoreGradRawParams);     \
    template __global__ void crf_rows_grad_alpha_raw_kernel<8, E>(ScoreGradRawParams);     \
    template __global__ void crf_rows_grad_beta_raw_kernel<1, E>(ScoreGradRawParams);      \
    template __global__ void crf_rows_grad_beta_raw_kernel<2, E>(ScoreGradRawParams);      \
    template __global__ void crf_rows_grad_beta_raw_kernel<4, E>(ScoreGradRawParams);      \
    template __global__ void crf_rows_grad_beta_raw_kernel<8, E>(ScoreGradRawParams);
CRF_ROWS_GRAD_RAW_INST(float)       // crf_ctc_score_grad_rows on raw network output
CRF_ROWS_GRAD_RAW_INST(AlnBf16)
CRF_ROWS_GRAD_RAW_INST(AlnF16)
#undef CRF_ROWS_GRAD_RAW_INST

}  // namespace crf
