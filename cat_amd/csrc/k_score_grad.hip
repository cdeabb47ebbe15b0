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
#include "k_score_grad_body.h"   // the bodies of stages 1 and 2, shared with k_rows.hip

namespace crf {

template <int NR>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_ctc_score_grad_alpha_kernel(ScoreGradParams p) { score_grad_alpha_body<NR, float>(p); }
template <int NR, typename E>
__global__ __launch_bounds__(kScoreWaves * 64) void crf_ctc_score_grad_alpha_raw_kernel(ScoreGradRawParams p) { score_grad_alpha_body<NR, E>(p); }

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
