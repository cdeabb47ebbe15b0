// cat_amd/csrc/crf_kernels_decl.h -- what the host side (crf_host.hip, crf_host_ctc.hip) needs to know of the kernel families: their argument blocks, the constants
// that size grids and LDS, and the DECLARATIONS of the kernel templates.  The definitions live in k_*.hip, one translation unit per family,
// each of which instantiates explicitly what the host launches.
#pragma once
#include "crf_device.h"

namespace crf {

// ---- k_chain.hip ----
template <int G> __global__ void crf_prep_kernel(LossParams p);
__global__ void crf_stage_i32_kernel(int *__restrict__ dst, const int *__restrict__ src, int64_t n);
__global__ void crf_gate_kernel(const int *started, int target);
template <bool GV> __global__ void crf_den_pair_kernel(LossParams p);
template <int NR> __global__ void crf_ctc_pair_kernel(LossParams p);
__global__ void crf_ctc_check_kernel(LossParams p);

// ---- k_align.hip ----
constexpr int kAlnFrames = 16;   // frames per back-pointer word (2 bits per frame and state)
constexpr int kAlnG = 4;         // blocks of kAlnFrames frames per back-trace tile: kAlnG x (2 kAlnFrames kAlnG) words, one per thread
// Kernel arguments of the forced alignment (crf_ctc_align, crf_ctc_align_logits): the activations are read in place, row (b, t) at
// b * xs_b + t * xs_t ELEMENTS (floats; with raw network output in 16 bits, AlnBf16 / AlnF16)
struct AlnBf16 { unsigned short u; };   // element types of the kernel template: two bytes, upcast in registers (a shift / a convert)
struct AlnF16 { _Float16 h; };
struct AlignParams {
    const void *x;
    const int *labels, *lab_off, *lx, *ly;
    int B, T, V, blank;
    int Sc, NB;                 // back-pointer words: [B][NB = ceil(T / kAlnFrames)][Sc = 2 * max_label_len + 1 rounded up to 64]
    int64_t xs_b, xs_t;
    unsigned *bp;
    int *pos;                   // [B][T]
    float *score;               // [B]
    int *invalid;               // [B] or null
    float *lse;                 // [B][T] crf_ctc_align_logits: log sum_v exp(x[b][t][v]) of the frames t < lx[b] (crf_align_lse_kernel)
};
// E: float, AlnBf16, AlnF16.  LSE: the score is normalised, raw best sum - sum_t lse[b][t] in fp64 (raw network output).
template <int NR, typename E = float, bool LSE = false> __global__ void crf_ctc_align_kernel(AlignParams p);
// lanes per frame of the lse kernel: 16 for rows of up to 256 entries (four frames per wave), else a whole wave
constexpr int kAlnLseSmallV = 256;
template <int G, typename E> __global__ void crf_align_lse_kernel(AlignParams p);

// ---- k_score.hip ----
constexpr int kScoreWaves = 4;            // hypotheses (waves) per workgroup of the wave geometry
constexpr int kScoreWaveMaxStates = 512;  // 2 max_hyp_len + 1 up to here: one wave per hypothesis (64 lanes x 8 states), beyond: one workgroup
// Kernel arguments of the hypothesis scores (crf_ctc_score, crf_ctc_score_logits): hypothesis h is the labels [hyp_off[h], + hyp_len[h])
// on the rows of utterance hyp_utt[h]; the activations as for the alignment (row (u, t) at u * xs_b + t * xs_t ELEMENTS, read in place)
struct ScoreParams {
    const void *x;
    const int *labels, *hyp_off, *hyp_len, *hyp_utt, *lx;
    int B, H, T, V, blank;
    int64_t xs_b, xs_t;
    float *score;               // [H]
    int *invalid;               // [H] or null
    const float *lse;           // [B][T] crf_ctc_score_logits: the frames' normalisers (crf_align_lse_kernel), else null
};
// E: float, AlnBf16, AlnF16.  LSE: score = raw sum-product - sum_t lse[u][t] in fp64 (raw network output).
template <int NR, typename E = float, bool LSE = false> __global__ void crf_ctc_score_wave_kernel(ScoreParams p);   // NR 1, 2, 4, 8
template <int NR, typename E = float, bool LSE = false> __global__ void crf_ctc_score_wg_kernel(ScoreParams p);     // NR 2, 4, kCtcRegs

// ---- k_score_grad.hip ----
constexpr int kScoreGradMaxLen = 255;     // the wave geometry only: 2 max_hyp_len + 1 <= kScoreWaveMaxStates
constexpr int kScoreGradMaxV = 8192;      // the reduce stage keeps a row of V floats per frame in LDS: 32 KiB per row at most
constexpr int kScoreGradFrames = 8;       // ... and up to this many frames per workgroup (fewer beyond V = 1024: at most 32 KiB of rows)
constexpr int kScoreGradReduceThreads = 256;
// Kernel arguments of crf_ctc_score_grad: ScoreParams' fields, then the weights, the workspace sections and the output
struct ScoreGradParams {
    const void *x;
    const int *labels, *hyp_off, *hyp_len, *hyp_utt, *lx;
    int B, H, T, V, blank;
    int64_t xs_b, xs_t;
    float *score;               // [H] or null
    int *invalid;               // [H] or null
    const float *weight;        // [H] or null: all 1
    float *occ;                 // [H][T] rows of S doubles, workspace; rows t < lx of live hypotheses: alpha_t[s] in fp64 after stage 1; after stage 2 S floats exp(alpha + beta - score) at the row's start
    float *hscore;              // [H] workspace: the score as crf_ctc_score_wave_kernel wrote it (-inf for an invalid hypothesis)
    float *grad;                // the activations' layout: row (u, t) at u * xs_b + t * xs_t
    int S, FB;                  // states per row of occ (64 NR); frames per workgroup of the reduce stage
};
template <int NR> __global__ void crf_ctc_score_grad_alpha_kernel(ScoreGradParams p);   // NR 1, 2, 4, 8
template <int NR> __global__ void crf_ctc_score_grad_beta_kernel(ScoreGradParams p);
__global__ void crf_ctc_score_grad_reduce_kernel(ScoreGradParams p);   // dynamic LDS: FB x V words
// crf_ctc_score_grad_logits: the same on raw network output of element type E (float, AlnBf16, AlnF16) -- hscore is then the normalised
// score crf_ctc_score_wave_kernel<NR, E, true> wrote, and grad takes log_softmax's term as well.  A block of its own, so that the
// kernels above keep their arguments.
struct ScoreGradRawParams : ScoreGradParams {
    const float *lse;           // [B][T] workspace: the frames' normalisers (crf_align_lse_kernel)
};
template <int NR, typename E> __global__ void crf_ctc_score_grad_alpha_raw_kernel(ScoreGradRawParams p);   // NR 1, 2, 4, 8
template <int NR, typename E> __global__ void crf_ctc_score_grad_beta_raw_kernel(ScoreGradRawParams p);
template <typename E> __global__ void crf_ctc_score_grad_reduce_raw_kernel(ScoreGradRawParams p);          // dynamic LDS: FB x V words

// ---- k_rows.hip ----
constexpr int kRowsThreads = 256;         // hypotheses per workgroup of the plan and merge kernels
constexpr int kRowsClasses = 7;           // the score call's instantiations: wave NR 1, 2, 4, 8, then workgroup NR 2, 4, 8
constexpr int kRowsWaveClasses = 4;       // ... the first four: the gradient's
constexpr int kRowsNoClass = -1;          // a length < 0, above the call's len_cap or above the row stride
// the class of a hypothesis of L >= 0 labels: the instantiation launch_score (crf_host_ctc.hip) takes for max_hyp_len = L
__host__ __device__ constexpr int rows_class(int L) {
    return L <= 31 ? 0 : L <= 63 ? 1 : L <= 127 ? 2 : L <= 255 ? 3 : L <= 511 ? 4 : L <= 1023 ? 5 : 6;
}
static_assert(2 * 255 + 1 <= kScoreWaveMaxStates && 2 * 256 + 1 > kScoreWaveMaxStates && kScoreGradMaxLen == 255 && kCtcThreads == 512 && kCtcRegs == 8,
              "rows_class follows the wave and workgroup geometries of k_score.hip");
// Kernel arguments of the plan: hypothesis h is the first hyp_len[h] words of row h, rows `stride` words apart
struct RowsPlanParams {
    const int *hyp_len;         // [H]
    int H, stride, len_cap, ncls;   // ncls = rows_class(len_cap) + 1 classes are launched
    int *hyp_off;               // [H] h * stride
    int *cls;                   // [H] the class, or kRowsNoClass
    int *len_c;                 // [ncls][H] hyp_len[h] where cls[h] = c, else -1
};
// ... and of the merge: the per-class results [ncls][H] into the caller's vectors (each may be null)
struct RowsMergeParams {
    const int *cls;
    const float *cscore;
    const int *cinvalid;
    int H, ncls;
    float *score, *hscore;
    int *invalid;
};
__global__ void crf_rows_plan_kernel(RowsPlanParams p);
__global__ void crf_rows_merge_kernel(RowsMergeParams p);
// stages 1 and 2 of the score gradient with the rows of occ p.S doubles apart (k_score_grad_body.h, ROWS)
template <int NR> __global__ void crf_rows_grad_alpha_kernel(ScoreGradParams p);   // NR 1, 2, 4, 8
template <int NR> __global__ void crf_rows_grad_beta_kernel(ScoreGradParams p);
template <int NR, typename E> __global__ void crf_rows_grad_alpha_raw_kernel(ScoreGradRawParams p);
template <int NR, typename E> __global__ void crf_rows_grad_beta_raw_kernel(ScoreGradRawParams p);

// ---- k_sample.hip ----
constexpr int kSampleSmallV = 256;       // rows of up to here: 16 lanes per row and 16 rows per workgroup, beyond: a wave per row and workgroup
constexpr int kSampleMaxV = 8192;         // the row and its running sums are staged in LDS: 32.5 KiB per row at most
constexpr int kSampleWaves = 4;           // paths (waves) per workgroup of the collapse
constexpr int kSampleRowThreads(int G) { return G == 16 ? 256 : 64; }
// Kernel arguments of crf_ctc_sample: the activations as for the alignment (row (n, t) at n * xs_b + t * xs_t ELEMENTS, read in place)
struct SampleParams {
    const void *x;
    const int *lx;
    int B, T, V, K, blank;
    unsigned seed_lo, seed_hi, offset;
    int64_t xs_b, xs_t;
    int *cls;                   // [B K][T] the class drawn per frame (workspace; frames t >= lx are never written, and never read)
    int *hyps, *hyp_len;        // [B K][T], [B K]
    int *paths;                 // [B K][T] or null
};
// G lanes per row: 16, 64.  E: float, AlnBf16, AlnF16.  GREEDY: the arg-max instead of the K draws (K = 1).  Dynamic LDS: (rows per
// workgroup) x (V + 2 G) words, none with GREEDY.
template <int G, typename E, bool GREEDY> __global__ void crf_sample_row_kernel(SampleParams p);
__global__ void crf_sample_collapse_kernel(SampleParams p);

// ---- k_beam.hip ----
constexpr int kBeamMaxW = 64;             // beam slots: one lane each
constexpr int kBeamMaxC = 64;             // classes per frame that take part besides the blank: one lane each, one bit each of a slot's mask
constexpr int kBeamMaxV = 8192;           // the row stage keeps a row of V floats per wave in LDS: 32 KiB per row at most
constexpr int kBeamRowsV = 4096;          // rows of up to here: four waves (rows) per workgroup of the row stage, beyond one: at most 64 KiB of rows
// Kernel arguments of crf_ctc_beam: the activations as for the alignment (row (n, t) at n * xs_b + t * xs_t ELEMENTS, read in place)
struct BeamParams {
    const void *x;
    const int *lx;
    int B, T, V, blank;
    int W, nbest, C, normalize; // C: min(top_classes, V - 1)
    int fill_trace;             // trace is the caller's buffer: its rows t >= lx take -1
    int64_t xs_b, xs_t;
    float *val;                 // [B T][C + 1] workspace, rows t < lx: the blank's value, then the C values of E_t in descending order
    int *cls;                   // [B T][C + 1] workspace: the blank, then their classes (-1: no class left above -inf)
    int *trace;                 // [B][T][W] the caller's trace_dev or the workspace: parent slot + 64 (class + 1), -1 for an empty slot
    int *hyps, *hyp_len;        // [B nbest][T], [B nbest]
    float *score;               // [B nbest]
};
// E: float, AlnBf16, AlnF16; one wave per row, blockDim.x / 64 rows per workgroup; dynamic LDS: that many x V words
template <typename E> __global__ void crf_beam_row_kernel(BeamParams p);
__global__ void crf_beam_search_kernel(BeamParams p);   // one wave (workgroup) per utterance

// ---- k_beam_lm.hip ----
constexpr int kBeamLmWaves = 4;           // waves per utterance of the fused search: all resolve the frame's LM lookups, the first one searches
constexpr int kBeamLmStride = 65;         // words a row of the two LDS matrices [slot][place] takes: 64 and one of padding (bank conflicts)
constexpr int kNgramMaxOrder = 8;         // the back-off walk takes at most this many steps
constexpr int kNgramRowSteps = 14;        // ... and the search of a row at most this many (rows hold at most kBeamMaxV = 2^13 arcs)
// The n-gram LM as the kernel walks it (include/ctc_crf_hip.h crf_ngram_tables; device pointers): state 0 is the empty history with a
// dense row, every other state a sorted row of arcs, a back-off state and a back-off weight
struct NgramDev {
    const int *row_off, *arc_label, *arc_next, *bo_state, *uni_next;
    const float *arc_logp, *bo_weight, *uni_logp;
    int S, A, V, order, start;
};
// Kernel arguments of crf_ctc_beam_lm: the LM-free call's, the tables, the two weights and the LM part of the scores
struct BeamLmParams {
    BeamParams b;
    NgramDev lm;
    float alpha, beta;
    float *lm_score;            // [B nbest] or null
};
__global__ void crf_beamlm_search_kernel(BeamLmParams p);   // kBeamLmWaves waves (one workgroup) per utterance

// ---- k_beam_chunk.hip ----
// The record of one utterance's beam between two crf_ctc_beam_chunk calls (include/ctc_crf_hip.h): the slots' fields as arrays of W
// entries, one after the other -- pb, pnb, lm (fp64), id, pid (64-bit), alive, e, len, lms (int32): kBeamStateSlotBytes a slot -- then
// the W label rows of cap int32, then zero bytes up to a multiple of 16.
constexpr int kBeamStateSlotBytes = 5 * 8 + 4 * 4;
constexpr int kBeamStateMaxCap = 8192;    // labels kept per prefix at most (kNgramMaxStride, kEditStripMaxCols: what the consumers of the rows take)
__host__ __device__ constexpr int64_t beam_state_rows_off(int64_t W) { return kBeamStateSlotBytes * W; }
__host__ __device__ constexpr int64_t beam_state_bytes(int64_t W, int64_t cap) { return (beam_state_rows_off(W) + 4 * W * cap + 15) & ~(int64_t)15; }
// Kernel arguments of crf_ctc_beam_chunk: the searches' with T = the chunk's frames, lx = the chunk's lengths and hyps rows of cap words
struct BeamChunkParams {
    BeamLmParams q;             // (without an LM: q.b alone is read)
    const char *state_in;       // [B] records or null: every utterance starts fresh
    const int *reset;           // [B] or null: != 0 starts utterance b fresh
    char *state_out;            // [B] records
    int cap;
    int64_t rec;                // beam_state_bytes(W, cap)
};
__global__ void crf_beam_chunk_kernel(BeamChunkParams p);     // one wave (workgroup) per utterance
__global__ void crf_beamlm_chunk_kernel(BeamChunkParams p);   // kBeamLmWaves waves (one workgroup) per utterance

// ---- k_ngram.hip ----
constexpr int kNgramScoreWaves = 4;       // hypotheses (waves) per workgroup
constexpr int kNgramMaxStride = 8192;     // words between two rows, and the per-token outputs' row length
// Kernel arguments of crf_ngram_score: hypothesis h is the first hyp_len[h] entries of row h of hyps (rows `stride` entries apart)
struct NgramScoreParams {
    NgramDev lm;
    const float *eos;           // [S] log P(</s> | state), or null without add_eos
    const int *hyps, *hyp_len;
    int64_t H;
    int stride, use_start, add_eos;
    float *score;               // [H]
    int *invalid;               // [H] or null
    float *tok_logp;            // [H][stride] (TOK) or null
    int *tok_order;             // [H][stride] (TOK) or null; either of the two may be null alone
};
// TOK: the per-position outputs are written (at least one of them is asked for).  One wave per hypothesis, no LDS.
template <bool TOK> __global__ void crf_ngram_score_kernel(NgramScoreParams p);

// ---- k_rnnt.hip ----
constexpr int kRnntMaxU1 = 1024;          // lattice columns U + 1 at most: one thread per column, one workgroup per (utterance, direction)
constexpr int kRnntMaxV = 8192;
constexpr int kRnntWaves = 4;             // lattice nodes (waves) per workgroup of the row and gradient stages
constexpr int kRnntPF = 4;                // diagonals per staging batch of the lattice stage (two register sets in flight)
constexpr int kRnntPrepThreads = 256;
// Kernel arguments of crf_rnnt_loss / crf_rnnt_grad.  Row r of x (V elements) is lattice node (n, t, u): r = (n T + t) U1 + u in the padded
// layout, node_off[n] + t (U_n + 1) + u in the compact one; the workspace's per-node arrays are indexed by the same r.
struct RnntParams {
    const void *x;
    const int *labels, *lx, *ly;
    int N, T, U1, V, blank, compact;
    int64_t R;                  // rows of x: N T U1, or the compact rows
    int64_t nlab;               // entries of labels: N (U1 - 1), or the compact total
    float *row;                 // [R][4], 16-byte aligned: M = max_v x_v, ls = log sum_v exp(x_v - M), lb = (x[blank] - M) - ls, ll = (x[y_u] - M) - ls (-inf at u = U_n) of the live nodes
    double *alpha, *beta;       // [R] of the live nodes
    double *total;              // [N] log p(y | x), -inf for an invalid utterance or one without a finite path
    int *node_off;              // [N + 1] first row of utterance n
    int *lab_off, *tn, *un;     // [N] first label; T_n and U_n of a valid utterance, tn = 0 for an invalid one
    float *cost;                // [N]
    int *invalid;               // [N] or null
    const float *weight;        // [N] d loss / d cost[n] (crf_rnnt_grad)
    void *grad;                 // [R][V] in x's element type (crf_rnnt_grad)
};
__global__ void crf_rnnt_prep_kernel(RnntParams p);                                // one workgroup: offsets, validity
__global__ void crf_rnnt_gather_kernel(RnntParams p);                              // normalised input: a thread per node
template <typename E> __global__ void crf_rnnt_row_kernel(RnntParams p);           // raw input: a wave per node
template <bool WG> __global__ void crf_rnnt_lattice_kernel(RnntParams p);          // grid (N, 2); WG: U1 > 64, rup64(U1) threads
template <typename E, bool RAW> __global__ void crf_rnnt_grad_kernel(RnntParams p); // a wave per row of grad

// ---- k_rnnt_join.hip ----
constexpr int kJoinRowThreads = 256;      // row stage: a 16 x 16 grid of threads, 2 x 2 nodes each ...
constexpr int kJoinTT = 32;               // ... over kJoinTT frames x kJoinTU rows of one utterance,
constexpr int kJoinTU = 32;
constexpr int kJoinVC = 128;              // columns of the tile's f and g rows staged in LDS at a time (fp32: 2 x 32 x (128 + 4) x 4 bytes)
constexpr int kJoinGV = 256;              // grad stage: class columns (threads) per workgroup,
constexpr int kJoinGU = 32;               // lattice rows whose g and d g a thread holds in registers at a time,
constexpr int kJoinGL = 16;               // frames per chunk: the nodes' scalars of kJoinGL x kJoinGU nodes are formed once per workgroup,
constexpr int kJoinSplit = 4;             // partial sums of d g over the frames: split s takes the chunks s, s + kJoinSplit, ...
// Kernel arguments of crf_rnnt_simple_loss / crf_rnnt_simple_grad: the padded RnntParams (x unused, grad unused) and the joiner's two inputs.
struct JoinParams {
    RnntParams r;
    const void *f, *g;          // [N][T][V] and [N][U1][V] in one element type, raw
    float *df_part;             // [N][T][V] d f of the live rows (crf_rnnt_simple_grad)
    float *dg_part;             // [kJoinSplit][N][U1][V] partial d g of the live rows and splits
    void *grad_f, *grad_g;      // like f and g, either may be null
};
template <typename E> __global__ void crf_join_row_kernel(JoinParams q);          // grid (N ceil(T / kJoinTT), ceil(U1 / kJoinTU))
template <typename E> __global__ void crf_join_grad_kernel(JoinParams q);         // grid (N ceil(V / kJoinGV), kJoinSplit)
template <typename E> __global__ void crf_join_fold_kernel(JoinParams q);         // grid (N max(T, U1), 2): a workgroup per row of d f / d g

// ---- k_ctct.hip ----
constexpr int kCtctPF = 4;                // frames per staging batch of the lattice stage (two register sets in flight)
// Kernel arguments of crf_ctct_loss / crf_ctct_grad: the padded RnntParams (stage 0 is crf_rnnt_prep_kernel as it is) with the sections read
// as the CTC-T node record -- row [R][4] = (b, r, e, log s), alpha [R][2] and beta [R][2] fp64 -- and the rows' maxima beside them.
struct CtctParams {
    RnntParams r;
    float *rmax;                // [R] the row's maximum M (0 for normalised input)
};
__global__ void crf_ctct_gather_kernel(CtctParams q);                              // normalised input: a thread per node
template <typename E> __global__ void crf_ctct_row_kernel(CtctParams q);           // raw input: a wave per node
template <bool WG> __global__ void crf_ctct_lattice_kernel(CtctParams q);          // grid (N, 2); WG: U1 > 64, rup64(U1) threads
template <typename E, bool RAW> __global__ void crf_ctct_grad_kernel(CtctParams q); // a wave per row of grad

// ---- k_edit.hip ----
constexpr int kEditWaves = 4;            // hypotheses (waves) per workgroup of the register geometry
constexpr int kEditStripRows = 512;       // reference rows one wave holds (64 lanes x 8): longer references are walked in strips of this many
constexpr int kEditStripMaxCols = 8192;   // the strip path keeps one (cost, counts) pair per hypothesis column in LDS: 64 KiB at most
// Kernel arguments of crf_ctc_edit_distance: hypothesis h is the first hyp_len[h] entries of row h of hyps (rows `stride` entries apart),
// its reference refs[ref_off[u] .. + ref_len[u]) with u = hyp_utt[h]
struct EditParams {
    const int *hyps, *hyp_len, *hyp_utt;
    const int *refs, *ref_off, *ref_len;
    int B, H, stride, max_ref;
    int *dist;                  // [H]
    int *ops;                   // [H][3] (nsub, ndel, nins) or null
};
// NR reference rows per lane: 1, 2, 4, 8.  STRIP (NR = 8 only): one wave per workgroup, references of more than kEditStripRows rows in
// strips; dynamic LDS: stride x 8 bytes.
template <int NR, bool STRIP> __global__ void crf_ctc_edit_kernel(EditParams p);

// ---- k_res.hip ----
constexpr int kEpRegsR = 2;  // emission-row prefetch registers (V <= 2*512 for the resident kernels)
constexpr int kPoll = 4;      // granules polled concurrently per thread
constexpr int kResBatch = 6;   // measured: 5 -> 6 = -2% (fewer, longer straight-line blocks); 10 spills
static_assert(kResNCH % kResBatch == 0, "kResNCH must be a multiple of kResBatch");
// Kernel arguments of the resident kernels: only what ONE direction needs (the full LossParams is ~90
// SGPRs of pointers, most of which the compiler would keep live or spill around the unrolled frame body).
struct ResParams {
    ResDirDev L;
    int K, B, T, V, b0, rows_cu_max, Rout, Gf, Gb;
    const int *lx;
    const float *ep, *mx;
    float *Out;                 // Q (fwd) or BP (bwd) rows
    float *Row0;                // [B][Rout] spare rows: b_0 of the backward recursion
    int *Eout;                  // EQ (fwd) or EB (bwd)
    unsigned long long *xch;
    int *err;
    // forward side tables / results
    const float *x_start, *x_end;
    float *den_zs, *cost_alpha;
    int *den_ez;
    // backward side tables / results
    const int *z_lab;
    const float *z_end, *brow_start, *brow_end;
    const int2 *bcsr;
    float *cb_part;
    double *cb_mxs;
    int *cb_F;
    int *redo;                  // [2][B], see LossParams
};

// LDS map of the resident kernels: the two state-vector buffers sit at byte offsets 0 and kResXB; a gather
// is `ds_read_b32 v, (buffer base SGPR + 16-bit offset from the packed arc word)` -- one VALU (an SDWA add)
// per arc besides the FMA.
constexpr int kResXB = 65536;                 // bytes per state-vector buffer  -> gather vector <= 16384 entries (16-bit byte offsets);
                                              // 32 KiB until round 2: graphs of 8 k - 16 k states fell to the utterance-minor kernels (27 ms
                                              // instead of ~14 at S = 8193 / A = 208 k)
constexpr int kResGmax = kResXB / 4;
__global__ void crf_res_pair_kernel(ResParams pf, ResParams pb);

// ---- k_fac.hip ----
// chunks gathered per batch (template arguments of the instantiations the host launches and k_fac.hip instantiates)
#ifndef CRF_FAC4_NB
#define CRF_FAC4_NB 2       // chunks gathered per batch by the 1024-thread kernels (3: one weight pair spills INSIDE the frame loop, behind a vmcnt(0))
#endif
#ifndef CRF_FAC4_NB_ML
#define CRF_FAC4_NB_ML 2    // ... with multi-lane rows: the butterfly's registers make batches of 3 spill (V = 217: recursions 3.32 -> 3.02 ms)
#endif
#ifndef CRF_FAC5_NB2
#define CRF_FAC5_NB2 4      // ... by the two-utterance kernel on 512 threads x 30 chunks (256 registers per wave: 16 ds_read_b64 = 32 registers in flight)
#endif
#ifndef CRF_FAC3_NB2
#define CRF_FAC3_NB2 2      // chunks gathered per batch by the two-utterance kernels (8 ds_read_b64 = 16 registers in flight)
#endif
#define CRF_STR_(x) #x
#define CRF_STR(x) CRF_STR_(x)
#ifndef CRF_FAC3_NB_F
#define CRF_FAC3_NB_F 4
#endif
#ifndef CRF_FAC3_NB_B
#define CRF_FAC3_NB_B 4
#endif
struct FacParams {
    FacDirDev L;
    int B, T, V, Rout, NT, Rf;
    const int *lx;
    const float *ep, *mx;
    float *Out;                 // Q (fwd) or BP (bwd) rows
    float *Row0;                // [B][Rout] spare rows: b_0 of the backward recursion
    int *Eout;                  // EQ (fwd) or EB (bwd)
    int *started;               // workgroups of the den kernels that have started (gate for the numerator chains)
    int i0, i1;                 // iterations of this launch (segment)
    int nb;                     // stage bounds (iterations), bound[0] = 0 < ... < bound[nb-1] >= T; nb <= 1: no stage flags
    int bound[16];
    int *stage_cnt;             // [16] fine-grained counters: += 1 per utterance when the rows of all iterations < bound[k] are in memory
    float *state;               // [B][rup64(G) + 64] parked state vector and exponent between segments
    const int4 *frow_meta;
    const float *x_start, *x_end;
    float *den_zs, *cost_alpha;
    int *den_ez;
    const int4 *brow_meta;
    const int *z_lab;
    const float *z_end, *brow_start, *brow_end;
    const int *bx_idx; const float *bx_w; int nbx; float bx_se;   // rowless states of the backward recursion (FacDev)
    float *cb_part;
    double *cb_mxs;
    int *cb_F;
    int *redo;                  // [2][B], see LossParams
    // two CUs per recursion (FacDev::K = 2): the utterances [b0, b0 + nbu) of this launch, the exchange granules, the error word
    int K, b0, nbu, Gf, Gb;
    const int *xlist;           // forward: the L / A entries this CU fetches every frame (FacDev::xlist), [xl0, xl1)
    int xlist_off[3];
    unsigned long long *xch;
    int *err;
    // two utterances per workgroup (fac_chain_body2): pairs of this launch, rows that take the stores of an utterance that has ended
    int npair, dump_stride;
    float *dump;                // [2 directions][npair][dump_stride]
};
template <bool FLAG, int NTH, int NCH, int NBF, int NBB, bool ML, bool RL = false, bool ADT = false> __global__ void crf_fac_pair_kernel(FacParams pf, FacParams pb);
template <bool FLAG, int NTH, int NCH, int NBF, int NBB, bool ML, bool RL> __global__ void crf_fac_pair2_kernel(FacParams pf, FacParams pb);
template <int NTH, int NCH, int NBF, int NBB> __global__ void crf_fac2_pair_kernel(FacParams pf, FacParams pb);

// ---- k_grad.hip ----
#ifndef CRF_GD_FRAMES
#define CRF_GD_FRAMES 16
#endif
constexpr int kGDThreads = 256, kGDFrames = CRF_GD_FRAMES, kGDRowRegs = 5;   // rows of up to 5*256 float4 = 5120 floats
constexpr int kGDEpRegs = 4;                                      // V <= 4*256
constexpr int kGCThreads = 256, kGCFrames = 16, kGCRegs = 16, kGCVRegs = 4;  // 2L+1 <= 4096, V <= 1024
__global__ void crf_grad_kernel(LossParams p);
template <int NCPT, int EPR, int NT = kGDThreads, int CH = kChunk, int RR = kGDRowRegs, int WPE = 1> __global__ void crf_grad_den_kernel(LossParams p);
template <int REGS> __global__ void crf_grad_ctc_kernel(LossParams p);

// ---- k_batch.hip ----
struct BatchParams {
    BatchDev g;
    StreamDev st;                  // arc streams for AL = 64 / UL lane groups
    const float *start_lin, *end_lin;
    const float *x_start;          // [SX] a_0 of the forward vector's entries: the S states, then the U entries of factored streams
    int S, P, B, Bp, T, V, max_label, ngrp;
    int SX;                        // entries of the forward vector (S + StreamDev::NU)
    const int *lx;
    const float *ep, *moff;        // [B][T][V] e' (prep kernel), [B][T] log-likelihood offset per frame
    float *ept;                    // [T][grp][V][UL] e' transposed
    float *Af, *Zb;                // [2][grp][SX][UL], [2][grp][P][UL]
    float *Q, *BP;                 // [T][grp][P][UL]
    unsigned *mxf, *mxb;           // [3][Bp] maxima of the vectors (float bits; the values are non-negative)
    int *Ef, *Fb;                  // [Bp] running exponents
    float *zs, *zb;                // [Bp] scaled partition sums
    float *den_zs, *cost_alpha, *cost_beta;
    int *den_ez, *redo;
    float *grad;                   // [B][T][V]
    float c_den;
    int j;                         // launch number: forward frame j, backward frame T - j
    unsigned *bar;                 // crf_batch_persist_kernel: [512] words of the grid barrier, zeroed by crf_batch_init_kernel
    int *err;                      // ... its time-out word (crf_batch_cost_kernel turns the costs into NaN)
};
constexpr int kBatThreads = 256, kBatWaves = kBatThreads / kWave;
// (kStreamBatch, kStreamChunk, kStreamBundles, kStreamRecB: crf_internal.h, shared with the host's task cutter)
// Factored streams (NM = 3 descriptor words per row, crf_internal.h StreamDev): the ring holds NR values per row instead of the
// one emission row -- forward {e[label 0], e[label 1], U of the row's couple}, backward {e[label 0], e[label 1], z of the two
// extra arcs} -- all known from the descriptor, so all requested a bundle ahead like the emissions; epi gets them as e[NR].
constexpr int kStreamLds = 2 * kStreamRecB + 2 * 64 * 16 + kStreamBundles * 32 * 16;   // per wave: records (2 halves) | emission ring | descriptors
// (factored streams of small utterance groups -- many rows side by side -- have tasks of fewer bundles, so that a workgroup's
// four slices stay below half of the LDS: crf_internal.h stream_max_bundles, shared with the host's task cutter)
template <int UL, bool FAC>
constexpr int stream_lds() { return FAC ? 2 * kStreamRecB + 2 * 64 * 16 * 4 + stream_max_bundles(UL, true) * (256 / UL) * 48 : kStreamLds; }
template <int UL> __global__ void crf_batch_transpose_kernel(BatchParams p);
__global__ void crf_batch_init_kernel(BatchParams p);
template <int UL, int D, bool FAC = false> __global__ void crf_batch_frame_kernel(BatchParams p);
template <int UL, int D, bool FAC = false> __global__ void crf_batch_persist_kernel(BatchParams p);
template <int UL> __global__ void crf_batch_zsum_kernel(BatchParams p);
__global__ void crf_batch_cost_kernel(BatchParams p);
template <int UL> __global__ void crf_batch_grad_kernel(BatchParams p);

// ---- k_robust.hip ----
__global__ void crf_den_check_kernel(LossParams p, int parts);
template <bool GV> __global__ void crf_robust_den_kernel(LossParams p);
template <int NR> __global__ void crf_robust_ctc_kernel(LossParams p);
__global__ void crf_robust_ctc_fix_kernel(LossParams p);
__global__ void crf_finalize_kernel(LossParams p);
__global__ void crf_robust_grad_kernel(LossParams p);

}  // namespace crf
