/*
 * include/ctc_crf_hip.h -- C ABI of libctc_crf_hip.so, the MI355X-native (gfx950) CTC-CRF loss.
 *
 * This is the drop-in boundary for the reference's native layer L0:
 * plain pointers and sizes, no torch types.  It deliberately does NOT keep the reference's
 * denominator symbols (binding.cpp:20-49: Init / Release / compute_alpha / compute_beta_and_grad)
 * because those bake in the per-frame-launch design (separate alpha and beta entry points,
 * [32]-striped grad_storage).  Each entry point below names the reference interface it replaces.
 * The numerator's warp-ctc C API (gpu_ctc/ctc.h:76-109: compute_ctc_loss, get_workspace_size,
 * ctcGetStatusString) IS exported by this library as well, declared in include/ctc.h with the
 * warp-ctc semantics (host-resident labels, host costs, one stream sync per call); it sits on
 * crf_ctc_fwd_bwd below.
 *
 * Conventions
 *   - every pointer named *_dev is device memory on the graph's device; all work is enqueued on
 *     `stream` (a hipStream_t passed as void*); nothing here synchronises the host.
 *   - return value: 0 = CRF_OK, otherwise a crf_status; crf_last_error() gives the message
 *     (the reference printf()s and exit(1)s, den_calculate.cu:16-25, or drops the status,
 *     binding.cpp:111).
 *   - log_probs: [B][T][V] float32, contiguous (the reference's `logits`, ctc_crf/__init__.py:61);
 *     labels: flattened int32 without padding, blank = 0; lx/ly: int32 [B].  (crf_ctc_fwd_bwd, crf_ctc_align
 *     and their *_logits twins: also time-major [T][B][V] and any blank.)
 */
#ifndef CTC_CRF_HIP_H_
#define CTC_CRF_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    CRF_OK = 0,
    CRF_ERR_IO = 1,          /* cannot open / parse the FST file                      */
    CRF_ERR_FORMAT = 2,      /* not an OpenFst vector/standard binary, or epsilon ilabel */
    CRF_ERR_ARG = 3,         /* bad argument (null pointer, V <= max label, ...)      */
    CRF_ERR_HIP = 4,         /* a HIP runtime call failed                             */
    CRF_ERR_WORKSPACE = 5,   /* workspace too small                                   */
    CRF_ERR_UNSUPPORTED = 6  /* graph / label length exceeds what this build handles  */
} crf_status;

typedef struct crf_graph crf_graph; /* opaque: the denominator graph, resident on one GPU */

/* Replaces Init(fst_name, n_gpus, gpus) (den_calculate.cu:288-392) + ReadFst (fst_read.cc:11-62),
 * for ONE device: reads an OpenFst vector/standard binary without OpenFst, applies the same
 * conventions (label = ilabel-1, weight = -cost, end_weight = -Final), builds the device arc
 * tables and uploads them.  Unlike the reference there is no process-global state: any number of
 * graphs may coexist; one is created per (den_lm, device). */
int crf_graph_create(const char *fst_path, int device, crf_graph **out);

/* Same, from arc arrays already in reference conventions (lab = ilabel-1, w = -cost, log domain;
 * start_w/end_w = -inf for non-start / non-final states). */
int crf_graph_create_from_arcs(int64_t num_states, int64_t num_arcs, const int32_t *src,
                               const int32_t *dst, const int32_t *lab, const float *w,
                               const float *start_w, const float *end_w, int device,
                               crf_graph **out);

/* Replaces Release(n_gpus, gpus) (den_calculate.cu:394-425). */
void crf_graph_destroy(crf_graph *g);

/* Replaces the globals DEN_NUM_STATES / DEN_NUM_ARCS (binding.cpp:14-15).  `num_pairs` is the
 * number of distinct (destination state, label) pairs, the unit the kernels store per frame. */
int crf_graph_dims(const crf_graph *g, int64_t *num_states, int64_t *num_arcs, int64_t *num_pairs,
                   int64_t *max_label);

/* Diagnostics of the compiled tables: out[0..9] = states, arcs, pairs, padded pair rows, padded state
 * rows, forward ELL arcs incl. padding, backward ELL arcs incl. padding, forward / backward LDS
 * gathers that share a bank with an earlier lane of their half-wave (extra LDS cycles per frame),
 * max_in_degree*100000 + max_out_degree; out[10..15] = register-resident layout: CUs per recursion K
 * (0 = graph too large, streaming kernels are used), forward / backward arc slots incl. padding,
 * forward / backward extra LDS cycles (busiest bank per half-wave gather), forward_rows*100000 + backward_rows;
 * out[16..23] = factored layout (one CU per recursion, T o LM structure): available (0/1), matched state pairs,
 * weights re-gauged (0/1), single-gather (tail) rows, forward / backward arc slots, fused backward rows, Gf*100000 + Gb;
 * out[24] = geometry of the factored kernels: 0 = 768 threads, row constants in registers (at most 3 slices of rows per wave),
 * 1 = 768 threads, row constants in an LDS table, 2 = 512 threads, 3 = as 1 over TWO compute units per recursion, 4 = 1024
 * threads with the table (four waves per SIMD: the planner's first choice); -1 = no factored layout; out[25] = chunks of four
 * arcs per thread in that geometry (20; 21 = the 768-thread table geometry with all chunk slots holding arcs, taken by graphs
 * that do not fit 20; 15 with 1024 threads; 30 with 512 threads).
 * A graph created with device < 0 is compiled on the host
 * only (no GPU needed) and can be used with crf_graph_dims / crf_graph_stats / crf_graph_destroy. */
int crf_graph_stats(const crf_graph *g, int64_t *out, int n);

/* Replaces the torch::empty temporaries of gpu_den (binding.cpp:77-79): bytes of device scratch
 * crf_loss_fwd_bwd / crf_ctc_fwd_bwd need (include/ctc.h's get_workspace_size adds the host
 * metadata and outputs of compute_ctc_loss to this).  `g` may be NULL when c_den == 0 (plain CTC).
 * `max_label_len` >= max(ly). */
int64_t crf_workspace_bytes(const crf_graph *g, int64_t B, int64_t T, int64_t V, int64_t max_label_len);

/* Which denominator kernels a call of this shape takes (no reference counterpart: the reference has one set of kernels,
 * den_calculate.cu:63-261, for every graph): 0 streaming, 1 generic register-resident (K CUs per recursion),
 * 2 factored register-resident, 3 utterance-minor; < 0 on error.  Diagnostics / bench labels. */
int crf_den_kernels(const crf_graph *g, int64_t B, int64_t T, int64_t V);

/* Test aid (no reference counterpart): builds the arc streams of the utterance-minor kernels for UL utterances per group and
 * about `want` tasks per direction ON THE HOST and checks them against the graph's row tables (every row once, records = arcs,
 * flags, task limits); works on host-only graphs.  out4 = {tasks, rows outside the streams, steps, arc records}, both
 * directions summed.  UL < 0: the FACTORED streams for -UL utterances per group (T o LM graphs; all zero for other graphs):
 * records, flags, the three descriptor words of every row and the bundles-per-task limit against the factored rows. */
int crf_debug_stream_check(const crf_graph *g, int UL, int want, int64_t *out4);

/* Test aid: the block -> (utterance group, direction, chunk) mapping of the utterance-minor frame kernel for a grid of
 * 8 * nslot workgroups and `ncombo` combos: 0 when every (combo, chunk) is taken by exactly one workgroup. */
int crf_debug_decode_check(int nslot, int ncombo);
/* Host check of the factored rows of the utterance-minor kernels (T o LM graphs; no GPU): one step of both recursions through
 * them equals the step through the plain tables on random vectors.  out4: {U entries, forward records, backward records, arcs};
 * all zero when the graph has no such rows. */
int crf_debug_facbatch_check(const crf_graph *g, int64_t *out4);
/* Test aid (no GPU): emulates the data flow of the factored register-resident kernels on the layout tables of a (host-only)
 * graph for T frames of random emissions -- packed arc words, slice ends, multi-lane rows, row constants, entries, second copy,
 * rowless states, and with two compute units per recursion exactly what crosses between them (a gather of anything else yields
 * NaN).  out3 = {sum over end states by the graph's own row tables, factored forward, factored backward}: all three agree. */
int crf_debug_fac_emulate(const crf_graph *g, int T, unsigned seed, double *out3);
/* Test aid (no GPU): the stage plan of the staged grad pass for utterances of up to T frames and a batch of B, as crf_loss_fwd_bwd makes it
 * under the current debug switches (piece, taper, stages, segments, gd_stage_launches, gd_sub).  out (n_out >= 76 ints): [0] number of stages,
 * [1] length of the equal pieces, [2] 1 when the stages 2.. are ONE launch, [3] workgroups of that launch, then four arrays of 18 ints indexed by
 * the stage: its end (bound[0] = 0 ... bound[nstage] = T, in iterations of the recursions), its first workgroup in the one launch, frames per
 * workgroup, candidate blocks per run.  tests/test_stage_plan.py walks the grid the way crf_grad_den_kernel does: every frame block once. */
int crf_debug_stage_plan(int64_t T, int64_t B, int32_t *out, int n_out);
/* The same for the GENERIC register-resident layout over K compute units (any graph that fits: rows = pairs forward, state
 * copies backward, one produced entry per row, every product exchanged): out3 = {sum by the recursion over the graph's arcs,
 * layout forward, layout backward}; the grad pass's pair lists are checked frame by frame as well. */
int crf_debug_res_emulate(const crf_graph *g, int T, unsigned seed, double *out3);

/* Test aid (no GPU, no HIP call; works on host-only graphs and with g = NULL for numerator-only calls): the sections of the workspace
 * of crf_loss_fwd_bwd / crf_ctc_fwd_bwd and their *_logits twins for this shape under the current debug switches, in layout order, from
 * the very records the call carves its pointers from.  Writes (offset, bytes) pairs for as many sections as fit n_out int64 and returns
 * the number of sections; crf_debug_ws_section_names() gives their names, comma-separated, in the same order.  Every section starts on
 * a multiple of 256, the last one ends at or below crf_workspace_bytes(...); with the switch ws_gap = n every section is followed by
 * n x 256 bytes that belong to no section and that no kernel may touch (tests/guard.py checks them), unset the layout is the packed one.
 * crf_debug_align_ws_sections: the same for crf_ctc_align (logits = 0: the back-pointer words "bp") and crf_ctc_align_logits (logits = 1:
 * "bp", then the lse values "lse"); -1 with crf_last_error() set for a shape the build does not take. */
int crf_debug_ws_sections(const crf_graph *g, int64_t B, int64_t T, int64_t V, int64_t max_label_len, int64_t *out, int n_out);
const char *crf_debug_ws_section_names(void);
int crf_debug_align_ws_sections(int logits, int64_t B, int64_t T, int64_t V, int64_t max_label_len, int64_t *out, int n_out);
const char *crf_debug_align_ws_section_names(void);
/* The arrays INSIDE the sections "pb", "xch" and "bsm" of the loss call's workspace, from the very lists the call takes its pointers
 * from: (offset, bytes, element bytes) triples for as many fields as fit n_out int64, packed in list order; returns the number of
 * fields, crf_debug_ws_field_names(section) gives their names.  n is the batch size B ("bsm": B rounded up to the utterance group,
 * Bp).  Offsets count from the section's start -- for "xch" from the end of the exchange granules, i.e. the fields are the LAST bytes
 * of that section.  Fields named spare* belong to no kernel.  -1 / NULL with crf_last_error() set for any other section name.  (The
 * switch ws_gap acts between sections only.) */
int crf_debug_ws_fields(const char *section, int64_t n, int64_t *out, int n_out);
const char *crf_debug_ws_field_names(const char *section);

/* The hot path.  Replaces, in one call and with no host synchronisation:
 *   gpu_ctc  (binding.cpp:86-117  -> compute_ctc_loss, ctc_entrypoint.cu:29-60)
 *   gpu_den  (binding.cpp:65-84   -> compute_alpha + compute_beta_and_grad, den_calculate.cu:427-481)
 *   and the combine of _CTC_CRF.forward (ctc_crf/__init__.py:78-87).
 *
 *   grad_dev[b][t][v]  = c_den * gamma_den[b][t][v] - c_ctc * gamma_ctc[b][t][v]   (0 for t >= lx[b])
 *   loss_dev[0]        = sum_b ( c_den * logZ_den[b] - c_ctc * logp_ctc[b] )
 *   costs_den_dev[b]   = logZ_den[b]   (the reference's costs_alpha_den; may be NULL)
 *   costs_beta_dev[b]  = logZ_den[b] computed from the backward recursion (costs_beta_den; may be NULL)
 *   costs_ctc_dev[b]   = logp_ctc[b]   (+loglike, as the modified warp-ctc returns; may be NULL)
 *
 * CTC-CRF loss:  c_den = s, c_ctc = s*(1+lamb), s = 1/B if size_average else 1.
 * gpu_den alone: c_den = 1, c_ctc = 0.     gpu_ctc / WARP_CTC_LOSS: c_den = 0, c_ctc = s (g may be NULL).
 *
 * labels_dev: flattened labels; label_off_dev[b] = start of utterance b in it (int32 [B]).
 * Utterances the reference treats as invalid (L + repeats > T, gpu_ctc.h:166-174, where it returns
 * uninitialised memory) contribute logp_ctc = 0 and gamma_ctc = 0 and set invalid_dev[b] = 1
 * (invalid_dev may be NULL). */
int crf_loss_fwd_bwd(const crf_graph *g, const float *log_probs_dev, const int32_t *labels_dev,
                     const int32_t *label_off_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                     int64_t B, int64_t T, int64_t V, int64_t max_label_len, float c_den, float c_ctc,
                     float *grad_dev, float *loss_dev, float *costs_den_dev, float *costs_beta_dev,
                     float *costs_ctc_dev, int32_t *invalid_dev, void *workspace_dev,
                     int64_t workspace_bytes, void *stream);

/* Numerator only (plain CTC), with the two options of warp-ctc's ctcOptions / the reference's gpu_ctc (binding.cpp:86-117):
 *   time_major = 0: act_dev and grad_dev are [B][T][V] (as crf_loss_fwd_bwd);
 *   time_major = 1: they are [T][B][V], the layout gpu_ctc hands warp-ctc (ctc.h:49-62) -- no transposed copy is made;
 *   blank: the blank's column, in [0, V); labels must lie in [0, V) and differ from it (not checked here: labels are device memory).
 * Otherwise crf_loss_fwd_bwd with g = NULL, c_den = 0 and the same conventions (no host sync; workspace from
 * crf_workspace_bytes(NULL, B, T, V, max_label_len)):
 *   grad_dev[row (b, t)] = -c_ctc * gamma_ctc[b][t]  (0 for t >= lx[b]),  loss_dev[0] = -c_ctc * sum_b logp_ctc[b],
 *   costs_ctc_dev[b] = logp_ctc[b] (may be NULL), invalid_dev[b] (may be NULL). */
int crf_ctc_fwd_bwd(const float *act_dev, int time_major, int blank, const int32_t *labels_dev,
                    const int32_t *label_off_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                    int64_t B, int64_t T, int64_t V, int64_t max_label_len, float c_ctc,
                    float *grad_dev, float *loss_dev, float *costs_ctc_dev, int32_t *invalid_dev,
                    void *workspace_dev, int64_t workspace_bytes, void *stream);

/* crf_ctc_fwd_bwd on the RAW network output: the log_softmax in front of plain CTC and its backward fused in, as
 * crf_loss_fwd_bwd_logits does for the CTC-CRF loss, in either layout and with any blank.  Replaces, besides gpu_ctc,
 *   torch.log_softmax(x.float(), -1)  (cat/ctc/train.py:191-196, the non-CRF branch) and its backward.
 * act_dev: [B][T][V] or [T][B][V] (time_major) of dtype 0 = fp32, 1 = bf16, 2 = fp16, read element by element and upcast in registers
 * (rows of 16-bit elements need 2-byte alignment only, as for crf_ctc_align_logits); everything else as
 * crf_ctc_fwd_bwd (workspace from crf_workspace_bytes(NULL, ...), no host sync):
 *   costs_ctc_dev[b] = logp_ctc[b] under log_softmax of the upcast input,   loss_dev[0] = -c_ctc * sum_b costs_ctc_dev[b],
 *   grad_dev (fp32, the caller's layout): for a valid utterance and t < lx[b]
 *       grad[row (b, t)][v] = -c_ctc * (gamma_ctc[b][t][v] - softmax(x[b][t])[v]),
 *   exactly 0 for rows t >= lx[b] and for invalid utterances; invalid_dev as in crf_ctc_fwd_bwd.
 * CRF_ERR_ARG: dtype outside 0..2, c_ctc == 0. */
int crf_ctc_fwd_bwd_logits(const void *act_dev, int dtype, int time_major, int blank, const int32_t *labels_dev,
                           const int32_t *label_off_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                           int64_t B, int64_t T, int64_t V, int64_t max_label_len, float c_ctc,
                           float *grad_dev, float *loss_dev, float *costs_ctc_dev, int32_t *invalid_dev,
                           void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Forced alignment: the single best alignment of each transcript through the numerator's 2L+1 states (no reference counterpart:
 * the reference returns the sum over alignments only).  Conventions of crf_ctc_fwd_bwd: no host sync, all work on `stream`, act_dev
 * read in place as [B][T][V] (time_major = 0) or [T][B][V] (1), any blank in [0, V), labels_dev / label_off_dev / lx_dev / ly_dev as
 * there.  Log domain, fp32:  v_t[s] = act[b][t][lab(s)] + max(v_{t-1}[s], v_{t-1}[s-1], v_{t-1}[s-2] if s odd and lab(s) != lab(s-2)).
 * Ties go to the smallest move -- stay, then advance by one, then skip; at the end state 2L before 2L-1 -- so the result is
 * reproducible bit for bit.
 *   pos_dev[b][t]   always [B][T]: the index k in [0, ly[b]) of the transcript position emitted at frame t < lx[b], -1 for a blank
 *                   frame, -2 for t >= lx[b];
 *   score_dev[b]    the log-probability of that path (the fp32 sum of its entries in frame order);
 *   invalid_dev[b]  (may be NULL) 1 for an utterance with L + repeats > lx, lx <= 0 or a label outside [0, V): score -inf, row -2.
 * A valid utterance whose every alignment has probability 0: score -inf, row -2, invalid 0.  ly = 0 is valid (all frames -1).
 * Workspace: crf_ctc_align_workspace_bytes (2 bits per frame and state; its contents on entry do not matter); -1 with
 * crf_last_error() set for a shape this build does not take.  CRF_ERR_ARG: null pointer, blank outside [0, V), B * T > INT32_MAX;
 * CRF_ERR_UNSUPPORTED: V > 8192, max_label_len > 2047; CRF_ERR_WORKSPACE: workspace too small -- all answered before any HIP call. */
int64_t crf_ctc_align_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t max_label_len);
int crf_ctc_align(const float *act_dev, int time_major, int blank, const int32_t *labels_dev,
                  const int32_t *label_off_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                  int64_t B, int64_t T, int64_t V, int64_t max_label_len,
                  int32_t *pos_dev, float *score_dev, int32_t *invalid_dev,
                  void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Forced alignment on the RAW network output: act_dev is [B][T][V] or [T][B][V] of dtype 0 = fp32, 1 = bf16, 2 = fp16, read in place
 * (2-byte elements are upcast in registers; rows of 16-bit elements need 2-byte alignment only).  Everything else -- arguments, limits
 * (V <= 8192, max_label_len <= 2047, B * T <= INT32_MAX), pos_dev / invalid_dev, errors answered before any HIP call -- as crf_ctc_align,
 * plus CRF_ERR_ARG for a dtype outside 0..2.  Contract, with x^ the exact fp32 upcast of the input:
 *   - the path is the one crf_ctc_align's recursion finds on x^ ITSELF: fp32, sums in frame order, the same strict tie rule (stay, then
 *     advance, then skip; state 2L before 2L-1), no normalisation inside the recursion.  Every alignment of an utterance takes one
 *     entry from each of its lx frames, so log_softmax's normaliser sum_t lse_t is common to all of them: in exact arithmetic this is
 *     the best path under log_softmax(x^) as well;
 *   - score_dev[b] = float(double(raw best sum) - sum_{t < lx[b]} double(lse_t)),  lse_t = m_t + log sum_v exp(x^[t][v] - m_t),
 *     m_t = max_v x^[t][v], each lse_t computed in fp32 by a row kernel (16 lanes per frame for V <= 256, 64 otherwise: a lane adds
 *     its entries v = lane, lane + G, ... in order, the lanes' sums meet in a butterfly), the sum over t in fp64 in a fixed order
 *     (no atomics);
 *   - pos_dev and score_dev are reproducible bit for bit across calls and across the two layouts;
 *   - a dead utterance (raw best sum = -inf) or an invalid one returns exactly what crf_ctc_align returns; the lse sum is not used.
 * Workspace: crf_ctc_align_logits_workspace_bytes = crf_ctc_align_workspace_bytes + the lse values [B][T] (fp32; those of frames
 * t >= lx[b] are neither written nor read); -1 for a shape this build does not take. */
int64_t crf_ctc_align_logits_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t max_label_len);
int crf_ctc_align_logits(const void *act_dev, int dtype, int time_major, int blank, const int32_t *labels_dev,
                         const int32_t *label_off_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                         int64_t B, int64_t T, int64_t V, int64_t max_label_len,
                         int32_t *pos_dev, float *score_dev, int32_t *invalid_dev,
                         void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Forward-only CTC log-likelihoods of H hypotheses over B utterances (what cat/ctc/train_jsa.py:147-160 and decode_jsa_mls.py:189-191
 * get from nn.CTCLoss(reduction='none') under no_grad, the latter on repeat_interleave'd activations; N-best rescoring): hypothesis h is
 * the labels labels_dev[hyp_off_dev[h] .. + hyp_len_dev[h]) scored on the rows of utterance u = hyp_utt_dev[h].  The activations are read in
 * place, [B][T][V] (time_major = 0) or [T][B][V] (1), and never replicated; no backward chain, no gradient, no workspace, no host sync,
 * all work on `stream`.  Log domain, fp32, the largest term subtracted, one fixed operand order:
 *   v_t[s] = act[u][t][lab(s)] + log(exp(v_{t-1}[s]) + exp(v_{t-1}[s-1]) + [s odd and lab(s) != lab(s-2)] exp(v_{t-1}[s-2])),  t < lx[u],
 *   score_dev[h] = logaddexp(v[2L], v[2L-1])      (+log p, the sign of costs_ctc_dev)
 * so a hypothesis's score does not depend on its place in the list, on the other hypotheses or on the layout: the same bits across calls,
 * across a permutation of the list and across the two layouts, as long as max_hyp_len selects the same kernel (up to 2 max_hyp_len + 1 =
 * 512 states one wave per hypothesis with 1, 2, 4 or 8 states per lane, beyond one workgroup per hypothesis; crf_last_score_kernel()
 * names the instantiation of this thread's last call, e.g. "crf_ctc_score_wave_kernel<4>").  -inf entries flow through without NaN.
 *   hyp_utt_dev[h] in [0, B), in any order; an utterance may own no hypothesis.  Device memory, not checked here (an entry outside
 *                   [0, B) makes the hypothesis invalid, nothing is read for it);
 *   invalid_dev[h]  (may be NULL) 1 for a hypothesis with L + repeats > lx[u], lx[u] <= 0 or a label outside [0, V): score -inf -- the
 *                   alignment's rule.  A valid one whose every alignment has probability 0: score -inf, invalid 0.  L = 0 is valid:
 *                   the sum of the blank's column.
 * CRF_ERR_ARG: null pointer (invalid_dev excepted), blank outside [0, V), B, H, T or V <= 0, max_hyp_len < 0, B * T > INT32_MAX (H and V
 * are ints as well); CRF_ERR_UNSUPPORTED: max_hyp_len > 2047.  No limit on V.  All answered before any HIP call. */
int crf_ctc_score(const float *act_dev, int time_major, int blank, const int32_t *labels_dev, const int32_t *hyp_off_dev,
                  const int32_t *hyp_len_dev, const int32_t *hyp_utt_dev, const int32_t *lx_dev,
                  int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len,
                  float *score_dev, int32_t *invalid_dev, void *stream);
const char *crf_last_score_kernel(void);

/* crf_ctc_score on the RAW network output: act_dev of dtype 0 = fp32, 1 = bf16, 2 = fp16, read in place (2-byte elements are upcast in
 * registers; rows of 16-bit elements need 2-byte alignment only).  The contract of crf_ctc_align_logits, with x^ the exact upcast:
 * the recursion above runs on x^ itself, and
 *   score_dev[h] = float(double(raw) - sum_{t < lx[u]} double(lse_t)),   lse_t of row (u, t) by crf_ctc_align_logits's row kernel,
 * the sum in fp64 in a fixed order (no atomics); a raw score of -inf stays -inf.  Reproducible bit for bit as crf_ctc_score is.
 * Workspace: crf_ctc_score_logits_workspace_bytes (the lse values [B][T], fp32; >= 4 B T; its contents on entry do not matter; -1 for
 * B, T or V <= 0 or B * T > INT32_MAX).  Errors as crf_ctc_score, plus CRF_ERR_ARG for a dtype outside 0..2 or a null workspace and
 * CRF_ERR_WORKSPACE (the message names the bytes needed). */
int64_t crf_ctc_score_logits_workspace_bytes(int64_t B, int64_t T, int64_t V);
int crf_ctc_score_logits(const void *act_dev, int dtype, int time_major, int blank, const int32_t *labels_dev,
                         const int32_t *hyp_off_dev, const int32_t *hyp_len_dev, const int32_t *hyp_utt_dev, const int32_t *lx_dev,
                         int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len,
                         float *score_dev, int32_t *invalid_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* The weighted gradient of crf_ctc_score's scores, H hypotheses folded into ONE tensor of the activations' shape (minimum-risk / MWER
 * training on sampled or N-best hypotheses, the nn.CTCLoss(reduction='none', zero_infinity=True) / length losses with gradient of
 * cat/ctc/train_jsa.py:194-201, any per-hypothesis or per-utterance weighting -- without repeat_interleave'd activations and without an
 * [H][T][V] gradient):
 *   grad_dev[u][t][v] = sum over h with hyp_utt_dev[h] = u of  weight_dev[h] * gamma_h[t][v],
 *   gamma_h[t][v]     = d log p(h | act[u]) / d act[u][t][v] = sum over s with lab_h(s) = v of  exp(alpha_t[s] + beta_t[s] - score_dev[h]).
 * Inputs: the activations are fp32 log-probs, [B][T][V] (time_major = 0) or [T][B][V] (1), read in place and never replicated; grad_dev
 * has the layout of act_dev; the hypotheses as for crf_ctc_score; weight_dev [H] fp32, NULL = all 1.
 * Validity and scores: validity is crf_ctc_score's rule (the alignment's).  score_dev[h] and invalid_dev[h] (either may be NULL) are exactly
 * what crf_ctc_score writes for the same arguments, bit for bit: the forward recursion is the score kernels', with the same operand order
 * and the same instantiation chosen from max_hyp_len -- the call launches that very kernel first (crf_last_score_grad_kernel() names
 * the gradient's own alpha pass, e.g. "crf_ctc_score_grad_alpha_kernel<4>", with the same states per lane).  The occupancies come from a
 * second pair of recursions that carry their vectors in fp64 (fp32 log-domain vectors lose 1e-4 of a posterior within a few hundred
 * frames), and each frame's 2 L + 1 of them are normalised by their own sum -- in exact arithmetic exp(score_dev[h]), the score the
 * caller sees.
 * Gradient: the call writes EVERY entry of grad_dev; its contents on entry do not matter.  Rows of frames t >= lx[u] and of utterances
 * that own no hypothesis are 0.  A hypothesis that is invalid, scores -inf or has a weight of exactly 0 contributes nothing (the
 * zero_infinity=True rule of the caller this replaces).  For finite weights and activations that hold no NaN and no +inf there is no
 * NaN and no inf in grad_dev; -inf activations are allowed and give occupancy 0.  L = 0 is valid: occupancy 1 in the blank's column
 * for every frame t < lx[u].  The gradient is NOT promised bit for bit: as the numerator's grad pass does, the states of a frame are
 * scattered onto their labels with LDS float adds, whose order is not fixed (scores and invalid are bit for bit all the same).
 * Limits: max_hyp_len <= 255 (one wave per hypothesis, 2 L + 1 <= 512 states) and V <= 8192 (the reduce stage keeps a row in LDS), beyond
 * CRF_ERR_UNSUPPORTED, the message naming the limit.
 * Workspace: crf_ctc_score_grad_workspace_bytes (the stored alphas, [H][T][64 NR] fp64 with NR = 1, 2, 4, 8 the states per lane -- fp64 so
 * that they are exact whatever the cost per frame; the fp32 occupancies then go over the first half of each row -- and the H scores;
 * >= 8 H T (2 max_hyp_len + 1); offsets into it are 64-bit; its contents on entry do not matter;
 * -1 with crf_last_error() set for a shape not taken).
 * CRF_ERR_ARG: null pointer (weight_dev, score_dev and invalid_dev excepted), blank outside [0, V), B, H, T or V <= 0, max_hyp_len < 0,
 * B * T > INT32_MAX (H and V are ints as well); CRF_ERR_WORKSPACE: workspace too small (the message names the bytes needed) -- all
 * answered before any HIP call.  No host synchronisation, all work on `stream`, no environment variable read. */
int64_t crf_ctc_score_grad_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len);
int crf_ctc_score_grad(const float *act_dev, int time_major, int blank, const int32_t *labels_dev, const int32_t *hyp_off_dev,
                       const int32_t *hyp_len_dev, const int32_t *hyp_utt_dev, const int32_t *lx_dev, const float *weight_dev,
                       int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len,
                       float *score_dev, int32_t *invalid_dev, float *grad_dev,
                       void *workspace_dev, int64_t workspace_bytes, void *stream);
const char *crf_last_score_grad_kernel(void);

/* crf_ctc_score_grad on the RAW network output: act_dev of dtype 0 = fp32, 1 = bf16, 2 = fp16, read in place in either layout and never
 * copied or staged as fp32 (2-byte elements are upcast in registers; rows of 16-bit elements need 2-byte alignment only).  With x^ the
 * exact fp32 upcast and lse_t the normaliser of row (u, t) by crf_ctc_align_logits's row kernel:
 * Validity and scores: score_dev[h] and invalid_dev[h] (either may be NULL) are exactly what crf_ctc_score_logits writes for the same
 * arguments, bit for bit -- the call launches that row kernel and that very score kernel first.
 * Gradient: d (sum_h weight_dev[h] score_dev[h]) / d x^, log_softmax's backward included, fp32 in the layout of act_dev:
 *   grad_dev[u][t][v] = sum over the live h of u of  weight_dev[h] * gamma_h[t][v]  -  W_u * exp(x^[u][t][v] - lse_t),   t < lx[u],
 *   W_u = the sum of weight_dev[h] over the live h of u, accumulated in ascending h,
 * gamma_h the occupancies of log_softmax(x^) as above.  The recursions run on x^ itself, carried in fp64 as crf_ctc_score_grad's:
 * sum_t lse_t is common to all alignments of a hypothesis, and the exponent alpha + beta - s takes the raw sum-product
 * s = double(score) + sum_t double(lse_t), that sum in crf_ctc_score_logits's order.  A hypothesis is live as above: valid, score > -inf and a
 * weight other than 0.  The call writes EVERY entry of grad_dev; rows of frames t >= lx[u] and of utterances without a live hypothesis
 * are exactly 0, the softmax term included (a dead, invalid or zero-weight hypothesis adds nothing to W_u).  The activations hold no NaN
 * and no +inf; -inf entries are allowed as long as a row keeps one finite entry, and raw output of -inf on a label of a hypothesis
 * makes it score -inf, so it is not live.  The gradient is NOT promised bit for bit (LDS float adds, as above).
 * crf_last_score_grad_kernel() names the alpha pass with its element type, e.g. "crf_ctc_score_grad_alpha_raw_kernel<4, bf16>" (f32, bf16, f16).
 * Limits as crf_ctc_score_grad: max_hyp_len <= 255 and V <= 8192, beyond CRF_ERR_UNSUPPORTED with the same messages.
 * Workspace: crf_ctc_score_grad_logits_workspace_bytes = crf_ctc_score_grad_workspace_bytes' sections and behind them the lse values
 * [B][T], fp32; its contents on entry do not matter; -1 with crf_last_error() set where crf_ctc_score_grad_workspace_bytes returns -1.
 * CRF_ERR_ARG: a dtype outside 0..2 and what crf_ctc_score_grad answers so; CRF_ERR_WORKSPACE: workspace too small (the message names
 * the bytes needed) -- all answered before any HIP call.  No host synchronisation, all work on `stream`, no environment variable read. */
int64_t crf_ctc_score_grad_logits_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len);
int crf_ctc_score_grad_logits(const void *act_dev, int dtype, int time_major, int blank, const int32_t *labels_dev,
                              const int32_t *hyp_off_dev, const int32_t *hyp_len_dev, const int32_t *hyp_utt_dev, const int32_t *lx_dev,
                              const float *weight_dev, int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len,
                              float *score_dev, int32_t *invalid_dev, float *grad_dev,
                              void *workspace_dev, int64_t workspace_bytes, void *stream);

/* crf_ctc_score / crf_ctc_score_logits and their gradients on hypotheses that LIE ON THE DEVICE as padded rows -- exactly the rows
 * crf_ctc_sample and crf_ctc_beam write: hypothesis h is the first hyp_len_dev[h] words of row h of hyps_dev, rows hyp_stride words
 * apart; words behind the length are never read.  dtype -1: act_dev holds fp32 log-probs; 0 / 1 / 2: raw network output in fp32 / bf16 /
 * fp16 (the *_logits calls' arithmetic; the frames' lse values are computed once per call).
 * The host does not know the lengths, only a bound: len_cap is the caller's promise about the list and need not be its true maximum.  The
 * kernel is chosen on the device PER HYPOTHESIS, among the seven instantiations of crf_ctc_score (one wave per hypothesis for L <= 31, 63,
 * 127, 255; one workgroup for L <= 511, 1023, 2047): the call runs one pass per class whose lower end is at most len_cap, each on a masked
 * copy of the lengths, and merges the results.  score_dev[h] and invalid_dev[h] are therefore the bits crf_ctc_score / crf_ctc_score_logits
 * write for a list whose longest hypothesis lies in h's class; they depend on h's own labels and its utterance's rows only -- not on its
 * place in the list, on the other hypotheses, on len_cap (as long as it admits h) or on the layout.  crf_last_score_kernel() /
 * crf_last_score_grad_kernel() name the highest class launched (the gradient's: "crf_rows_grad_alpha_kernel<8>",
 * "crf_rows_grad_alpha_raw_kernel<8, bf16>").
 * Validity: what the host-list calls mark invalid stays invalid (L + repeats > lx[u], lx[u] <= 0, a label outside [0, V), hyp_utt outside
 * [0, B)); in addition L < 0, L > len_cap or L > hyp_stride gives score -inf and invalid 1 -- nothing is read for such a hypothesis and it
 * adds nothing to the gradient.  It is a result, not an error.
 * crf_ctc_score_grad_rows: crf_ctc_score_grad's contract unchanged (every entry of grad_dev is written, rows t >= lx[u] and utterances
 * without a live hypothesis are 0, not bit for bit); only the four wave classes take part, so len_cap <= 255 and V <= 8192.  The stored
 * alphas are [H][T][64 NR] fp64 with NR of len_cap's class: the workspace grows with the bound, not with the true lengths.
 * Workspace: the *_workspace_bytes functions (-1 with crf_last_error() set where the call would fail); its contents on entry do not
 * matter.  crf_debug_score_rows_ws_sections / _section_names (grad = 0 / 1) list its sections as crf_debug_align_ws_sections does: the
 * gradient's "occ", "hscore", then "hyp_off", "cls", "len", "cscore", "cinvalid" and, for raw output, "lse".
 * CRF_ERR_ARG: a null pointer (invalid_dev, weight_dev and, for the gradient, score_dev may be NULL); a dtype outside -1..2; B, H, T, V or
 * hyp_stride <= 0; len_cap < 0; H * hyp_stride or B * T > INT32_MAX; blank outside [0, V).  CRF_ERR_UNSUPPORTED: len_cap > 2047 (the
 * gradient: > 255, or V > 8192), the message names the limit.  CRF_ERR_WORKSPACE: the message names the bytes needed.  All answered
 * before any HIP call.  No host synchronisation, all work on `stream`, no environment variable read. */
int64_t crf_ctc_score_rows_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, int dtype);
int crf_ctc_score_rows(const void *act_dev, int dtype, int time_major, int blank, const int32_t *hyps_dev, int64_t hyp_stride,
                       const int32_t *hyp_len_dev, const int32_t *hyp_utt_dev, const int32_t *lx_dev, int64_t B, int64_t H, int64_t T,
                       int64_t V, int64_t len_cap, float *score_dev, int32_t *invalid_dev,
                       void *workspace_dev, int64_t workspace_bytes, void *stream);
int64_t crf_ctc_score_grad_rows_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, int dtype);
int crf_ctc_score_grad_rows(const void *act_dev, int dtype, int time_major, int blank, const int32_t *hyps_dev, int64_t hyp_stride,
                            const int32_t *hyp_len_dev, const int32_t *hyp_utt_dev, const int32_t *lx_dev, const float *weight_dev,
                            int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, float *score_dev, int32_t *invalid_dev,
                            float *grad_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int crf_debug_score_rows_ws_sections(int grad, int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, int dtype, int64_t *out, int n_out);
const char *crf_debug_score_rows_ws_section_names(int grad);

/* Label sequences drawn on the GPU (what cat/ctc/train_jsa.py:256-269 `_sample` gets from torch.multinomial over N T rows, a transpose and
 * the third-party ctc_align.align_; with greedy = 1 the best path: arg-max per frame): per frame K classes from softmax(x), then the CTC
 * map B on each of the B K frame paths.  The activations are read in place, [B][T][V] (time_major = 0) or [T][B][V] (1), dtype 0 = fp32,
 * 1 = bf16, 2 = fp16 (rows of 16-bit elements need 2-byte alignment only), x^ = the exact fp32 upcast of row (n, t), t < lx[n].
 *   Weights   w_v = exp(x^_v - max_v x^_v); the draws follow w / sum w = softmax(x^) -- for log-probs that is exp(x): ONE code path for
 *             log-probs and raw output, no fuse switch.  Rows must hold neither NaN nor +inf (their draws are unspecified; no access out
 *             of bounds whatever a row holds).  A row of -inf only emits the blank.
 *   Uniforms  (r0, r1, r2, r3) = Philox4x32-10(counter = (t, n, k >> 2, offset), key = (seed & 0xffffffff, seed >> 32));
 *             draw k uses u = (r[k & 3] >> 8) 2^-24 in [0, 1).  n: the utterance's index in the call, t: the frame.
 *   Selection the smallest v with C[v] > u C[V-1] (both fp32).  C is the kernel's fp32 inclusive running sum of w: chunks of G consecutive
 *             classes (G = 16 for V <= 256, else 64), a Hillis-Steele scan inside a chunk, the earlier chunks' sum added last -- and, as
 *             the partial sums of a parallel scan are not ordered among themselves, of those sums the running maximum over the classes
 *             of positive weight.  Exact consequences: a class with w_v = 0 (entry -inf, or exp underflows) is never drawn; some class
 *             with w_v > 0 always is (a search that runs off the end takes the last one).
 *   Greedy    (K = 1) the smallest v attaining the row maximum of x^ -- torch.argmax's rule, so class 0 for a row of -inf only.
 *   Collapse  frame t of path h = n K + k is kept iff c_t != blank and (t = 0 or c_t != c_{t-1});  hyps_dev[h][0 .. len) = the kept
 *             classes in frame order, hyp_len_dev[h] = len, hyps_dev[h][len .. T) = the BLANK's index (the padded rows go straight into
 *             an embedding).  lx[n] <= 0: length 0, a row of blanks; lx[n] > T counts as T.
 *   paths_dev (may be NULL) [B K][T]: the class drawn per frame, -1 for t >= lx[n].
 * Every entry of hyps_dev, hyp_len_dev and paths_dev is written by the call.  For fixed (seed, offset) the outputs of (n, k) are the same
 * bits in both layouts, for any B and any other utterances in the call, for any K > k and across calls; they may differ between dtypes and
 * between the two row kernels (crf_last_sample_kernel() names this thread's last one: "crf_sample_row_kernel<16>" for V <= 256,
 * "crf_sample_row_kernel<64>" beyond, "... , greedy>" for the arg-max).
 * Workspace: crf_ctc_sample_workspace_bytes (the classes per frame, [B K][T] int32; its contents on entry do not matter; -1 with
 * crf_last_error() set for a shape not taken).  No host synchronisation, all work on `stream`, no environment variable read.
 * CRF_ERR_ARG: null pointer (paths_dev excepted), dtype outside 0..2, blank outside [0, V), B, T, V or K <= 0, greedy with K != 1,
 * B * T or B * K > INT32_MAX; CRF_ERR_UNSUPPORTED: V > 8192 (the row's CDF is staged in LDS); CRF_ERR_WORKSPACE: workspace too small (the
 * message names the bytes needed) -- all answered before any HIP call. */
int64_t crf_ctc_sample_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t K);
int crf_ctc_sample(const void *act_dev, int dtype, int time_major, int blank, const int32_t *lx_dev,
                   int64_t B, int64_t T, int64_t V, int64_t K, uint64_t seed, uint32_t offset, int greedy,
                   int32_t *hyps_dev, int32_t *hyp_len_dev, int32_t *paths_dev,
                   void *workspace_dev, int64_t workspace_bytes, void *stream);
const char *crf_last_sample_kernel(void);

/* CTC prefix beam search on the GPU, LM-free (what cat/ctc/train.py:273-281, train_jsa.py:467-476 and decode.py:163-222 get from the
 * third-party CPU ctcdecode.CTCBeamDecoder after a host round trip of the whole activations): the N-best label sequences of every
 * utterance, as rows that go into crf_ctc_score / crf_ctc_score_grad unchanged.  The activations are read in place, [B][T][V]
 * (time_major = 0) or [T][B][V] (1), dtype 0 = fp32, 1 = bf16, 2 = fp16, x^ = the exact fp32 upcast; normalize = 0: x = x^ are taken as
 * log-probs, normalize = 1: x = x^ - lse_t (log_softmax; lse_t in fp32).  Any blank in [0, V); beam width W in [1, 64]; nbest in [1, W];
 * top_classes in [1, 64], of which the call uses C = min(top_classes, V - 1).
 *   Per frame t < lx[b]:  E_t = the C non-blank classes of largest x^, equal values to the lower index first, as a list in that order.
 *             The blank always takes part.  With C >= V - 1 nothing is pruned: the textbook search.  (A class at -inf never yields a
 *             candidate, in E_t or not.)
 *   Recursion The beam starts as the empty prefix, pb = 0, pnb = -inf.  For a beam prefix l with last label e (a (+) b = log(e^a + e^b)):
 *             stay       pb' = x[blank] + (pb (+) pnb);  pnb' = x[e] + pnb if e in E_t, else -inf (ctcdecode's rule: a repeat is pruned
 *                        with its class);
 *             extension  by c in E_t: pnb' = x[c] + (pb if c == e else pb (+) pnb), pb' = -inf.
 *             Prefix identity is by LABEL SEQUENCE: if l + c is itself in the beam, the extension's mass is added into that prefix's
 *             stay candidate (its pnb') and is no candidate of its own -- also when l left the beam and came back while l + c stayed
 *             (the kernel keeps a 64-bit hash-chain id per prefix and its parent's id: W x W compares per frame).
 *             A candidate's score is pb' (+) pnb'; candidates at -inf are dropped, the beam may hold fewer than W.  The W best survive
 *             under the total order: score descending, then stay before extension, then parent slot ascending, then -- among the
 *             extensions of one parent -- their place in E_t (equal x^: class ascending).  Slot k of the new beam is rank k.
 *             pb and pnb are carried in fp64 (fp32 exp / log of the differences inside (+)).
 *   hyps_dev  [B nbest][T]: row b nbest + r = the labels of rank r, then the BLANK's index up to T (crf_ctc_sample's rows).
 *   hyp_len_dev [B nbest];  score_dev [B nbest] fp32 = pb (+) pnb after frame lx - 1.  A missing rank has length 0 and score -inf.
 *             lx[b] <= 0: rank 0 is the empty prefix at score 0; lx[b] > T counts as T.
 *   trace_dev (may be NULL) [B][T][W] int32: after frame t, slot k: parent_slot + 64 (class + 1), class = -1 for a stay; -1 for an empty
 *             slot and for t >= lx[b].
 * Every entry of hyps_dev, hyp_len_dev, score_dev and trace_dev is written by the call.  The results are the same bits across calls, in
 * both layouts and whatever other utterances share the call.  Rows must hold neither NaN nor +inf (results unspecified; no access out of
 * bounds whatever a row holds).  crf_last_beam_kernel() names the row kernel of this thread's last call: "crf_beam_row_kernel<f32>",
 * "<bf16>", "<f16>".
 * Workspace: crf_ctc_beam_workspace_bytes (the frames' blank value and E_t as (value, class) pairs, [B T][C + 1] each, and the trace
 * words [B][T][W]; its contents on entry do not matter; -1 with crf_last_error() set for a shape not taken).  No host synchronisation,
 * all work on `stream`, no environment variable read.
 * CRF_ERR_ARG: null pointer (trace_dev excepted), dtype outside 0..2, normalize outside 0..1, blank outside [0, V), B, T or V <= 0, W or
 * top_classes outside [1, 64], nbest outside [1, W], B * T > INT32_MAX; CRF_ERR_UNSUPPORTED: V > 8192 (the row stage keeps the row in
 * LDS); CRF_ERR_WORKSPACE: workspace too small (the message names the bytes needed) -- all answered before any HIP call. */
int64_t crf_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t W, int64_t top_classes);
int crf_ctc_beam(const void *act_dev, int dtype, int time_major, int blank, int normalize, const int32_t *lx_dev,
                 int64_t B, int64_t T, int64_t V, int64_t W, int64_t nbest, int64_t top_classes,
                 int32_t *hyps_dev, int32_t *hyp_len_dev, float *score_dev, int32_t *trace_dev,
                 void *workspace_dev, int64_t workspace_bytes, void *stream);
const char *crf_last_beam_kernel(void);

/* crf_ctc_beam with shallow fusion of a token-level n-gram language model: what the reference's decoders get from
 * ctcdecode.CTCBeamDecoder(model_path=<KenLM n-gram>, alpha, beta, is_token_based=True) (cat/ctc/decode.py:163-222, the `kenlm:` blocks of
 * cat/ctc/train.py:258-281, train_jsa.py:452-476, train_me2e.py:308-331; the LM of cat/utils/pipeline/ngram.sh over token indices).  A
 * token of the LM is a class of the network output, so the LM's factor is a function of the prefix alone and prefixes that merge carry
 * the same factor.
 *   Tables    crf_ngram_tables: the back-off n-gram model compiled to states (cat_amd/ngram_lm.py builds them from an ARPA file).  State 0
 *             is the empty history (the root), every other state a history of 1 .. order - 1 tokens; states are sorted by history length,
 *             so bo_state[s] < s for s > 0.  Row s of the arcs is arc_*[row_off[s] .. row_off[s + 1]), arc_label ascending strictly; the
 *             root's row is DENSE instead (uni_logp[V], uni_next[V]; row_off[0] = row_off[1] = 0), so every back-off chain ends in one
 *             indexed load.  Values are natural logs in fp32, all finite.  `start` is the state the search begins in (that of <s>, or 0).
 *             The tables are the caller's device memory: the library allocates nothing and keeps no pointer behind the call.
 *   Lookup    lp(s, c), next(s, c): search c in row s; found at arc i: lp = acc + arc_logp[i], next = arc_next[i]; otherwise
 *             acc += bo_weight[s] and s = bo_state[s]; at the root lp = acc + uni_logp[c], next = uni_next[c] (acc starts at 0; fp32).
 *   Recursion The acoustic part is crf_ctc_beam's, unchanged: pb, pnb, the merge rule, E_t, the repeat pruned with its class.  Each
 *             prefix also carries its LM state and lm = alpha * log P_lm(prefix) + beta * length in fp64: an extension by c has the
 *             parent's lm + lmw with lmw = alpha * lp(state, c) + beta in fp32 (product and sum rounded separately), a stay keeps both.
 *             A candidate's score is (pb' (+) pnb') + lm.  The W best survive under the total order: score descending, then stay before
 *             extension, then parent slot ascending, then -- among the extensions of one parent -- x[c] + lmw descending (the fp64 sum
 *             of the two fp32 values), then their place in E_t.
 *   score_dev [B nbest] fp32 = (pb (+) pnb) + lm after frame lx - 1, the fused score; lm_score_dev (may be NULL) [B nbest] fp32 = lm (0
 *             for a missing rank).  hyps_dev, hyp_len_dev and trace_dev as for crf_ctc_beam.  No end-of-sentence term is added.
 * The results are the same bits across calls, in both layouts and whatever other utterances share the call.  With alpha == 0 and
 * beta == 0 every output equals crf_ctc_beam's bit for bit (where two extensions of one parent tie in score, crf_ctc_beam's rule and
 * this one agree whenever their x are equal).
 * Memory safety whatever the tables hold: the back-off walk takes at most min(order, 8) rows and then the root's, the search of a row
 * at most 14 probes (rows hold at most V <= 8192 arcs), every state and arc index is clamped into [0, S) and [0, A).  Tables that do not
 * pass crf_ngram_tables_check give unspecified results, never an access out of bounds and never a hang.
 * crf_ngram_tables_check runs on HOST copies of the tables (the struct's pointers are host pointers), with no HIP call: offsets start at
 * 0, are monotone and end at A, the root's sparse row is empty, labels ascend strictly inside a row and lie in [0, V), arc_next, uni_next
 * and start lie in [0, S), bo_state[s] < s (0 for the root), order lies in [1, 8], V in [1, 8192], every value is finite.  CRF_ERR_ARG with
 * a message that names the first offending entry.
 * crf_last_beam_kernel() names the row kernel as for crf_ctc_beam.  Workspace: crf_ctc_beam_lm_workspace_bytes (crf_ctc_beam's sections).
 * No host synchronisation, all work on `stream`, no environment variable read.
 * Errors: crf_ctc_beam's, and CRF_ERR_ARG for a null lm, lm->V != V, alpha or beta not finite, lm->S < 1, lm->order outside [1, 8],
 * lm->start outside [0, S) or a null table -- all answered before any HIP call.
 * Not covered: an end-of-sentence term in the search (it is in crf_ngram_score, not in the search), word-level LMs and lexicons, KenLM's
 * binary formats, an LM in crf_ctc_sample. */
typedef struct crf_ngram_tables {
    const int32_t *row_off;    /* [S + 1] */
    const int32_t *arc_label;  /* [A] */
    const float *arc_logp;     /* [A] */
    const int32_t *arc_next;   /* [A] */
    const int32_t *bo_state;   /* [S] */
    const float *bo_weight;    /* [S]; 0 where the model gives none */
    const float *uni_logp;     /* [V] the root's dense row */
    const int32_t *uni_next;   /* [V] */
    int64_t S, A, V;
    int32_t order, start;
} crf_ngram_tables;
int crf_ngram_tables_check(const crf_ngram_tables *host_tables);
int64_t crf_ctc_beam_lm_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t W, int64_t top_classes);
int crf_ctc_beam_lm(const void *act_dev, int dtype, int time_major, int blank, int normalize, const int32_t *lx_dev,
                    int64_t B, int64_t T, int64_t V, int64_t W, int64_t nbest, int64_t top_classes,
                    const crf_ngram_tables *lm, float alpha, float beta,
                    int32_t *hyps_dev, int32_t *hyp_len_dev, float *score_dev, float *lm_score_dev, int32_t *trace_dev,
                    void *workspace_dev, int64_t workspace_bytes, void *stream);

/* Streaming prefix beam search: crf_ctc_beam (lm == NULL) or crf_ctc_beam_lm (lm != NULL; alpha and beta are read only then) on a CHUNK
 * of Tc frames, with the beam carried from call to call in a state the caller keeps -- for encoders that run chunk by chunk
 * (cat/ctc/decode.py --streaming: model.chunk_infer, cat/ctc/train_unified.py, train_me2e_chunk.py).  Any split of an utterance's frames
 * into chunks gives the bits of the whole-utterance call: the recursion, E_t, the merge rule, the total order of the selection, the fp64
 * sums and the LM arithmetic are those calls', operation for operation.
 *   State     B self-contained records of crf_ctc_beam_state_record_bytes(W, cap) bytes (a multiple of 16), utterance-major: utterances
 *             may be permuted, selected or copied with plain byte copies.  A record holds, per slot k < W, what the searches keep in
 *             registers, as arrays of W entries one after the other: pb[W], pnb[W], lm[W] (fp64), id[W], parent id[W] (uint64),
 *             alive[W], last label[W], length[W], LM state[W] (int32) -- 56 W bytes -- then W label rows of cap int32 (row k: the first
 *             min(length, cap) labels of slot k's prefix, then the blank's index), then zero bytes up to the next multiple of 16:
 *             record_bytes = (56 W + 4 W cap + 15) & ~15.  The layout is the library's own and one for both searches: without an LM the
 *             lm entries and LM states are 0.  A state continues only under the W, cap, top_classes, blank, LM, alpha and beta it was made
 *             with (not checked here).  Both state pointers are 8-byte aligned.
 *   act_dev   the CHUNK's activations, [B][Tc][V] or [Tc][B][V], dtype and normalize as for crf_ctc_beam.  lx_chunk_dev[b]: how many of
 *             the chunk's frames belong to utterance b, clamped to [0, Tc]; with 0 the record passes through unchanged and the outputs
 *             repeat what the state holds.
 *   Fresh     Where state_in_dev == NULL or reset_dev != NULL and reset_dev[b] != 0, utterance b starts from the empty prefix exactly as
 *             the whole-utterance calls do and its input record is never read: a first call needs no initialised state, and a batch slot
 *             is reused for the next utterance by setting its reset word.
 *   state_out_dev  every byte of every record is written.  It must not overlap state_in_dev (label rows move between slots); the input
 *             state is never written, so a caller can branch from or rewind to an older state.
 *   Outputs   the whole calls' outputs as if the utterance ended after the frames seen so far: hyp_len_dev [B nbest] is the TRUE length,
 *             score_dev = pb (+) pnb (+ lm), lm_score_dev (may be NULL; written only with lm) as for crf_ctc_beam_lm.  hyps_dev
 *             [B nbest][cap]: rank r's first min(length, cap) labels, then the blank's index up to cap.  A prefix longer than cap keeps
 *             searching and scoring exactly as if cap were large, only its labels beyond cap are not kept: hyp_len > cap is how the
 *             caller sees it (the convention crf_ctc_score_rows / crf_ctc_edit_distance have for rows over their bound).  trace_dev (may
 *             be NULL) [B][Tc][W]: the chunk's trace rows, -1 for t >= lx_chunk.  Every output word is written.
 * Whatever a record holds, no access leaves the call's buffers (results are unspecified for records no call of this library wrote).
 * Workspace: crf_ctc_beam_chunk_workspace_bytes = crf_ctc_beam_workspace_bytes at T = Tc.  No host synchronisation, all work on `stream`,
 * no environment variable read.  crf_last_beam_kernel() names the row kernel as for crf_ctc_beam.
 * Errors: crf_ctc_beam's, with lm crf_ctc_beam_lm's, and CRF_ERR_ARG for a null state_out_dev, cap outside [1, 8192], overlapping or
 * misaligned states -- all answered before any HIP call.  crf_ctc_beam_state_record_bytes: -1 with crf_last_error() set for W outside
 * [1, 64] or cap outside [1, 8192].
 * Not covered: endpointing, an end-of-sentence term, emitting only the stable common prefix of the beam, W or top_classes above 64, a
 * state that survives a change of W or LM. */
int64_t crf_ctc_beam_state_record_bytes(int64_t W, int64_t cap);
int64_t crf_ctc_beam_chunk_workspace_bytes(int64_t B, int64_t Tc, int64_t V, int64_t W, int64_t top_classes);
int crf_ctc_beam_chunk(const void *act_dev, int dtype, int time_major, int blank, int normalize, const int32_t *lx_chunk_dev,
                       int64_t B, int64_t Tc, int64_t V, int64_t W, int64_t nbest, int64_t top_classes,
                       const crf_ngram_tables *lm, float alpha, float beta,
                       const void *state_in_dev, const int32_t *reset_dev, void *state_out_dev, int64_t cap,
                       int32_t *hyps_dev, int32_t *hyp_len_dev, float *score_dev, float *lm_score_dev, int32_t *trace_dev,
                       void *workspace_dev, int64_t workspace_bytes, void *stream);

/* n-gram LM scores of H hypotheses that lie on the device as padded rows: log P_lm of the second pass, what cat/lm/rescore.py:168-177
 * (final = score + alpha * log P_lm + beta * len per N-best entry) takes from cat/shared/decoder.py:542-572 (NGram.score: `.cpu()`, a
 * list of strings and one kenlm.Model.score call per sentence) and cat/utils/lm/lmweight_search.py repeats per (alpha, beta) -- for the
 * rows crf_ctc_sample / crf_ctc_beam / crf_ctc_beam_lm leave on the device, with any model and independent of the weights.
 *   Tables    crf_ngram_tables and the Lookup rule as above.  eos_logp_dev (may be NULL without add_eos) [S] fp32: log P(</s> | history
 *             of state s) in natural log, resolved when the model is compiled (cat_amd/ngram_lm.py eos_logp).
 *   Hypothesis h = the first hyp_len_dev[h] entries of row h of hyps_dev, rows hyp_stride entries apart; entries behind the length are
 *             never read.
 *   Position  token_logp_dev (may be NULL) [H][hyp_stride] fp32: for i < L bit for bit lp(state_i, t_i) of the Lookup rule (acc starts at
 *             0, the terms are added in fp32 in the walk's order, one rounded addition each; there is no multiply), state_i the state of
 *             the sequential walk from `start` (use_start != 0) or from the root (use_start == 0) -- the kernel resolves every position
 *             on its own from the last order - 1 tokens, which gives the same state.  token_order_dev (may be NULL) [H][hyp_stride]
 *             int32: the tokens of the n-gram found, context tokens used plus 1 (a <s> in the context counts; 1 at the root's row, also
 *             for a class that took <unk>'s value).  Both are 0 for L <= i < hyp_stride: every word of both is written.
 *             token_order reads the history length of a state off the order of the states: sorted by history length and, inside one
 *             length, in the order of the arcs that lead to them (as cat_amd/ngram_lm.py numbers them); with tables numbered otherwise
 *             it is some value in [1, order].
 *   Score     score_dev [H] fp32 = float(sum_{i<L} double(token_logp[h][i]) + (add_eos ? double(eos_logp[state_L]) : 0)), state_L the
 *             state behind the last token (`start`, or the root, for an empty row).  The fp64 sum runs in an order that depends on L
 *             alone: a row's outputs are the same bits in any batch, at any place of the list, in any call and whichever optional
 *             outputs are asked for.  An empty row scores 0, or eos_logp[start] (of the root with use_start == 0).
 *   Invalid   hyp_len[h] < 0 or > hyp_stride, or a token outside [0, V) among the first L: score = -inf, invalid_dev[h] (may be NULL) = 1
 *             (else 0), its per-token rows all 0; nothing is read outside the row's first min(max(L, 0), hyp_stride) words.
 * Memory safety whatever the tables hold, as for crf_ctc_beam_lm: at most min(order, 8) rows per look-up and then the root's, at most 14
 * probes per row, every state and arc index clamped.  Tables that do not pass crf_ngram_tables_check give unspecified values, never an
 * access out of bounds and never a hang.
 * crf_last_ngram_score_kernel() names the instantiation of this thread's last call: "crf_ngram_score_kernel<scores>" or
 * "crf_ngram_score_kernel<tokens>" (a per-token output asked for).  No workspace, no host synchronisation, all work on `stream`, no
 * environment variable read.
 * CRF_ERR_ARG: a null lm, a null table, null hyps_dev / hyp_len_dev / score_dev, lm->S < 1, lm->order outside [1, 8], lm->start outside
 * [0, S), lm->V outside [1, 8192], H < 0, hyp_stride outside [1, 8192], add_eos with a null eos_logp_dev -- all answered before any HIP
 * call.  H == 0 succeeds and launches nothing.
 * Not covered: word-level LMs and lexicons, KenLM's binary formats, neural LMs, V or hyp_stride beyond 8192. */
int crf_ngram_score(const crf_ngram_tables *lm, const float *eos_logp_dev, const int32_t *hyps_dev, int64_t hyp_stride,
                    const int32_t *hyp_len_dev, int64_t H, int use_start, int add_eos, float *score_dev, int32_t *invalid_dev,
                    float *token_logp_dev, int32_t *token_order_dev, void *stream);
const char *crf_last_ngram_score_kernel(void);

/* The RNN-T transducer loss and its gradient: what cat/rnnt/train.py:217 and train_unified.py:292-306 call as
 * warp_rnnt.rnnt_loss(joinout, y, lsub, ly, compact=...).  cost[n] = -log p(y_n | x_n), summed over all monotone alignments of the lattice
 * T_n x (U_n + 1): blank moves t -> t + 1, label y[u] moves u -> u + 1, the path ends with a blank at (T_n - 1, U_n).
 *
 * The joiner output is read in place as rows of V elements, one per lattice node:
 *   padded   (compact_rows < 0):  [N][T][U1][V], labels_dev [N][U1 - 1]                        (U1 = U + 1, compact_labels is ignored)
 *   compact  (compact_rows >= 0): [compact_rows][V], the utterances back to back, each T_n x (U_n + 1) row-major, and labels_dev
 *            [compact_labels] likewise; the offsets are prefix sums taken ON THE DEVICE from lx_dev / ly_dev (int32 [N], device), T and U1
 *            are then bounds on the lengths only.
 * crf_rnnt_loss / crf_rnnt_grad take normalised fp32 log-probabilities; the *_logits forms take the RAW joiner output, dtype 0 = fp32,
 * 1 = bf16, 2 = fp16 (upcast in registers), and are the loss of log_softmax(logits): no normalised copy is ever made.
 *
 * crf_rnnt_loss* is the forward: cost_dev [N], invalid_dev [N] (may be NULL) and the workspace, which keeps what the backward needs.
 * crf_rnnt_grad* takes THE SAME arguments and the same workspace, unchanged since the forward, and grad_output_dev [N], the derivative of
 * the caller's scalar with respect to cost[n] (any reduction and scale already folded in).  It writes EVERY element of grad_dev, which has
 * the shape and -- logits form -- the element type of the input:
 *   normalised:  grad[r][v] = grad_output[n] * d cost[n] / d log_probs[r][v]: zero except at the blank's column and at column
 *                labels[n][u] of a live node (t < T_n, u <= U_n);
 *   logits:      grad[r][v] = g_v - softmax(x[r])_v * (g_blank + g_label), g the two entries above: log_softmax's backward folded in.
 * Rows of padding nodes, of invalid utterances and of utterances without a finite path are written as zeros; there is no memset.
 *
 * Invalid input is decided on the device, without an error and without a host synchronisation: an utterance with T_n outside [1, T], U_n
 * outside [0, U1 - 1], a label outside [0, V) or equal to `blank`, or (compact) rows or labels that would reach past compact_rows /
 * compact_labels, gets cost +inf, invalid 1 and a zero gradient; in the compact layout an utterance whose LENGTHS are out of range claims no
 * rows.  A lattice without a finite path (entries of -inf) gets cost +inf and a zero gradient with invalid 0; no NaN is produced.
 *
 * Workspace, with R = N T U1 (padded) or compact_rows and al(x) = x rounded up to a multiple of 256:
 *   crf_rnnt_workspace_bytes = al(16 R) + al(8 R) + al(8 R) + al(8 N + 4 (4 N + 1))
 * -- per node four floats (the row's maximum M, log s = log sum_v exp(x_v - M), (x[blank] - M) - log s, (x[label] - M) - log s: the
 * normaliser in two steps, as log_softmax takes it, so that a common offset of the logits costs no digits) and alpha and beta in fp64
 * (eight floats; fp32 alpha / beta lose the gradient's fourth digit on long lattices), per utterance the total in fp64, two offsets and
 * the two checked lengths.  It must be 16-byte aligned.  -1 with the message set for sizes the call would refuse.
 *
 * Errors, all answered before any HIP call: a null pointer (CRF_ERR_ARG), dtype outside 0..2, N, T, U1 or V < 1, blank outside [0, V),
 * rows outside [1, INT32_MAX], T U1 (padded) or compact_rows > INT32_MAX / 4, a misaligned workspace (CRF_ERR_ARG), U1 > 1024 or V > 8192 (CRF_ERR_UNSUPPORTED),
 * a workspace that is too small (CRF_ERR_WORKSPACE).  One stream, no host synchronisation, no environment variable.
 * Not covered: warp_rnnt's gather mode as a separate entry (the kernels read two columns of a normalised row anyway), fastemit_lambda,
 * any RNN-T decoding.  rnnt_loss_simple is crf_rnnt_simple_loss below. */
int64_t crf_rnnt_workspace_bytes(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t compact_rows);
int crf_rnnt_loss(const float *log_probs_dev, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev, int64_t N,
                  int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, float *cost_dev, int32_t *invalid_dev,
                  void *workspace_dev, int64_t workspace_bytes, void *stream);
int crf_rnnt_loss_logits(const void *logits_dev, int dtype, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                         int64_t N, int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, float *cost_dev,
                         int32_t *invalid_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int crf_rnnt_grad(const float *log_probs_dev, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev, int64_t N,
                  int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, const float *grad_output_dev, float *grad_dev,
                  void *workspace_dev, int64_t workspace_bytes, void *stream);
int crf_rnnt_grad_logits(const void *logits_dev, int dtype, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                         int64_t N, int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels,
                         const float *grad_output_dev, void *grad_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
/* The workspace's sections as (offset, bytes) pairs -- "row", "alpha", "beta", "utt" -- for the guard-band tests; with the switch ws_gap
 * n x 256 untouched bytes follow every section.  Returns the number of sections, -1 for sizes the call would refuse. */
int crf_debug_rnnt_ws_sections(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t *out, int n_out);
const char *crf_debug_rnnt_ws_section_names(void);

/* The same loss for a joiner that is a plain sum (cat/rnnt/joiner.py:231-232 LogAdd; cat/rnnt/train.py:206-213 calls it as
 * warp_rnnt.rnnt_loss_simple(enc_out, pred_out, y, lsub, ly)):
 *   crf_rnnt_simple_loss(f, g, ...) == crf_rnnt_loss_logits(f[:, :, None, :] + g[:, None, :, :], ...)
 * from f_dev [N][T][V] and g_dev [N][U1][V] alone, both raw, contiguous and of one dtype (0 = fp32, 1 = bf16, 2 = fp16), read in place;
 * f + g is formed in fp32 from their exact values and the joint tensor [N][T][U1][V] is never formed.  Labels, lengths, validity, cost,
 * invalid (may be NULL) and the no-finite-path rule are those of crf_rnnt_loss in the padded layout.
 * crf_rnnt_simple_grad takes the same arguments and the forward's workspace, and grad_output_dev [N]; it writes EVERY element of
 * grad_f_dev [N][T][V] and grad_g_dev [N][U1][V] (the inputs' dtype; either pointer may be NULL, that gradient is then not formed):
 *   d f[t][v] = sum over u <= U_n, d g[u][v] = sum over t < T_n   of   gb [v = blank] + gl [v = y_u] - (gb + gl) softmax_v(f[t] + g[u])
 * with gb, gl the node's two occupancies times grad_output[n]; zeros for t >= T_n, u > U_n, invalid utterances and lattices without a
 * finite path.  No atomics: the same bits run to run and for an utterance alone or in any batch.
 * Workspace: crf_rnnt_simple_workspace_bytes = crf_rnnt_workspace_bytes(N, T, U1, V, -1) + al(4 N T V) + al(16 N U1 V): the sections
 * "row", "alpha", "beta", "utt" as above, then "df" (d f in fp32) and "dg" (four partial sums of d g over interleaved chunks of 16 frames,
 * added in a fixed order); nothing is proportional to T U1 V.  Errors and limits as for crf_rnnt_loss (U1 <= 1024, V <= 8192). */
int64_t crf_rnnt_simple_workspace_bytes(int64_t N, int64_t T, int64_t U1, int64_t V);
int crf_rnnt_simple_loss(const void *f_dev, const void *g_dev, int dtype, int blank, const int32_t *labels_dev, const int32_t *lx_dev,
                         const int32_t *ly_dev, int64_t N, int64_t T, int64_t U1, int64_t V, float *cost_dev, int32_t *invalid_dev,
                         void *workspace_dev, int64_t workspace_bytes, void *stream);
int crf_rnnt_simple_grad(const void *f_dev, const void *g_dev, int dtype, int blank, const int32_t *labels_dev, const int32_t *lx_dev,
                         const int32_t *ly_dev, int64_t N, int64_t T, int64_t U1, int64_t V, const float *grad_output_dev, void *grad_f_dev,
                         void *grad_g_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int crf_debug_rnnt_simple_ws_sections(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t *out, int n_out);
const char *crf_debug_rnnt_simple_ws_section_names(void);

/* The CTC-Transducer (CTC-T) loss and its gradient: what cat/rnnt/train.py:216-219 calls as warp_ctct.ctct_loss(xys, y, lsub, ly) with
 * topo="ctct".  A path labels EVERY frame t < T_n with one class; blanks and repeats collapse as in CTC and the collapse is y_n; frame
 * t's emission is read from row u = the number of labels the path has emitted before frame t.  cost[n] = -log of the sum over those paths.
 * With b(t,u) = lp[t][u][blank], r(t,u) = lp[t][u][y_u] (u >= 1) and e(t,u) = lp[t][u][y_{u+1}] (u < U), and per column the two masses
 * Ab / An after t frames with u labels emitted that end in a blank (or in nothing yet) / in y_u:
 *   Ab[0][0] = 0, everything else -inf
 *   Ab[t+1][u] = lse(Ab[t][u], An[t][u]) + b(t,u)
 *   An[t+1][u] = lse(An[t][u] + r(t,u), Ab[t][u-1] + e(t,u-1), An[t][u-1] + e(t,u-1) only if y_u != y_{u-1})
 *   total = lse(Ab[T][U], An[T][U]),  cost = -total
 * A lattice with T_n < U_n + #{u: y_u = y_{u+1}} has no path.  With lp independent of u this is plain CTC.
 *
 * The joiner output is read in place as [N][T][U1][V] (U1 = U + 1; the padded layout only: the caller's call has no compact argument),
 * labels_dev [N][U1 - 1], lx_dev / ly_dev int32 [N] on the device.  crf_ctct_loss / crf_ctct_grad take normalised fp32 log-probabilities;
 * the *_logits forms take the RAW joiner output, dtype 0 = fp32, 1 = bf16, 2 = fp16, and are the loss of log_softmax(logits).
 * crf_ctct_loss* is the forward: cost_dev [N], invalid_dev [N] (may be NULL) and the workspace.  crf_ctct_grad* takes THE SAME arguments and
 * the same workspace, unchanged since the forward, and grad_output_dev [N]; it writes EVERY element of grad_dev (the input's shape and --
 * logits form -- element type):
 *   normalised:  grad[r][v] = grad_output[n] (g_b [v = blank] + g_r [v = y_u] + g_e [v = y_{u+1}]), the three occupancies of a live node
 *                (y_u = y_{u+1}: one column, the terms add); sum over u of a frame's entries = -grad_output[n];
 *   logits:      grad[r][v] = g_v - softmax(x[r])_v * (g_b + g_r + g_e).
 * Rows of padding nodes, of invalid utterances and of utterances without a path are written as zeros; there is no memset.
 * Invalid input (T_n outside [1, T], U_n outside [0, U1 - 1], a label outside [0, V) or equal to `blank`) is decided on the device: cost
 * +inf, invalid 1, zero gradient.  A lattice without a finite path gets cost +inf and a zero gradient with invalid 0; no NaN is produced.
 *
 * Workspace, with R = N T U1 and al(x) = x rounded up to a multiple of 256:
 *   crf_ctct_workspace_bytes = al(16 R) + al(4 R) + al(16 R) + al(16 R) + al(8 N + 4 (4 N + 1))
 * -- per node the record (b, r, e, log s) and, apart, the row's maximum M (the normaliser in two steps, as for crf_rnnt_loss), forward
 * (X, An) and backward (Bb, Bn) in fp64, X = lse(Ab, An) where y_{u+1} may follow y_u directly and Ab where not; per utterance as for
 * crf_rnnt_loss.  It must be 16-byte aligned.  -1 with the message set for sizes the call would refuse.
 * Errors, all answered before any HIP call, and limits (U1 <= 1024, V <= 8192, T U1 <= INT32_MAX / 4) as for crf_rnnt_loss.
 * Not covered: the compact layout, a form on f and g without the joint tensor (warp_ctct.ctct_simple_loss), any CTC-T or RNN-T decoding. */
int64_t crf_ctct_workspace_bytes(int64_t N, int64_t T, int64_t U1, int64_t V);
int crf_ctct_loss(const float *log_probs_dev, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev, int64_t N,
                  int64_t T, int64_t U1, int64_t V, float *cost_dev, int32_t *invalid_dev, void *workspace_dev, int64_t workspace_bytes,
                  void *stream);
int crf_ctct_loss_logits(const void *logits_dev, int dtype, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                         int64_t N, int64_t T, int64_t U1, int64_t V, float *cost_dev, int32_t *invalid_dev, void *workspace_dev,
                         int64_t workspace_bytes, void *stream);
int crf_ctct_grad(const float *log_probs_dev, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev, int64_t N,
                  int64_t T, int64_t U1, int64_t V, const float *grad_output_dev, float *grad_dev, void *workspace_dev, int64_t workspace_bytes,
                  void *stream);
int crf_ctct_grad_logits(const void *logits_dev, int dtype, int blank, const int32_t *labels_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                         int64_t N, int64_t T, int64_t U1, int64_t V, const float *grad_output_dev, void *grad_dev, void *workspace_dev,
                         int64_t workspace_bytes, void *stream);
/* The workspace's sections -- "row", "rmax", "alpha", "beta", "utt" -- as crf_debug_rnnt_ws_sections gives them. */
int crf_debug_ctct_ws_sections(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t *out, int n_out);
const char *crf_debug_ctct_ws_section_names(void);

/* Token edit distance of H hypotheses to the transcripts of their utterances, with the operation counts of one optimal alignment: what
 * cat/ctc/train.py:200-210 (cal_wer), train_jsa.py:371-387 (cal_per), train_me2e.py:250-256 and train_me2e_kaldi.py:420-426 compute with
 * a Python loop of Levenshtein.distance after `.cpu().tolist()`, and the risk of minimum-risk / MWER training, for the rows that
 * crf_ctc_sample / crf_ctc_beam leave on the device.  Tokens are compared as int32: no vocabulary, no blank, no activations.
 *   Hypothesis h = the first hyp_len_dev[h] entries of row h of hyps_dev, rows hyp_stride entries apart (the padded rows of
 *             crf_ctc_sample / crf_ctc_beam); entries behind hyp_len are never read.
 *   Reference of utterance u = hyp_utt_dev[h]: refs_dev[ref_off_dev[u] .. + ref_len_dev[u]) (the flattened labels of the loss calls).
 *   Distance  With r the reference (length R) and y the hypothesis (length Y): D[0][j] = j, D[i][0] = i, and for i, j >= 1 the cell
 *             takes the smallest of  diag = D[i-1][j-1] + (r_i != y_j),  del = D[i-1][j] + 1,  ins = D[i][j-1] + 1.
 *             dist_dev[h] = D[R][Y].
 *   Counts    ops_dev (may be NULL) [H][3] int32 = (nsub, ndel, nins).  Every cell carries the three counts; the border cells carry
 *             (0, i, 0) and (0, 0, j); among candidates of equal cost the cell takes the FIRST in the order diag, del, ins (strict
 *             compares in that order), inherits that predecessor's counts and adds one to the matching count (nothing for a match).
 *             Hence nsub + ndel + nins = dist, hits = R - nsub - ndel, Y = hits + nsub + nins.
 *   Invalid   hyp_utt[h] outside [0, B), hyp_len[h] < 0 or > hyp_stride, or ref_len[u] outside [0, max_ref_len]: dist = -1 and
 *             ops = (-1, -1, -1); neither its row nor its reference is read.
 * Every entry of dist_dev and ops_dev is written by the call, by a plain store (no atomics).  Integers only: a hypothesis's result
 * depends on the two token sequences alone -- the same bits across calls, wherever it stands in the list, whatever shares the call and
 * whichever instantiation max_ref_len selects.  crf_last_edit_kernel() names that of this thread's last call:
 * "crf_ctc_edit_kernel<1>", "<2>", "<4>", "<8>" (max_ref_len <= 64, 128, 256, 512: one wave per hypothesis, the reference rows in
 * registers) or "crf_ctc_edit_kernel<8, strips>" (longer references in strips of 512 rows, 8 hyp_stride bytes of LDS).
 * max_ref_len is a host bound of ref_len_dev; the bound of the hypotheses is hyp_stride.  No workspace, no host synchronisation, all
 * work on `stream`, no environment variable read.
 * CRF_ERR_ARG: null pointer (ops_dev excepted), B, H or hyp_stride <= 0, max_ref_len < 0, H * hyp_stride > INT32_MAX;
 * CRF_ERR_UNSUPPORTED: max_ref_len > 2047, or max_ref_len > 512 together with hyp_stride > 8192 (the strips keep a cell per column in
 * LDS) -- all answered before any HIP call. */
int crf_ctc_edit_distance(const int32_t *hyps_dev, int64_t hyp_stride, const int32_t *hyp_len_dev, const int32_t *hyp_utt_dev,
                          const int32_t *refs_dev, const int32_t *ref_off_dev, const int32_t *ref_len_dev,
                          int64_t B, int64_t H, int64_t max_ref_len, int32_t *dist_dev, int32_t *ops_dev, void *stream);
const char *crf_last_edit_kernel(void);

/* Replaces the cudaMemcpyAsync calls that bring labels, label lengths and input lengths to the device
 * (gpu_ctc.h:143-229; `input_lengths.cuda()`, ctc_crf/__init__.py:73): copies n int32 from PINNED host
 * memory (hipHostMalloc / torch pin_memory: device-accessible) to device memory with a kernel on `stream` --
 * no DMA engine start-up between two calls.  The host buffer must stay untouched until the stream has passed. */
int crf_stage_i32(int32_t *dst_dev, const int32_t *src_pinned_host, int64_t n, void *stream);

/* crf_loss_fwd_bwd with the log_softmax in front of it fused in.  Replaces, in addition,
 *   logits = torch.log_softmax(netout, dim=-1)   and   criterion(logits.float(), ...)   (cat/ctc/train.py:174-186)
 * and log_softmax's backward: `logits_dev` are the RAW network outputs [B][T][V], dtype 0 = fp32, 1 = bf16, 2 = fp16
 * (upcast in registers; the recursions, costs and the gradient stay fp32/fp64), and
 *   grad_dev[b][t][v] = d loss / d logits[b][t][v]
 *                     = (c_den gamma_den - c_ctc gamma_ctc) - softmax(logits)[v] * sum_v (c_den gamma_den - c_ctc gamma_ctc)
 * in fp32.  Everything else as crf_loss_fwd_bwd; c_ctc must not be 0 (the softmax term rides on the numerator half of
 * the grad pass).  Costs are those of log_softmax(logits). */
int crf_loss_fwd_bwd_logits(const crf_graph *g, const void *logits_dev, int dtype, const int32_t *labels_dev,
                            const int32_t *label_off_dev, const int32_t *lx_dev, const int32_t *ly_dev,
                            int64_t B, int64_t T, int64_t V, int64_t max_label_len, float c_den, float c_ctc,
                            float *grad_dev, float *loss_dev, float *costs_den_dev, float *costs_beta_dev,
                            float *costs_ctc_dev, int32_t *invalid_dev, void *workspace_dev,
                            int64_t workspace_bytes, void *stream);

/* Diagnostics (no reference counterpart; the reference has no profiler hooks).
 * crf_profile_enable(1): every following crf_loss_fwd_bwd on this thread brackets each of its
 * kernel launches with HIP events on the stream the kernel is launched on.
 * crf_profile_read synchronises on those events and returns, for the LAST call, up to `n`
 * durations in milliseconds in the fixed order
 *   [0] prep  [1] den forward chain  [2] den backward chain  [3] ctc forward chain
 *   [4] ctc backward chain  [5] grad  [6] finalize  [7] whole call (first launch .. last launch)
 * (-1 for kernels that were not launched).  Returns the number of slots written. */
void crf_profile_enable(int on);
/* The template instantiation of the kernel that ran the denominator recursions in this thread's last call, e.g.
 * "crf_fac_pair_kernel<true,768,21,4,4,false,false>" (the prefix of the name rocprofv3 reports): bench.py keys its committed PMC
 * traffic numbers by workload AND by this string. */
const char *crf_last_den_kernel(void);
/* Streams this thread's last call put work on: 1 = the caller's only, 2 = + the context's side stream, 3 = + its third stream
 * (the numerator's log-domain fallback chains beside the staged grad pass: taken when a recent call of the context needed them). */
int crf_last_call_streams(void);
/* What the side stream of the (device, caller stream) context of this thread's last call is: "plain (candidate 2)", "priority-low
 * (candidate 9)", "cu-mask (candidate 13) + third stream", "none (candidate 13)" -- the kind of stream that was found to run
 * beside the caller's and how many candidates had been probed by then (crf_host.hip find_beside).  The reference runs everything
 * on the caller's stream (binding.cpp:75,102) and has nothing to report. */
const char *crf_last_side_stream(void);
/* How many utterances of this thread's last call were redone by a fallback: out2[0] = denominator (crf_robust_den_kernel: the scaled fp32
 * recursions lost the utterance's mass, or -- lagged scale -- a frame shrank the vector by more than 2^90), out2[1] = numerator
 * (crf_robust_ctc_kernel: frames outside the fp64 range of the rescaled chains).  Synchronises `stream` (the stream of that call) and
 * copies two words: a diagnostic for benchmarks and tests, not for the training loop.  LIFETIME: the words live in that call's workspace
 * (or, with fine-grained flag words, in the buffer of its (device, stream) context): ask right after the call, before the workspace is
 * freed or handed to another call and before another thread calls on the same device and stream -- later the counts are another call's
 * or the pointer dangles.  The reference has no fallback: its log-domain kernels (den_calculate.cu:29-35) pay exp + log1p on every arc
 * instead. */
int crf_last_fallback_counts(int32_t *out2, void *stream);
/* What can differ between two builds of this library: the geometry dials of the kernel instantiations as "NAME=value" pairs separated by
 * blanks, e.g. "FAC4_NB=2 FAC4_NB_ML=2 ... GD_FRAMES=16" (NAME: the macro CRF_NAME of cat_amd/csrc, overridden with
 * CRF_BUILD_DEFS=-DCRF_NAME=n), and "TIMING=1" in a timing build (-DCRF_TIMING). */
const char *crf_build_switches(void);
int crf_profile_read(float *ms_out, int n);

/* Diagnostics, timing builds only (CRF_BUILD_DEFS=-DCRF_TIMING python -m cat_amd.build --force): copies
 * the in-kernel phase stamps (shader cycles, s_memtime) of the last call into `out`; returns the number of
 * values, 0 in a product build.  tools/timing_probe.py decodes them.  No reference counterpart. */
int crf_timing_read(unsigned long long *out, int n);

/* Debug / experiment switches of tests and tools (no reference counterpart).  The library NEVER reads the process
 * environment: every switch is set here, by name, process-wide; crf_debug_unset returns it to its default.  Switches marked
 * G are read when a graph is created, C per loss call, X when a (device, stream) context is first used;
 * crf_debug_list() returns one "name: when  what" line per switch.  CRF_ERR_ARG for an unknown name. */
int crf_debug_set(const char *key, int value);
int crf_debug_unset(const char *key);
const char *crf_debug_list(void);

/* Message for the last non-zero status returned on this thread. */
const char *crf_last_error(void);

/* Library version string, e.g. "ctc_crf_hip 0.1.0 (gfx950)". */
const char *crf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CTC_CRF_HIP_H_ */
