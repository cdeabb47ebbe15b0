// cat_amd/csrc/crf_host_ctc.hip -- the host side of the surfaces on the plain CTC lattice, which share nothing with the loss call
// (crf_host.hip) but crf_host_util.h: forced alignment (crf_ctc_align*, k_align.hip), hypothesis scores (crf_ctc_score*, k_score.hip), their
// weighted gradient (crf_ctc_score_grad*, k_score_grad.hip), both on hypotheses that lie on the device as padded rows (crf_ctc_score_rows,
// crf_ctc_score_grad_rows, k_rows.hip), sampled / best-path label sequences (crf_ctc_sample, k_sample.hip), the
// prefix beam search (crf_ctc_beam, k_beam.hip; with an n-gram LM: crf_ctc_beam_lm, k_beam_lm.hip, crf_ngram_tables_check) and -- on token sequences alone, no lattice -- the edit distance of hypotheses to
// their transcripts (crf_ctc_edit_distance, k_edit.hip) and their n-gram LM scores (crf_ngram_score, k_ngram.hip) -- and the RNN-T
// transducer loss on the joiner's lattice (crf_rnnt_loss, crf_rnnt_grad, k_rnnt.hip) and the CTC-Transducer loss on the same lattice
// (crf_ctct_loss, crf_ctct_grad, k_ctct.hip) --
// argument checks, workspace sections, kernel choice, the C-ABI entry points of include/ctc_crf_hip.h.  Every error is answered before
// any HIP call.  The activations are read in place in either layout and -- the *_logits entry points and crf_ctc_sample -- in f32, bf16
// or f16.
#include <cmath>
#include <type_traits>

#include "crf_device.h"
#include "crf_kernels_decl.h"
#include "crf_host_util.h"

namespace crf {

static thread_local const char *g_sample_kernel = ""; // template instantiation of the row kernel of this thread's last crf_ctc_sample (crf_last_sample_kernel)
static thread_local const char *g_beam_kernel = "";   // ... of the row kernel of this thread's last crf_ctc_beam (crf_last_beam_kernel)
static thread_local const char *g_edit_kernel = "";   // ... of the kernel of this thread's last crf_ctc_edit_distance (crf_last_edit_kernel)
static thread_local const char *g_ngram_kernel = "";  // ... of the kernel of this thread's last crf_ngram_score (crf_last_ngram_score_kernel)
static thread_local const char *g_score_kernel = "";// ... of the kernel of this thread's last crf_ctc_score / crf_ctc_score_logits (crf_last_score_kernel)
static thread_local const char *g_score_grad_kernel = "";   // ... of the alpha pass of this thread's last crf_ctc_score_grad / crf_ctc_score_grad_logits (crf_last_score_grad_kernel)

// ---- what the three surfaces share ----
// f(E{}) with the element type of dtype 0 (f32), 1 (bf16), 2 (f16)
template <typename F>
static int with_dtype(int dtype, F &&f) {
    return dtype == 0 ? f(float{}) : dtype == 1 ? f(AlnBf16{}) : f(AlnF16{});
}
// the activations of a params block: row (b, t) at b * xs_b + t * xs_t elements, read in place in either layout
template <typename P>
static void set_act(P &p, const void *act, const int32_t *lx, int64_t B, int64_t T, int64_t V, int blank, int time_major) {
    p.x = act; p.lx = lx;
    p.B = (int)B; p.T = (int)T; p.V = (int)V; p.blank = blank;
    p.xs_b = time_major ? V : T * V; p.xs_t = time_major ? B * V : V;
}
// the argument checks with one text: CRF_OK, or the error with the message set
static int bad_dtype(const char *who) { set_error(std::string(who) + ": dtype must be 0 (f32), 1 (bf16) or 2 (f16)"); return CRF_ERR_ARG; }
static int check_blank(int blank, int64_t V) {
    if (blank < 0 || blank >= V) { set_error("blank " + std::to_string(blank) + " outside [0, V=" + std::to_string(V) + ")"); return CRF_ERR_ARG; }
    return CRF_OK;
}
static int check_ws(int64_t ws_bytes, int64_t need) {
    if (ws_bytes < need) { set_error("workspace too small: need " + std::to_string(need)); return CRF_ERR_WORKSPACE; }
    return CRF_OK;
}
// their workspaces: one to eight sections, laid down as the loss call's are (crf_host_util.h)
struct SideWs {
    WsSection sec[8];
    int nsec = 0;
    int64_t total = 0, gap = ws_gap_bytes();
    SideWs &add(const char *name, int64_t bytes) { sec[nsec++] = WsSection{name, total, bytes}; total = al(total + bytes) + gap; return *this; }
};
// raw network output: the frames' lse values [B][T] (crf_align_lse_kernel, G lanes per frame) in front of the alignment / the scores,
// on the same stream
template <typename E>
static int launch_row_lse(const void *x, const int *lx, int B, int T, int V, int64_t xs_b, int64_t xs_t, float *lse, hipStream_t st) {
    AlignParams a{};
    a.x = x; a.lx = lx; a.B = B; a.T = T; a.V = V; a.xs_b = xs_b; a.xs_t = xs_t; a.lse = lse;
    const int64_t frames = (int64_t)B * T;
    return V <= kAlnLseSmallV ? launch<crf_align_lse_kernel<16, E>>("crf_align_lse_kernel", dim3((unsigned)((frames + 15) / 16)), dim3(256), 0, st, a)
                              : launch<crf_align_lse_kernel<64, E>>("crf_align_lse_kernel", dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, st, a);
}

// ---- forced alignment (k_align.hip) ----
// one workgroup per utterance, states per thread from the longest label sequence as for the chains; LSE: raw network output, the lse
// values first, then the alignment on the upcast values
template <typename E, bool LSE>
static int launch_align(const AlignParams &p, hipStream_t st, int64_t max_label_len) {
    if constexpr (LSE)
        if (const int rc = launch_row_lse<E>(p.x, p.lx, p.B, p.T, p.V, p.xs_b, p.xs_t, p.lse, st)) return rc;
    return with_nr(2 * max_label_len + 1, kCtcThreads, [&](auto nr, int) {
        return launch<crf_ctc_align_kernel<decltype(nr)::value, E, LSE>>("crf_ctc_align_kernel", dim3((unsigned)p.B), dim3(kCtcThreads), 0, st, p);
    });
}
// its workspace: the back-pointer words [B][ceil(T / kAlnFrames)][2 * max_label_len + 1 rounded up to 64], then -- raw network output
// (crf_ctc_align_logits) -- the frames' lse values [B][T]
static const char *const kAlignWsNames[2] = {"bp", "lse"};
// < 0 with the message set; lse: with the lse section
static int64_t align_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t max_label_len, bool lse = false, SideWs *out = nullptr) {
    if (B <= 0 || T <= 0 || V <= 0 || max_label_len < 0) { set_error("crf_ctc_align: bad B/T/V/max_label_len"); return -CRF_ERR_ARG; }
    if (V > kMaxVocab) { set_error("V > " + std::to_string(kMaxVocab) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (max_label_len > kMaxCtcLabelLen) { set_error("label length > " + std::to_string(kMaxCtcLabelLen) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (B * T > INT32_MAX) { set_error("crf_ctc_align: B * T > INT32_MAX"); return -CRF_ERR_ARG; }
    const int64_t Sc = rup64((int)(2 * max_label_len + 1)), NB = (T + kAlnFrames - 1) / kAlnFrames;
    SideWs w;
    w.add(kAlignWsNames[0], B * NB * Sc * (int64_t)sizeof(unsigned));
    if (lse) w.add(kAlignWsNames[1], B * T * (int64_t)sizeof(float));
    if (out) *out = w;
    return w.total;
}
// both entry points: the checks, the argument block, the launch; dtype < 0: log-probs (crf_ctc_align), else raw output of that dtype with
// the lse values [B][T] behind the back-pointer words
static int align_call(const char *who, const void *act, int dtype, int time_major, int blank, const int32_t *labels, const int32_t *lab_off,
                      const int32_t *lx, const int32_t *ly, int64_t B, int64_t T, int64_t V, int64_t max_label_len, int32_t *pos,
                      float *score, int32_t *invalid, void *ws, int64_t ws_bytes, hipStream_t st) {
    if (!act || !labels || !lab_off || !lx || !ly || !pos || !score || !ws) { set_error(std::string(who) + ": null argument"); return CRF_ERR_ARG; }
    if (dtype > 2) return bad_dtype(who);
    SideWs w;
    const int64_t need = align_ws_bytes(B, T, V, max_label_len, dtype >= 0, &w);
    if (need < 0) return (int)-need;
    if (const int rc = check_blank(blank, V)) return rc;
    if (const int rc = check_ws(ws_bytes, need)) return rc;
    AlignParams p{};
    set_act(p, act, lx, B, T, V, blank, time_major);
    p.labels = labels; p.lab_off = lab_off; p.ly = ly;
    p.Sc = rup64((int)(2 * max_label_len + 1)); p.NB = (int)((T + kAlnFrames - 1) / kAlnFrames);
    p.bp = (unsigned *)((char *)ws + w.sec[0].off); p.pos = pos; p.score = score; p.invalid = invalid;
    if (dtype < 0) return launch_align<float, false>(p, st, max_label_len);
    p.lse = (float *)((char *)ws + w.sec[1].off);
    return with_dtype(dtype, [&](auto e) { return launch_align<decltype(e), true>(p, st, max_label_len); });
}

// ---- hypothesis scores (k_score.hip) ----
// up to kScoreWaveMaxStates states one wave per hypothesis and kScoreWaves of them per workgroup, beyond one workgroup per hypothesis (from
// two states per thread on); states per lane / thread from the call's longest hypothesis; LSE as for the alignment
template <typename E, bool LSE>
static int launch_score(const ScoreParams &p, hipStream_t st, int64_t max_hyp_len) {
    static const char *const wave_names[] = {"crf_ctc_score_wave_kernel<1>", "crf_ctc_score_wave_kernel<2>", "crf_ctc_score_wave_kernel<4>", "crf_ctc_score_wave_kernel<8>"};
    static const char *const wg_names[] = {"crf_ctc_score_wg_kernel<2>", "crf_ctc_score_wg_kernel<2>", "crf_ctc_score_wg_kernel<4>", "crf_ctc_score_wg_kernel<8>"};
    if constexpr (LSE)
        if (const int rc = launch_row_lse<E>(p.x, p.lx, p.B, p.T, p.V, p.xs_b, p.xs_t, const_cast<float *>(p.lse), st)) return rc;
    const int64_t ns = 2 * max_hyp_len + 1;
    if (ns <= kScoreWaveMaxStates)
        return with_nr(ns, 64, [&](auto nr, int k) {
            return launch<crf_ctc_score_wave_kernel<decltype(nr)::value, E, LSE>>(g_score_kernel = wave_names[k], dim3((unsigned)((p.H + kScoreWaves - 1) / kScoreWaves)),
                                                                    dim3(kScoreWaves * 64), 0, st, p);
        });
    return with_nr(ns, kCtcThreads, [&](auto nr, int k) {
        constexpr int NR = decltype(nr)::value < 2 ? 2 : decltype(nr)::value;
        return launch<crf_ctc_score_wg_kernel<NR, E, LSE>>(g_score_kernel = wg_names[k], dim3((unsigned)p.H), dim3(kCtcThreads), 0, st, p);
    });
}
// crf_ctc_score_logits' workspace: the lse values [B][T]
static int64_t score_ws_bytes(int64_t B, int64_t T, int64_t V) {
    if (B <= 0 || T <= 0 || V <= 0 || V > INT32_MAX) { set_error("crf_ctc_score: bad B/T/V"); return -CRF_ERR_ARG; }
    if (B * T > INT32_MAX) { set_error("crf_ctc_score: B * T > INT32_MAX"); return -CRF_ERR_ARG; }
    return SideWs().add("lse", B * T * (int64_t)sizeof(float)).total;
}
// both entry points: the checks, the argument block, the launch; dtype < 0: log-probs (crf_ctc_score, no workspace), else raw output of
// that dtype with the lse values in the workspace
static int score_call(const char *who, const void *act, int dtype, int time_major, int blank, const int32_t *labels, const int32_t *hyp_off,
                      const int32_t *hyp_len, const int32_t *hyp_utt, const int32_t *lx, int64_t B, int64_t H, int64_t T, int64_t V,
                      int64_t max_hyp_len, float *score, int32_t *invalid, void *ws, int64_t ws_bytes, hipStream_t st) {
    if (!act || !labels || !hyp_off || !hyp_len || !hyp_utt || !lx || !score || (dtype >= 0 && !ws)) { set_error(std::string(who) + ": null argument"); return CRF_ERR_ARG; }
    if (dtype > 2) return bad_dtype(who);
    if (H <= 0 || H > INT32_MAX || max_hyp_len < 0) { set_error(std::string(who) + ": bad H/max_hyp_len"); return CRF_ERR_ARG; }
    const int64_t need = score_ws_bytes(B, T, V);
    if (need < 0) return (int)-need;
    if (max_hyp_len > kMaxCtcLabelLen) { set_error("hypothesis length > " + std::to_string(kMaxCtcLabelLen) + " not supported by this build"); return CRF_ERR_UNSUPPORTED; }
    if (const int rc = check_blank(blank, V)) return rc;
    if (dtype >= 0)
        if (const int rc = check_ws(ws_bytes, need)) return rc;
    ScoreParams p{};
    set_act(p, act, lx, B, T, V, blank, time_major);
    p.labels = labels; p.hyp_off = hyp_off; p.hyp_len = hyp_len; p.hyp_utt = hyp_utt; p.H = (int)H;
    p.score = score; p.invalid = invalid;
    if (dtype < 0) return launch_score<float, false>(p, st, max_hyp_len);
    p.lse = (const float *)ws;
    return with_dtype(dtype, [&](auto e) { return launch_score<decltype(e), true>(p, st, max_hyp_len); });
}

// ---- the weighted gradient of the hypothesis scores (k_score_grad.hip) ----
// its workspace: the stored alphas [H][T][64 NR] in fp64 -- the occupancies, fp32, go over the first half of each row -- (NR from the call's
// longest hypothesis, as the score kernels'), then the H scores, then -- raw network output (crf_ctc_score_grad_logits) -- the frames' lse
// values [B][T].  < 0 with the message set; lse: with the lse section.
enum ScoreGradWs { kSgOcc, kSgHscore, kSgLse };
static const char *const kScoreGradWsNames[3] = {"occ", "hscore", "lse"};
static int64_t score_grad_ws_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len, bool lse = false, SideWs *out = nullptr) {
    if (B <= 0 || T <= 0 || V <= 0 || V > INT32_MAX) { set_error("crf_ctc_score_grad: bad B/T/V"); return -CRF_ERR_ARG; }
    if (H <= 0 || H > INT32_MAX || max_hyp_len < 0) { set_error("crf_ctc_score_grad: bad H/max_hyp_len"); return -CRF_ERR_ARG; }
    if (B * T > INT32_MAX) { set_error("crf_ctc_score_grad: B * T > INT32_MAX"); return -CRF_ERR_ARG; }
    if (max_hyp_len > kScoreGradMaxLen) { set_error("crf_ctc_score_grad: hypothesis length > " + std::to_string(kScoreGradMaxLen) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (V > kScoreGradMaxV) { set_error("crf_ctc_score_grad: V > " + std::to_string(kScoreGradMaxV) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    const int64_t S = with_nr(2 * max_hyp_len + 1, 64, [](auto nr, int) { return 64 * decltype(nr)::value; });
    if (H > (INT64_MAX / 16) / (T * S)) { set_error("crf_ctc_score_grad: H * T * states too large"); return -CRF_ERR_ARG; }
    SideWs w;
    w.add(kScoreGradWsNames[kSgOcc], H * T * S * (int64_t)sizeof(double)).add(kScoreGradWsNames[kSgHscore], H * (int64_t)sizeof(float));
    if (lse) w.add(kScoreGradWsNames[kSgLse], B * T * (int64_t)sizeof(float));
    if (out) *out = w;
    return w.total;
}
// the launches on one stream: RAW the frames' lse values first; then the score call's own kernel (scores into the workspace, invalid to the
// caller) -- crf_ctc_score's on log-probs, crf_ctc_score_logits' on raw output of element type E -- then the three stages
template <typename E, bool RAW>
static int launch_score_grad(const ScoreGradRawParams &p, hipStream_t st, int64_t max_hyp_len) {
    static const char *const names[] = {"crf_ctc_score_grad_alpha_kernel<1>", "crf_ctc_score_grad_alpha_kernel<2>", "crf_ctc_score_grad_alpha_kernel<4>", "crf_ctc_score_grad_alpha_kernel<8>"};
    static const char *const raw_names[3][4] = {
        {"crf_ctc_score_grad_alpha_raw_kernel<1, f32>", "crf_ctc_score_grad_alpha_raw_kernel<2, f32>", "crf_ctc_score_grad_alpha_raw_kernel<4, f32>", "crf_ctc_score_grad_alpha_raw_kernel<8, f32>"},
        {"crf_ctc_score_grad_alpha_raw_kernel<1, bf16>", "crf_ctc_score_grad_alpha_raw_kernel<2, bf16>", "crf_ctc_score_grad_alpha_raw_kernel<4, bf16>", "crf_ctc_score_grad_alpha_raw_kernel<8, bf16>"},
        {"crf_ctc_score_grad_alpha_raw_kernel<1, f16>", "crf_ctc_score_grad_alpha_raw_kernel<2, f16>", "crf_ctc_score_grad_alpha_raw_kernel<4, f16>", "crf_ctc_score_grad_alpha_raw_kernel<8, f16>"}};
    constexpr int ei = std::is_same<E, float>::value ? 0 : std::is_same<E, AlnBf16>::value ? 1 : 2;
    if constexpr (RAW)
        if (const int rc = launch_row_lse<E>(p.x, p.lx, p.B, p.T, p.V, p.xs_b, p.xs_t, const_cast<float *>(p.lse), st)) return rc;
    ScoreParams sp{};
    sp.x = p.x; sp.labels = p.labels; sp.hyp_off = p.hyp_off; sp.hyp_len = p.hyp_len; sp.hyp_utt = p.hyp_utt; sp.lx = p.lx;
    sp.B = p.B; sp.H = p.H; sp.T = p.T; sp.V = p.V; sp.blank = p.blank; sp.xs_b = p.xs_b; sp.xs_t = p.xs_t;
    sp.score = p.hscore; sp.invalid = p.invalid; sp.lse = p.lse;
    const ScoreGradParams &pl = p;            // the log-prob kernels' block
    const dim3 grid((unsigned)((p.H + kScoreWaves - 1) / kScoreWaves)), block(kScoreWaves * 64);
    int rc = with_nr(2 * max_hyp_len + 1, 64, [&](auto nr, int k) {
        constexpr int NR = decltype(nr)::value;
        if (const int r = launch<crf_ctc_score_wave_kernel<NR, E, RAW>>("crf_ctc_score_wave_kernel", grid, block, 0, st, sp)) return r;
        if constexpr (RAW) {
            if (const int r = launch<crf_ctc_score_grad_alpha_raw_kernel<NR, E>>(g_score_grad_kernel = raw_names[ei][k], grid, block, 0, st, p)) return r;
            return launch<crf_ctc_score_grad_beta_raw_kernel<NR, E>>("crf_ctc_score_grad_beta_raw_kernel", grid, block, 0, st, p);
        } else {
            if (const int r = launch<crf_ctc_score_grad_alpha_kernel<NR>>(g_score_grad_kernel = names[k], grid, block, 0, st, pl)) return r;
            return launch<crf_ctc_score_grad_beta_kernel<NR>>("crf_ctc_score_grad_beta_kernel", grid, block, 0, st, pl);
        }
    });
    if (rc) return rc;
    const int64_t nbt = (p.T + p.FB - 1) / p.FB;
    const dim3 rgrid((unsigned)(p.B * nbt)), rblock(kScoreGradReduceThreads);
    const size_t lds = (size_t)p.FB * p.V * sizeof(float);
    if constexpr (RAW) return launch<crf_ctc_score_grad_reduce_raw_kernel<E>>("crf_ctc_score_grad_reduce_raw_kernel", rgrid, rblock, lds, st, p);
    else return launch<crf_ctc_score_grad_reduce_kernel>("crf_ctc_score_grad_reduce_kernel", rgrid, rblock, lds, st, pl);
}
// both entry points: the checks, the argument block, the launches; dtype < 0: log-probs (crf_ctc_score_grad), else raw output of that dtype
// with the lse values behind the scores
static int score_grad_call(const char *who, const void *act, int dtype, int time_major, int blank, const int32_t *labels, const int32_t *hyp_off,
                           const int32_t *hyp_len, const int32_t *hyp_utt, const int32_t *lx, const float *weight, int64_t B, int64_t H,
                           int64_t T, int64_t V, int64_t max_hyp_len, float *score, int32_t *invalid, float *grad, void *ws, int64_t ws_bytes,
                           hipStream_t st) {
    if (!act || !labels || !hyp_off || !hyp_len || !hyp_utt || !lx || !grad || !ws) { set_error(std::string(who) + ": null argument"); return CRF_ERR_ARG; }
    if (dtype > 2) return bad_dtype(who);
    SideWs w;
    const int64_t need = score_grad_ws_bytes(B, H, T, V, max_hyp_len, dtype >= 0, &w);
    if (need < 0) return (int)-need;
    if (const int rc = check_blank(blank, V)) return rc;
    if (const int rc = check_ws(ws_bytes, need)) return rc;
    ScoreGradRawParams p{};
    set_act(p, act, lx, B, T, V, blank, time_major);
    p.labels = labels; p.hyp_off = hyp_off; p.hyp_len = hyp_len; p.hyp_utt = hyp_utt; p.H = (int)H;
    p.score = score; p.invalid = invalid; p.weight = weight; p.grad = grad;
    p.occ = (float *)((char *)ws + w.sec[kSgOcc].off); p.hscore = (float *)((char *)ws + w.sec[kSgHscore].off);
    p.S = (int)(w.sec[kSgOcc].bytes / (H * T * (int64_t)sizeof(double)));
    p.FB = (int)std::min<int64_t>(kScoreGradFrames, std::max<int64_t>(1, kScoreGradMaxV / V));
    if (dtype < 0) return launch_score_grad<float, false>(p, st, max_hyp_len);
    p.lse = (const float *)((char *)ws + w.sec[kSgLse].off);
    return with_dtype(dtype, [&](auto e) { return launch_score_grad<decltype(e), true>(p, st, max_hyp_len); });
}

// ---- scores and their gradient on hypotheses that lie on the device as padded rows (k_rows.hip) ----
// The host knows a bound len_cap on the lengths, not the lengths: the plan kernel gives every hypothesis the class of its own length, every
// class up to len_cap's runs the call's existing kernel on a masked length row, the merge kernel picks each hypothesis's result.
// Workspace: the gradient's occ [H][T][S] fp64 (S = 64 NR of len_cap's class) and hscore [H] in front, then hyp_off [H], cls [H],
// len [ncls][H], cscore [ncls][H], cinvalid [ncls][H] and -- raw network output -- the lse values [B][T].
enum RowsWsSec { kRwOcc, kRwHscore, kRwOff, kRwCls, kRwLen, kRwCscore, kRwCinvalid, kRwLse, kRwCount };
static const char *const kRowsWsNames[kRwCount] = {"occ", "hscore", "hyp_off", "cls", "len", "cscore", "cinvalid", "lse"};
static const char *rows_who(bool grad) { return grad ? "crf_ctc_score_grad_rows" : "crf_ctc_score_rows"; }
// < 0 with the message set; the sections of a score call are the gradient's without the first two
static int64_t rows_ws_bytes(bool grad, int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, int dtype, SideWs *out = nullptr) {
    const std::string who = rows_who(grad);
    if (dtype < -1 || dtype > 2) { set_error(who + ": dtype must be -1 (f32 log-probs), 0 (f32), 1 (bf16) or 2 (f16)"); return -CRF_ERR_ARG; }
    if (B <= 0 || H <= 0 || T <= 0 || V <= 0 || H > INT32_MAX || V > INT32_MAX || len_cap < 0) { set_error(who + ": bad B/H/T/V/len_cap"); return -CRF_ERR_ARG; }
    if (B > INT32_MAX / T) { set_error(who + ": B * T > INT32_MAX"); return -CRF_ERR_ARG; }
    const int64_t limit = grad ? kScoreGradMaxLen : kMaxCtcLabelLen;
    if (len_cap > limit) { set_error(who + ": len_cap > " + std::to_string(limit) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (grad && V > kScoreGradMaxV) { set_error(who + ": V > " + std::to_string(kScoreGradMaxV) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    const int64_t ncls = rows_class((int)len_cap) + 1, hb = H * (int64_t)sizeof(int);
    SideWs w;
    if (grad) {
        const int64_t S = 64ll << (ncls - 1);
        if (H > (INT64_MAX / 16) / (T * S)) { set_error(who + ": H * T * states too large"); return -CRF_ERR_ARG; }
        w.add(kRowsWsNames[kRwOcc], H * T * S * (int64_t)sizeof(double)).add(kRowsWsNames[kRwHscore], hb);
    }
    w.add(kRowsWsNames[kRwOff], hb).add(kRowsWsNames[kRwCls], hb).add(kRowsWsNames[kRwLen], ncls * hb).add(kRowsWsNames[kRwCscore], ncls * hb)
     .add(kRowsWsNames[kRwCinvalid], ncls * hb);
    if (dtype >= 0) w.add(kRowsWsNames[kRwLse], B * T * (int64_t)sizeof(float));
    if (out) *out = w;
    return w.total;
}
// the checks of both entry points, in the order of include/ctc_crf_hip.h; CRF_OK: w holds the sections
static int rows_check(bool grad, const void *act, int dtype, int blank, const int32_t *hyps, int64_t hyp_stride, const int32_t *hyp_len,
                      const int32_t *hyp_utt, const int32_t *lx, int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, const void *out,
                      const void *ws, int64_t ws_bytes, SideWs &w) {
    const std::string who = rows_who(grad);
    if (!act || !hyps || !hyp_len || !hyp_utt || !lx || !out || !ws) { set_error(who + ": null argument"); return CRF_ERR_ARG; }
    if (dtype < -1 || dtype > 2) return (int)-rows_ws_bytes(grad, 1, 1, 1, 1, 0, dtype);
    if (B <= 0 || H <= 0 || T <= 0 || V <= 0 || hyp_stride <= 0 || len_cap < 0) { set_error(who + ": bad B/H/T/V/hyp_stride/len_cap"); return CRF_ERR_ARG; }
    if (H > INT32_MAX / hyp_stride) { set_error(who + ": H * hyp_stride > INT32_MAX"); return CRF_ERR_ARG; }
    if (B > INT32_MAX / T) { set_error(who + ": B * T > INT32_MAX"); return CRF_ERR_ARG; }
    if (V > INT32_MAX) { set_error(who + ": bad V"); return CRF_ERR_ARG; }
    if (const int rc = check_blank(blank, V)) return rc;
    const int64_t need = rows_ws_bytes(grad, B, H, T, V, len_cap, dtype, &w);
    if (need < 0) return (int)-need;
    return check_ws(ws_bytes, need);
}
static const char *const kRowsScoreNames[kRowsClasses] = {"crf_ctc_score_wave_kernel<1>", "crf_ctc_score_wave_kernel<2>", "crf_ctc_score_wave_kernel<4>", "crf_ctc_score_wave_kernel<8>",
                                                          "crf_ctc_score_wg_kernel<2>", "crf_ctc_score_wg_kernel<4>", "crf_ctc_score_wg_kernel<8>"};
// the score kernel of class c on all H hypotheses (p.hyp_len: the class's masked lengths); the lse values are in place
template <typename E, bool LSE>
static int launch_score_class(int c, const ScoreParams &p, hipStream_t st) {
    const dim3 wgrid((unsigned)((p.H + kScoreWaves - 1) / kScoreWaves)), wblock(kScoreWaves * 64), ggrid((unsigned)p.H), gblock(kCtcThreads);
    switch (c) {
    case 0: return launch<crf_ctc_score_wave_kernel<1, E, LSE>>(kRowsScoreNames[0], wgrid, wblock, 0, st, p);
    case 1: return launch<crf_ctc_score_wave_kernel<2, E, LSE>>(kRowsScoreNames[1], wgrid, wblock, 0, st, p);
    case 2: return launch<crf_ctc_score_wave_kernel<4, E, LSE>>(kRowsScoreNames[2], wgrid, wblock, 0, st, p);
    case 3: return launch<crf_ctc_score_wave_kernel<8, E, LSE>>(kRowsScoreNames[3], wgrid, wblock, 0, st, p);
    case 4: return launch<crf_ctc_score_wg_kernel<2, E, LSE>>(kRowsScoreNames[4], ggrid, gblock, 0, st, p);
    case 5: return launch<crf_ctc_score_wg_kernel<4, E, LSE>>(kRowsScoreNames[5], ggrid, gblock, 0, st, p);
    default: return launch<crf_ctc_score_wg_kernel<kCtcRegs, E, LSE>>(kRowsScoreNames[6], ggrid, gblock, 0, st, p);
    }
}
// ... and behind it stages 1 and 2 of the gradient of wave class c, their rows of occ p.S doubles apart
template <typename E, bool RAW>
static int launch_score_grad_class(int c, const ScoreParams &sp, const ScoreGradRawParams &p, hipStream_t st) {
    const dim3 grid((unsigned)((p.H + kScoreWaves - 1) / kScoreWaves)), block(kScoreWaves * 64);
    const ScoreGradParams &pl = p;
    if (const int rc = launch_score_class<E, RAW>(c, sp, st)) return rc;
    auto stages = [&](auto nr) {
        constexpr int NR = decltype(nr)::value;
        if constexpr (RAW) {
            if (const int r = launch<crf_rows_grad_alpha_raw_kernel<NR, E>>("crf_rows_grad_alpha_raw_kernel", grid, block, 0, st, p)) return r;
            return launch<crf_rows_grad_beta_raw_kernel<NR, E>>("crf_rows_grad_beta_raw_kernel", grid, block, 0, st, p);
        } else {
            if (const int r = launch<crf_rows_grad_alpha_kernel<NR>>("crf_rows_grad_alpha_kernel", grid, block, 0, st, pl)) return r;
            return launch<crf_rows_grad_beta_kernel<NR>>("crf_rows_grad_beta_kernel", grid, block, 0, st, pl);
        }
    };
    switch (c) {
    case 0: return stages(std::integral_constant<int, 1>{});
    case 1: return stages(std::integral_constant<int, 2>{});
    case 2: return stages(std::integral_constant<int, 4>{});
    default: return stages(std::integral_constant<int, 8>{});
    }
}
// what both calls launch first: the plan, and -- raw network output -- the frames' lse values, ONCE for all classes
static int launch_rows_front(const RowsPlanParams &pp, const void *act, int dtype, const ScoreParams &p, hipStream_t st) {
    if (const int rc = launch<crf_rows_plan_kernel>("crf_rows_plan_kernel", dim3((unsigned)((pp.H + kRowsThreads - 1) / kRowsThreads)), dim3(kRowsThreads), 0, st, pp)) return rc;
    if (dtype < 0) return CRF_OK;
    return with_dtype(dtype, [&](auto e) { return launch_row_lse<decltype(e)>(act, p.lx, p.B, p.T, p.V, p.xs_b, p.xs_t, const_cast<float *>(p.lse), st); });
}
static int launch_rows_merge(const RowsMergeParams &mp, hipStream_t st) {
    return launch<crf_rows_merge_kernel>("crf_rows_merge_kernel", dim3((unsigned)((mp.H + kRowsThreads - 1) / kRowsThreads)), dim3(kRowsThreads), 0, st, mp);
}
// crf_ctc_score_rows: dtype < 0 log-probs, else raw output of that dtype
static int score_rows_call(const void *act, int dtype, int time_major, int blank, const int32_t *hyps, int64_t hyp_stride, const int32_t *hyp_len,
                           const int32_t *hyp_utt, const int32_t *lx, int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, float *score,
                           int32_t *invalid, void *ws, int64_t ws_bytes, hipStream_t st) {
    SideWs w;
    if (const int rc = rows_check(false, act, dtype, blank, hyps, hyp_stride, hyp_len, hyp_utt, lx, B, H, T, V, len_cap, score, ws, ws_bytes, w)) return rc;
    auto sec = [&](int k) { return (char *)ws + w.sec[k - kRwOff].off; };   // (a score call has no occ and no hscore)
    const int ncls = rows_class((int)len_cap) + 1;
    const RowsPlanParams pp{hyp_len, (int)H, (int)hyp_stride, (int)len_cap, ncls, (int *)sec(kRwOff), (int *)sec(kRwCls), (int *)sec(kRwLen)};
    float *cscore = (float *)sec(kRwCscore);
    int *cinvalid = (int *)sec(kRwCinvalid);
    ScoreParams p{};
    set_act(p, act, lx, B, T, V, blank, time_major);
    p.labels = hyps; p.hyp_off = pp.hyp_off; p.hyp_utt = hyp_utt; p.H = (int)H;
    if (dtype >= 0) p.lse = (const float *)sec(kRwLse);
    if (const int rc = launch_rows_front(pp, act, dtype, p, st)) return rc;
    for (int c = 0; c < ncls; ++c) {
        p.hyp_len = pp.len_c + (int64_t)c * H; p.score = cscore + (int64_t)c * H; p.invalid = cinvalid + (int64_t)c * H;
        const int rc = dtype < 0 ? launch_score_class<float, false>(c, p, st)
                                 : with_dtype(dtype, [&](auto e) { return launch_score_class<decltype(e), true>(c, p, st); });
        if (rc) return rc;
    }
    g_score_kernel = kRowsScoreNames[ncls - 1];
    return launch_rows_merge(RowsMergeParams{pp.cls, cscore, cinvalid, (int)H, ncls, score, nullptr, invalid}, st);
}
// crf_ctc_score_grad_rows: per wave class the score kernel and stages 1 and 2 into ONE occ section, the merge, then the one reduce launch
// on the merged scores and the true lengths (it reads the length of a live hypothesis only)
static int score_grad_rows_call(const void *act, int dtype, int time_major, int blank, const int32_t *hyps, int64_t hyp_stride,
                                const int32_t *hyp_len, const int32_t *hyp_utt, const int32_t *lx, const float *weight, int64_t B, int64_t H,
                                int64_t T, int64_t V, int64_t len_cap, float *score, int32_t *invalid, float *grad, void *ws, int64_t ws_bytes,
                                hipStream_t st) {
    static const char *const names[kRowsWaveClasses] = {"crf_rows_grad_alpha_kernel<1>", "crf_rows_grad_alpha_kernel<2>",
                                                        "crf_rows_grad_alpha_kernel<4>", "crf_rows_grad_alpha_kernel<8>"};
    static const char *const raw_names[3][kRowsWaveClasses] = {
        {"crf_rows_grad_alpha_raw_kernel<1, f32>", "crf_rows_grad_alpha_raw_kernel<2, f32>", "crf_rows_grad_alpha_raw_kernel<4, f32>", "crf_rows_grad_alpha_raw_kernel<8, f32>"},
        {"crf_rows_grad_alpha_raw_kernel<1, bf16>", "crf_rows_grad_alpha_raw_kernel<2, bf16>", "crf_rows_grad_alpha_raw_kernel<4, bf16>", "crf_rows_grad_alpha_raw_kernel<8, bf16>"},
        {"crf_rows_grad_alpha_raw_kernel<1, f16>", "crf_rows_grad_alpha_raw_kernel<2, f16>", "crf_rows_grad_alpha_raw_kernel<4, f16>", "crf_rows_grad_alpha_raw_kernel<8, f16>"}};
    SideWs w;
    if (const int rc = rows_check(true, act, dtype, blank, hyps, hyp_stride, hyp_len, hyp_utt, lx, B, H, T, V, len_cap, grad, ws, ws_bytes, w)) return rc;
    auto sec = [&](int k) { return (char *)ws + w.sec[k].off; };
    const int ncls = rows_class((int)len_cap) + 1;
    const RowsPlanParams pp{hyp_len, (int)H, (int)hyp_stride, (int)len_cap, ncls, (int *)sec(kRwOff), (int *)sec(kRwCls), (int *)sec(kRwLen)};
    float *cscore = (float *)sec(kRwCscore);
    int *cinvalid = (int *)sec(kRwCinvalid);
    ScoreGradRawParams p{};
    set_act(p, act, lx, B, T, V, blank, time_major);
    p.labels = hyps; p.hyp_off = pp.hyp_off; p.hyp_utt = hyp_utt; p.H = (int)H;
    p.weight = weight; p.grad = grad;         // (score and invalid stay null in the class passes: the merge writes the caller's)
    p.occ = (float *)sec(kRwOcc);
    p.S = 64 << (ncls - 1);
    p.FB = (int)std::min<int64_t>(kScoreGradFrames, std::max<int64_t>(1, kScoreGradMaxV / V));
    if (dtype >= 0) p.lse = (const float *)sec(kRwLse);
    ScoreParams sp{};
    set_act(sp, act, lx, B, T, V, blank, time_major);
    sp.labels = hyps; sp.hyp_off = pp.hyp_off; sp.hyp_utt = hyp_utt; sp.H = (int)H; sp.lse = p.lse;
    if (const int rc = launch_rows_front(pp, act, dtype, sp, st)) return rc;
    for (int c = 0; c < ncls; ++c) {
        sp.hyp_len = p.hyp_len = pp.len_c + (int64_t)c * H;
        sp.score = p.hscore = cscore + (int64_t)c * H;
        sp.invalid = cinvalid + (int64_t)c * H;
        const int rc = dtype < 0 ? launch_score_grad_class<float, false>(c, sp, p, st)
                                 : with_dtype(dtype, [&](auto e) { return launch_score_grad_class<decltype(e), true>(c, sp, p, st); });
        if (rc) return rc;
    }
    g_score_grad_kernel = dtype < 0 ? names[ncls - 1] : raw_names[dtype][ncls - 1];
    p.hscore = (float *)sec(kRwHscore);
    if (const int rc = launch_rows_merge(RowsMergeParams{pp.cls, cscore, cinvalid, (int)H, ncls, score, p.hscore, invalid}, st)) return rc;
    p.hyp_len = hyp_len;
    const int64_t nbt = (p.T + p.FB - 1) / p.FB;
    const dim3 rgrid((unsigned)(p.B * nbt)), rblock(kScoreGradReduceThreads);
    const size_t lds = (size_t)p.FB * p.V * sizeof(float);
    if (dtype < 0) return launch<crf_ctc_score_grad_reduce_kernel>("crf_ctc_score_grad_reduce_kernel", rgrid, rblock, lds, st, (const ScoreGradParams &)p);
    return with_dtype(dtype, [&](auto e) { return launch<crf_ctc_score_grad_reduce_raw_kernel<decltype(e)>>("crf_ctc_score_grad_reduce_raw_kernel", rgrid, rblock, lds, st, p); });
}

// ---- sampled / best-path label sequences (k_sample.hip) ----
// the row stage over the B T frames -- 16 lanes per row up to kSampleSmallV classes, beyond a wave per row, per row V + 2 G words of
// dynamic LDS (none for the arg-max) -- then the collapse, one wave per path, on the same stream
template <typename E>
static int launch_sample(const SampleParams &p, hipStream_t st, bool greedy) {
    const int64_t frames = (int64_t)p.B * p.T, H = (int64_t)p.B * p.K;
    auto rows = [&](auto g, const char *name, const char *name_greedy) {
        constexpr int G = decltype(g)::value, R = kSampleRowThreads(G) / G;   // rows per workgroup
        const dim3 grid((unsigned)((frames + R - 1) / R)), block(kSampleRowThreads(G));
        return greedy ? launch<crf_sample_row_kernel<G, E, true>>(g_sample_kernel = name_greedy, grid, block, 0, st, p)
                      : launch<crf_sample_row_kernel<G, E, false>>(g_sample_kernel = name, grid, block, (size_t)R * (p.V + 2 * G) * sizeof(float), st, p);
    };
    const int rc = p.V <= kSampleSmallV ? rows(std::integral_constant<int, 16>{}, "crf_sample_row_kernel<16>", "crf_sample_row_kernel<16, greedy>")
                                        : rows(std::integral_constant<int, 64>{}, "crf_sample_row_kernel<64>", "crf_sample_row_kernel<64, greedy>");
    return rc ? rc : launch<crf_sample_collapse_kernel>("crf_sample_collapse_kernel", dim3((unsigned)((H + kSampleWaves - 1) / kSampleWaves)),
                                                        dim3(kSampleWaves * 64), 0, st, p);
}
// its workspace: the classes drawn per frame, [B K][T] int32
static int64_t sample_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t K) {
    if (B <= 0 || T <= 0 || V <= 0 || K <= 0) { set_error("crf_ctc_sample: bad B/T/V/K"); return -CRF_ERR_ARG; }
    if (B > INT32_MAX || T > INT32_MAX || K > INT32_MAX || B * T > INT32_MAX) { set_error("crf_ctc_sample: B * T > INT32_MAX"); return -CRF_ERR_ARG; }
    if (B * K > INT32_MAX) { set_error("crf_ctc_sample: B * K > INT32_MAX"); return -CRF_ERR_ARG; }
    if (V > kSampleMaxV) { set_error("V > " + std::to_string(kSampleMaxV) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (K > (INT64_MAX / 8) / (B * T)) { set_error("crf_ctc_sample: B * K * T too large"); return -CRF_ERR_ARG; }
    return SideWs().add("cls", B * K * T * (int64_t)sizeof(int32_t)).total;
}

// ---- prefix beam search (k_beam.hip) ----
// its workspace: the frames' blank value and top-C (value, class) pairs, [B T][C + 1] floats and as many int32, then the trace words
// [B][T][W] int32 (not used by a call that brings a trace buffer of its own).  < 0 with the message set.
enum BeamWs { kBmVal, kBmCls, kBmTrace };
static const char *const kBeamWsNames[3] = {"val", "cls", "trace"};
static int64_t beam_ws_bytes(int64_t B, int64_t T, int64_t V, int64_t W, int64_t C, SideWs *out = nullptr) {
    if (B <= 0 || T <= 0 || V <= 0) { set_error("crf_ctc_beam: bad B/T/V"); return -CRF_ERR_ARG; }
    if (W < 1 || W > kBeamMaxW) { set_error("crf_ctc_beam: beam width " + std::to_string(W) + " outside [1, " + std::to_string(kBeamMaxW) + "]"); return -CRF_ERR_ARG; }
    if (C < 1 || C > kBeamMaxC) { set_error("crf_ctc_beam: top_classes " + std::to_string(C) + " outside [1, " + std::to_string(kBeamMaxC) + "]"); return -CRF_ERR_ARG; }
    if (B > INT32_MAX || T > INT32_MAX || B * T > INT32_MAX) { set_error("crf_ctc_beam: B * T > INT32_MAX"); return -CRF_ERR_ARG; }
    if (V > kBeamMaxV) { set_error("V > " + std::to_string(kBeamMaxV) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    const int64_t rs = std::min(C, V - 1) + 1;
    SideWs w;
    w.add(kBeamWsNames[kBmVal], B * T * rs * (int64_t)sizeof(float)).add(kBeamWsNames[kBmCls], B * T * rs * (int64_t)sizeof(int32_t))
     .add(kBeamWsNames[kBmTrace], B * T * W * (int64_t)sizeof(int32_t));
    if (out) *out = w;
    return w.total;
}
// the row stage over the B T frames, then one wave per utterance, on the same stream
template <typename E>
static int launch_beam(const BeamParams &p, hipStream_t st) {
    static const char *const names[3] = {"crf_beam_row_kernel<f32>", "crf_beam_row_kernel<bf16>", "crf_beam_row_kernel<f16>"};
    constexpr int ei = std::is_same<E, float>::value ? 0 : std::is_same<E, AlnBf16>::value ? 1 : 2;
    const int64_t frames = (int64_t)p.B * p.T;
    const int R = p.V <= kBeamRowsV ? 4 : 1;
    if (const int rc = launch<crf_beam_row_kernel<E>>(g_beam_kernel = names[ei], dim3((unsigned)((frames + R - 1) / R)), dim3(64 * R),
                                                      (size_t)R * p.V * sizeof(float), st, p)) return rc;
    return launch<crf_beam_search_kernel>("crf_beam_search_kernel", dim3((unsigned)p.B), dim3(64), 0, st, p);
}
// the same row stage, then the fused search of k_beam_lm.hip: one workgroup of kBeamLmWaves waves per utterance
template <typename E>
static int launch_beam_lm(const BeamLmParams &q, hipStream_t st) {
    static const char *const names[3] = {"crf_beam_row_kernel<f32>", "crf_beam_row_kernel<bf16>", "crf_beam_row_kernel<f16>"};
    constexpr int ei = std::is_same<E, float>::value ? 0 : std::is_same<E, AlnBf16>::value ? 1 : 2;
    const BeamParams &p = q.b;
    const int64_t frames = (int64_t)p.B * p.T;
    const int R = p.V <= kBeamRowsV ? 4 : 1;
    if (const int rc = launch<crf_beam_row_kernel<E>>(g_beam_kernel = names[ei], dim3((unsigned)((frames + R - 1) / R)), dim3(64 * R),
                                                      (size_t)R * p.V * sizeof(float), st, p)) return rc;
    return launch<crf_beamlm_search_kernel>("crf_beamlm_search_kernel", dim3((unsigned)p.B), dim3(64 * kBeamLmWaves), 0, st, q);
}
// the argument checks of crf_ctc_beam, crf_ctc_beam_lm (lm: null for the LM-free call) and crf_ctc_beam_chunk, and the kernels' arguments;
// no HIP call
static int beam_setup(const char *who, const void *act, int dtype, int time_major, int blank, int normalize, const int32_t *lx, int64_t B,
                      int64_t T, int64_t V, int64_t W, int64_t nbest, int64_t top_classes, const crf_ngram_tables *lm, bool with_lm, float alpha,
                      float beta, int32_t *hyps, int32_t *hyp_len, float *score, float *lm_score, int32_t *trace, void *ws, int64_t ws_bytes,
                      BeamLmParams &q) {
    const std::string w0 = std::string(who) + ": ";
    if (!act || !lx || !hyps || !hyp_len || !score || !ws || (with_lm && !lm)) { set_error(w0 + "null argument"); return CRF_ERR_ARG; }
    if (dtype < 0 || dtype > 2) return bad_dtype(who);
    if (normalize != 0 && normalize != 1) { set_error(w0 + "normalize must be 0 or 1, got " + std::to_string(normalize)); return CRF_ERR_ARG; }
    SideWs w;
    const int64_t need = beam_ws_bytes(B, T, V, W, top_classes, &w);
    if (need < 0) return (int)-need;
    if (nbest < 1 || nbest > W) { set_error(w0 + "nbest " + std::to_string(nbest) + " outside [1, W=" + std::to_string(W) + "]"); return CRF_ERR_ARG; }
    if (const int rc = check_blank(blank, V)) return rc;
    if (with_lm) {
        if (!std::isfinite(alpha) || !std::isfinite(beta)) {
            set_error(w0 + "alpha and beta must be finite, got " + std::to_string(alpha) + " and " + std::to_string(beta)); return CRF_ERR_ARG;
        }
        if (lm->V != V) { set_error(w0 + "the LM's V " + std::to_string(lm->V) + " is not the activations' V " + std::to_string(V)); return CRF_ERR_ARG; }
        if (lm->S < 1 || lm->S > INT32_MAX || lm->A < 0 || lm->A > INT32_MAX || lm->order < 1 || lm->order > kNgramMaxOrder || lm->start < 0 ||
            lm->start >= lm->S) {
            set_error(w0 + "bad LM tables: S " + std::to_string(lm->S) + ", A " + std::to_string(lm->A) + ", order " + std::to_string(lm->order) +
                      ", start " + std::to_string(lm->start));
            return CRF_ERR_ARG;
        }
        if (!lm->row_off || !lm->bo_state || !lm->bo_weight || !lm->uni_logp || !lm->uni_next ||
            (lm->A > 0 && (!lm->arc_label || !lm->arc_logp || !lm->arc_next))) { set_error(w0 + "null LM table"); return CRF_ERR_ARG; }
    }
    if (const int rc = check_ws(ws_bytes, need)) return rc;
    q = BeamLmParams{};
    BeamParams &p = q.b;
    set_act(p, act, lx, B, T, V, blank, time_major);
    p.W = (int)W; p.nbest = (int)nbest; p.C = (int)std::min(top_classes, V - 1); p.normalize = normalize;
    p.val = (float *)((char *)ws + w.sec[kBmVal].off); p.cls = (int *)((char *)ws + w.sec[kBmCls].off);
    p.trace = trace ? trace : (int *)((char *)ws + w.sec[kBmTrace].off); p.fill_trace = trace != nullptr;
    p.hyps = hyps; p.hyp_len = hyp_len; p.score = score;
    if (!with_lm) return CRF_OK;
    q.lm.row_off = lm->row_off; q.lm.arc_label = lm->arc_label; q.lm.arc_logp = lm->arc_logp; q.lm.arc_next = lm->arc_next;
    q.lm.bo_state = lm->bo_state; q.lm.bo_weight = lm->bo_weight; q.lm.uni_logp = lm->uni_logp; q.lm.uni_next = lm->uni_next;
    q.lm.S = (int)lm->S; q.lm.A = (int)lm->A; q.lm.V = (int)lm->V; q.lm.order = lm->order; q.lm.start = lm->start;
    q.alpha = alpha; q.beta = beta; q.lm_score = lm_score;
    return CRF_OK;
}
// crf_ctc_beam and crf_ctc_beam_lm: the checks, then the launch; every error before any HIP call
static int beam_call(const char *who, const void *act, int dtype, int time_major, int blank, int normalize, const int32_t *lx, int64_t B,
                     int64_t T, int64_t V, int64_t W, int64_t nbest, int64_t top_classes, const crf_ngram_tables *lm, bool with_lm, float alpha,
                     float beta, int32_t *hyps, int32_t *hyp_len, float *score, float *lm_score, int32_t *trace, void *ws, int64_t ws_bytes,
                     hipStream_t st) {
    BeamLmParams q;
    if (const int rc = beam_setup(who, act, dtype, time_major, blank, normalize, lx, B, T, V, W, nbest, top_classes, lm, with_lm, alpha, beta, hyps,
                                  hyp_len, score, lm_score, trace, ws, ws_bytes, q)) return rc;
    if (!with_lm) return with_dtype(dtype, [&](auto e) { return launch_beam<decltype(e)>(q.b, st); });
    return with_dtype(dtype, [&](auto e) { return launch_beam_lm<decltype(e)>(q, st); });
}
// the row stage on the chunk's frames, then the search that loads and stores the beam (k_beam_chunk.hip), on the same stream
template <typename E>
static int launch_beam_chunk(const BeamChunkParams &cp, bool with_lm, hipStream_t st) {
    static const char *const names[3] = {"crf_beam_row_kernel<f32>", "crf_beam_row_kernel<bf16>", "crf_beam_row_kernel<f16>"};
    constexpr int ei = std::is_same<E, float>::value ? 0 : std::is_same<E, AlnBf16>::value ? 1 : 2;
    const BeamParams &p = cp.q.b;
    const int64_t frames = (int64_t)p.B * p.T;
    const int R = p.V <= kBeamRowsV ? 4 : 1;
    if (const int rc = launch<crf_beam_row_kernel<E>>(g_beam_kernel = names[ei], dim3((unsigned)((frames + R - 1) / R)), dim3(64 * R),
                                                      (size_t)R * p.V * sizeof(float), st, p)) return rc;
    return with_lm ? launch<crf_beamlm_chunk_kernel>("crf_beamlm_chunk_kernel", dim3((unsigned)p.B), dim3(64 * kBeamLmWaves), 0, st, cp)
                   : launch<crf_beam_chunk_kernel>("crf_beam_chunk_kernel", dim3((unsigned)p.B), dim3(64), 0, st, cp);
}

// ---- edit distance (k_edit.hip) ----
// references of up to kEditStripRows tokens: one wave per hypothesis with the rows in registers, kEditWaves of them per workgroup, rows
// per lane from the call's longest reference; beyond: strips, one wave per workgroup and a cell per hypothesis column in dynamic LDS
static int launch_edit(const EditParams &p, hipStream_t st) {
    static const char *const names[] = {"crf_ctc_edit_kernel<1>", "crf_ctc_edit_kernel<2>", "crf_ctc_edit_kernel<4>", "crf_ctc_edit_kernel<8>"};
    if (p.max_ref > kEditStripRows)
        return launch<crf_ctc_edit_kernel<8, true>>(g_edit_kernel = "crf_ctc_edit_kernel<8, strips>", dim3((unsigned)p.H), dim3(64),
                                                    (size_t)p.stride * sizeof(int2), st, p);
    return with_nr(p.max_ref, 64, [&](auto nr, int k) {
        return launch<crf_ctc_edit_kernel<decltype(nr)::value, false>>(g_edit_kernel = names[k], dim3((unsigned)((p.H + kEditWaves - 1) / kEditWaves)),
                                                                       dim3(kEditWaves * 64), 0, st, p);
    });
}

// ---- n-gram LM scores of rows (k_ngram.hip) ----
// one wave per hypothesis, kNgramScoreWaves of them per workgroup, the grid over H in x; the per-token stores only where asked for
static int launch_ngram_score(const NgramScoreParams &p, hipStream_t st) {
    const dim3 grid((unsigned)((p.H + kNgramScoreWaves - 1) / kNgramScoreWaves)), block(64 * kNgramScoreWaves);
    if (p.tok_logp || p.tok_order) return launch<crf_ngram_score_kernel<true>>(g_ngram_kernel = "crf_ngram_score_kernel<tokens>", grid, block, 0, st, p);
    return launch<crf_ngram_score_kernel<false>>(g_ngram_kernel = "crf_ngram_score_kernel<scores>", grid, block, 0, st, p);
}

// ---- the RNN-T loss and its gradient (k_rnnt.hip) ----
// The workspace both calls share, R = the rows of the joiner output (N T U1 padded, compact_rows compact): row [R][4] floats (M, log s, lb, ll),
// alpha [R] and beta [R] fp64, utt: total [N] fp64, then node_off [N + 1], lab_off [N], tn [N], un [N] int32.  < 0 with the message set.
enum RnntWs { kRtRow, kRtAlpha, kRtBeta, kRtUtt, kRtCount };
static const char *const kRnntWsNames[kRtCount] = {"row", "alpha", "beta", "utt"};
static int64_t rnnt_ws_bytes(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t compact_rows, SideWs *out = nullptr, int64_t *rows = nullptr) {
    const std::string who = "crf_rnnt_loss: ";
    if (N <= 0 || T <= 0 || U1 <= 0 || V <= 0 || N > INT32_MAX || T > INT32_MAX) { set_error(who + "bad N/T/U+1/V"); return -CRF_ERR_ARG; }
    if (U1 > kRnntMaxU1) { set_error(who + "U > " + std::to_string(kRnntMaxU1 - 1) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (V > kRnntMaxV) { set_error(who + "V > " + std::to_string(kRnntMaxV) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    // (an utterance's nodes are indexed in 32 bits, times four for the row section: T U1 padded, at most all rows compact)
    if (compact_rows < 0 && T > (INT32_MAX / 4) / U1) { set_error(who + "T * (U + 1) > INT32_MAX / 4"); return -CRF_ERR_ARG; }
    if (compact_rows > INT32_MAX / 4) { set_error(who + "compact_rows > INT32_MAX / 4"); return -CRF_ERR_ARG; }
    const int64_t R = compact_rows < 0 ? N * T * U1 : compact_rows;
    if (R <= 0 || R > INT32_MAX || (compact_rows < 0 && N > INT32_MAX / (T * U1))) { set_error(who + "rows outside [1, INT32_MAX]"); return -CRF_ERR_ARG; }
    SideWs w;
    w.add(kRnntWsNames[kRtRow], 4 * R * (int64_t)sizeof(float)).add(kRnntWsNames[kRtAlpha], R * (int64_t)sizeof(double))
     .add(kRnntWsNames[kRtBeta], R * (int64_t)sizeof(double)).add(kRnntWsNames[kRtUtt], N * (int64_t)sizeof(double) + (4 * N + 1) * (int64_t)sizeof(int32_t));
    if (out) *out = w;
    if (rows) *rows = R;
    return w.total;
}
// the checks both calls share, in the order of include/ctc_crf_hip.h, and the kernels' arguments; no HIP call.  dtype < 0: normalised fp32
static int rnnt_setup(const char *who_, const void *x, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                      int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, const void *out, const void *ws,
                      int64_t ws_bytes, RnntParams &p) {
    const std::string who = who_;
    if (!x || !labels || !lx || !ly || !out || !ws) { set_error(who + ": null argument"); return CRF_ERR_ARG; }
    if (dtype > 2) return bad_dtype(who_);
    SideWs w;
    int64_t R = 0;
    const int64_t need = rnnt_ws_bytes(N, T, U1, V, compact_rows, &w, &R);
    if (need < 0) return (int)-need;
    if (const int rc = check_blank(blank, V)) return rc;
    if (compact_rows >= 0 && (compact_labels < 0 || compact_labels > INT32_MAX)) { set_error(who + ": bad compact_labels"); return CRF_ERR_ARG; }
    if ((uintptr_t)ws & 15) { set_error(who + ": the workspace must be 16-byte aligned"); return CRF_ERR_ARG; }
    if (const int rc = check_ws(ws_bytes, need)) return rc;
    p = RnntParams{};
    p.x = x; p.labels = labels; p.lx = lx; p.ly = ly;
    p.N = (int)N; p.T = (int)T; p.U1 = (int)U1; p.V = (int)V; p.blank = blank; p.compact = compact_rows >= 0;
    p.R = R; p.nlab = compact_rows >= 0 ? compact_labels : N * (U1 - 1);
    char *b = (char *)ws;
    p.row = (float *)(b + w.sec[kRtRow].off); p.alpha = (double *)(b + w.sec[kRtAlpha].off); p.beta = (double *)(b + w.sec[kRtBeta].off);
    p.total = (double *)(b + w.sec[kRtUtt].off);
    p.node_off = (int *)(p.total + N); p.lab_off = p.node_off + N + 1; p.tn = p.lab_off + N; p.un = p.tn + N;
    return CRF_OK;
}
// the forward: offsets and validity, the row stage, both recursions -- three launches on one stream
static int rnnt_loss_call(const char *who, const void *x, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                          int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, float *cost, int32_t *invalid, void *ws,
                          int64_t ws_bytes, hipStream_t st) {
    RnntParams p;
    if (const int rc = rnnt_setup(who, x, dtype, blank, labels, lx, ly, N, T, U1, V, compact_rows, compact_labels, cost, ws, ws_bytes, p)) return rc;
    p.cost = cost; p.invalid = invalid;
    if (const int rc = launch<crf_rnnt_prep_kernel>("crf_rnnt_prep_kernel", dim3(1), dim3(kRnntPrepThreads), 0, st, p)) return rc;
    const dim3 wgrid((unsigned)((p.R + kRnntWaves - 1) / kRnntWaves)), wblock(64 * kRnntWaves);
    int rc;
    if (dtype < 0) rc = launch<crf_rnnt_gather_kernel>("crf_rnnt_gather_kernel", dim3((unsigned)((p.R + 255) / 256)), dim3(256), 0, st, p);
    else rc = with_dtype(dtype, [&](auto e) { return launch<crf_rnnt_row_kernel<decltype(e)>>("crf_rnnt_row_kernel", wgrid, wblock, 0, st, p); });
    if (rc) return rc;
    const dim3 lgrid((unsigned)N, 2);
    if (U1 <= 64) return launch<crf_rnnt_lattice_kernel<false>>("crf_rnnt_lattice_kernel<wave>", lgrid, dim3(64), 0, st, p);
    return launch<crf_rnnt_lattice_kernel<true>>("crf_rnnt_lattice_kernel<workgroup>", lgrid, dim3((unsigned)rup64((int)U1)), 0, st, p);
}
// the backward on the forward's workspace: one launch
static int rnnt_grad_call(const char *who, const void *x, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                          int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, const float *weight, void *grad, void *ws,
                          int64_t ws_bytes, hipStream_t st) {
    RnntParams p;
    if (!weight) { set_error(std::string(who) + ": null argument"); return CRF_ERR_ARG; }
    if (const int rc = rnnt_setup(who, x, dtype, blank, labels, lx, ly, N, T, U1, V, compact_rows, compact_labels, grad, ws, ws_bytes, p)) return rc;
    p.weight = weight; p.grad = grad;
    const dim3 wgrid((unsigned)((p.R + kRnntWaves - 1) / kRnntWaves)), wblock(64 * kRnntWaves);
    if (dtype < 0) return launch<crf_rnnt_grad_kernel<float, false>>("crf_rnnt_grad_kernel", wgrid, wblock, 0, st, p);
    return with_dtype(dtype, [&](auto e) { return launch<crf_rnnt_grad_kernel<decltype(e), true>>("crf_rnnt_grad_kernel", wgrid, wblock, 0, st, p); });
}

// ---- the RNN-T loss of a joiner that is a plain sum f + g (k_rnnt_join.hip) ----
// Its workspace: the padded one of crf_rnnt_loss, then df [N][T][V] and dg [kJoinSplit][N][U1][V] in fp32 -- nothing proportional to T U1 V.
enum JoinWs { kJnDf = kRtCount, kJnDg, kJnCount };
static const char *const kJoinWsNames[kJnCount] = {"row", "alpha", "beta", "utt", "df", "dg"};
static int64_t join_ws_bytes(int64_t N, int64_t T, int64_t U1, int64_t V, SideWs *out = nullptr) {
    SideWs w;
    const int64_t base = rnnt_ws_bytes(N, T, U1, V, -1, &w);
    if (base < 0) return base;
    w.add(kJoinWsNames[kJnDf], N * T * V * (int64_t)sizeof(float)).add(kJoinWsNames[kJnDg], kJoinSplit * N * U1 * V * (int64_t)sizeof(float));
    if (out) *out = w;
    return w.total;
}
// the checks both calls share, in the order of include/ctc_crf_hip.h, and the kernels' arguments; no HIP call
static int join_setup(const char *who_, const void *f, const void *g, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly,
                      int64_t N, int64_t T, int64_t U1, int64_t V, const void *out, const void *ws, int64_t ws_bytes, JoinParams &q) {
    const std::string who = who_;
    if (!f || !g || !labels || !lx || !ly || !out || !ws) { set_error(who + ": null argument"); return CRF_ERR_ARG; }
    if (dtype < 0 || dtype > 2) return bad_dtype(who_);
    SideWs w;
    const int64_t need = join_ws_bytes(N, T, U1, V, &w);
    if (need < 0) return (int)-need;
    if (const int rc = check_blank(blank, V)) return rc;
    if ((uintptr_t)ws & 15) { set_error(who + ": the workspace must be 16-byte aligned"); return CRF_ERR_ARG; }
    if (const int rc = check_ws(ws_bytes, need)) return rc;
    q = JoinParams{};
    RnntParams &p = q.r;
    p.labels = labels; p.lx = lx; p.ly = ly;
    p.N = (int)N; p.T = (int)T; p.U1 = (int)U1; p.V = (int)V; p.blank = blank; p.compact = 0;
    p.R = N * T * U1; p.nlab = N * (U1 - 1);
    char *b = (char *)ws;
    p.row = (float *)(b + w.sec[kRtRow].off); p.alpha = (double *)(b + w.sec[kRtAlpha].off); p.beta = (double *)(b + w.sec[kRtBeta].off);
    p.total = (double *)(b + w.sec[kRtUtt].off);
    p.node_off = (int *)(p.total + N); p.lab_off = p.node_off + N + 1; p.tn = p.lab_off + N; p.un = p.tn + N;
    q.f = f; q.g = g;
    q.df_part = (float *)(b + w.sec[kJnDf].off); q.dg_part = (float *)(b + w.sec[kJnDg].off);
    return CRF_OK;
}
// the forward: crf_rnnt_loss's prep and lattice launches around the join row stage
static int join_loss_call(const char *who, const void *f, const void *g, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly,
                          int64_t N, int64_t T, int64_t U1, int64_t V, float *cost, int32_t *invalid, void *ws, int64_t ws_bytes, hipStream_t st) {
    JoinParams q;
    if (const int rc = join_setup(who, f, g, dtype, blank, labels, lx, ly, N, T, U1, V, cost, ws, ws_bytes, q)) return rc;
    q.r.cost = cost; q.r.invalid = invalid;
    if (const int rc = launch<crf_rnnt_prep_kernel>("crf_rnnt_prep_kernel", dim3(1), dim3(kRnntPrepThreads), 0, st, q.r)) return rc;
    const dim3 rgrid((unsigned)(N * ((T + kJoinTT - 1) / kJoinTT)), (unsigned)((U1 + kJoinTU - 1) / kJoinTU));
    if (const int rc = with_dtype(dtype, [&](auto e) { return launch<crf_join_row_kernel<decltype(e)>>("crf_join_row_kernel", rgrid, dim3(kJoinRowThreads), 0, st, q); }))
        return rc;
    const dim3 lgrid((unsigned)N, 2);
    if (U1 <= 64) return launch<crf_rnnt_lattice_kernel<false>>("crf_rnnt_lattice_kernel<wave>", lgrid, dim3(64), 0, st, q.r);
    return launch<crf_rnnt_lattice_kernel<true>>("crf_rnnt_lattice_kernel<workgroup>", lgrid, dim3((unsigned)rup64((int)U1)), 0, st, q.r);
}
// the backward on the forward's workspace: the partial sums, then every element of the gradients asked for
static int join_grad_call(const char *who, const void *f, const void *g, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly,
                          int64_t N, int64_t T, int64_t U1, int64_t V, const float *weight, void *grad_f, void *grad_g, void *ws, int64_t ws_bytes,
                          hipStream_t st) {
    JoinParams q;
    if (!weight) { set_error(std::string(who) + ": null argument"); return CRF_ERR_ARG; }
    if (const int rc = join_setup(who, f, g, dtype, blank, labels, lx, ly, N, T, U1, V, weight, ws, ws_bytes, q)) return rc;
    if (!grad_f && !grad_g) return CRF_OK;
    q.r.weight = weight; q.grad_f = grad_f; q.grad_g = grad_g;
    const dim3 ggrid((unsigned)(N * ((V + kJoinGV - 1) / kJoinGV)), kJoinSplit), fgrid((unsigned)(N * std::max(T, U1)), 2);
    return with_dtype(dtype, [&](auto e) {
        if (const int rc = launch<crf_join_grad_kernel<decltype(e)>>("crf_join_grad_kernel", ggrid, dim3(kJoinGV), 0, st, q)) return rc;
        return launch<crf_join_fold_kernel<decltype(e)>>("crf_join_fold_kernel", fgrid, dim3(256), 0, st, q);
    });
}

// ---- the CTC-Transducer loss and its gradient (k_ctct.hip) ----
// The workspace both calls share, R = N T U1 (padded only): row [R][4] floats (b, r, e, log s), rmax [R] floats (M), alpha [R][2] and
// beta [R][2] fp64, utt as for crf_rnnt_loss.  < 0 with the message set.
enum CtctWs { kCtRow, kCtMax, kCtAlpha, kCtBeta, kCtUtt, kCtCount };
static const char *const kCtctWsNames[kCtCount] = {"row", "rmax", "alpha", "beta", "utt"};
static int64_t ctct_ws_bytes(int64_t N, int64_t T, int64_t U1, int64_t V, SideWs *out = nullptr) {
    const std::string who = "crf_ctct_loss: ";
    if (N <= 0 || T <= 0 || U1 <= 0 || V <= 0 || N > INT32_MAX || T > INT32_MAX) { set_error(who + "bad N/T/U+1/V"); return -CRF_ERR_ARG; }
    if (U1 > kRnntMaxU1) { set_error(who + "U > " + std::to_string(kRnntMaxU1 - 1) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (V > kRnntMaxV) { set_error(who + "V > " + std::to_string(kRnntMaxV) + " not supported by this build"); return -CRF_ERR_UNSUPPORTED; }
    if (T > (INT32_MAX / 4) / U1) { set_error(who + "T * (U + 1) > INT32_MAX / 4"); return -CRF_ERR_ARG; }   // (an utterance's nodes are indexed in 32 bits)
    if (N > INT32_MAX / (T * U1)) { set_error(who + "rows outside [1, INT32_MAX]"); return -CRF_ERR_ARG; }
    const int64_t R = N * T * U1;
    SideWs w;
    w.add(kCtctWsNames[kCtRow], 4 * R * (int64_t)sizeof(float)).add(kCtctWsNames[kCtMax], R * (int64_t)sizeof(float))
     .add(kCtctWsNames[kCtAlpha], 2 * R * (int64_t)sizeof(double)).add(kCtctWsNames[kCtBeta], 2 * R * (int64_t)sizeof(double))
     .add(kCtctWsNames[kCtUtt], N * (int64_t)sizeof(double) + (4 * N + 1) * (int64_t)sizeof(int32_t));
    if (out) *out = w;
    return w.total;
}
// the checks both calls share, in the order of include/ctc_crf_hip.h, and the kernels' arguments; no HIP call.  dtype < 0: normalised fp32
static int ctct_setup(const char *who_, const void *x, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                      int64_t T, int64_t U1, int64_t V, const void *out, const void *ws, int64_t ws_bytes, CtctParams &q) {
    const std::string who = who_;
    if (!x || !labels || !lx || !ly || !out || !ws) { set_error(who + ": null argument"); return CRF_ERR_ARG; }
    if (dtype > 2) return bad_dtype(who_);
    SideWs w;
    const int64_t need = ctct_ws_bytes(N, T, U1, V, &w);
    if (need < 0) return (int)-need;
    if (const int rc = check_blank(blank, V)) return rc;
    if ((uintptr_t)ws & 15) { set_error(who + ": the workspace must be 16-byte aligned"); return CRF_ERR_ARG; }
    if (const int rc = check_ws(ws_bytes, need)) return rc;
    q = CtctParams{};
    RnntParams &p = q.r;
    p.x = x; p.labels = labels; p.lx = lx; p.ly = ly;
    p.N = (int)N; p.T = (int)T; p.U1 = (int)U1; p.V = (int)V; p.blank = blank; p.compact = 0;
    p.R = N * T * U1; p.nlab = N * (U1 - 1);
    char *b = (char *)ws;
    p.row = (float *)(b + w.sec[kCtRow].off); q.rmax = (float *)(b + w.sec[kCtMax].off);
    p.alpha = (double *)(b + w.sec[kCtAlpha].off); p.beta = (double *)(b + w.sec[kCtBeta].off);
    p.total = (double *)(b + w.sec[kCtUtt].off);
    p.node_off = (int *)(p.total + N); p.lab_off = p.node_off + N + 1; p.tn = p.lab_off + N; p.un = p.tn + N;
    return CRF_OK;
}
// the forward: crf_rnnt_loss's prep launch, the row stage, both recursions -- three launches on one stream
static int ctct_loss_call(const char *who, const void *x, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                          int64_t T, int64_t U1, int64_t V, float *cost, int32_t *invalid, void *ws, int64_t ws_bytes, hipStream_t st) {
    CtctParams q;
    if (const int rc = ctct_setup(who, x, dtype, blank, labels, lx, ly, N, T, U1, V, cost, ws, ws_bytes, q)) return rc;
    q.r.cost = cost; q.r.invalid = invalid;
    if (const int rc = launch<crf_rnnt_prep_kernel>("crf_rnnt_prep_kernel", dim3(1), dim3(kRnntPrepThreads), 0, st, q.r)) return rc;
    const dim3 wgrid((unsigned)((q.r.R + kRnntWaves - 1) / kRnntWaves)), wblock(64 * kRnntWaves);
    int rc;
    if (dtype < 0) rc = launch<crf_ctct_gather_kernel>("crf_ctct_gather_kernel", dim3((unsigned)((q.r.R + 255) / 256)), dim3(256), 0, st, q);
    else rc = with_dtype(dtype, [&](auto e) { return launch<crf_ctct_row_kernel<decltype(e)>>("crf_ctct_row_kernel", wgrid, wblock, 0, st, q); });
    if (rc) return rc;
    const dim3 lgrid((unsigned)N, 2);
    if (U1 <= 64) return launch<crf_ctct_lattice_kernel<false>>("crf_ctct_lattice_kernel<wave>", lgrid, dim3(64), 0, st, q);
    return launch<crf_ctct_lattice_kernel<true>>("crf_ctct_lattice_kernel<workgroup>", lgrid, dim3((unsigned)rup64((int)U1)), 0, st, q);
}
// the backward on the forward's workspace: one launch
static int ctct_grad_call(const char *who, const void *x, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                          int64_t T, int64_t U1, int64_t V, const float *weight, void *grad, void *ws, int64_t ws_bytes, hipStream_t st) {
    CtctParams q;
    if (!weight) { set_error(std::string(who) + ": null argument"); return CRF_ERR_ARG; }
    if (const int rc = ctct_setup(who, x, dtype, blank, labels, lx, ly, N, T, U1, V, grad, ws, ws_bytes, q)) return rc;
    q.r.weight = weight; q.r.grad = grad;
    const dim3 wgrid((unsigned)((q.r.R + kRnntWaves - 1) / kRnntWaves)), wblock(64 * kRnntWaves);
    if (dtype < 0) return launch<crf_ctct_grad_kernel<float, false>>("crf_ctct_grad_kernel", wgrid, wblock, 0, st, q);
    return with_dtype(dtype, [&](auto e) { return launch<crf_ctct_grad_kernel<decltype(e), true>>("crf_ctct_grad_kernel", wgrid, wblock, 0, st, q); });
}

}  // namespace crf

using namespace crf;

static int64_t or_minus1(int64_t n) { return n < 0 ? -1 : n; }   // the *_workspace_bytes exports: -1 with the message set

extern "C" {

int64_t crf_ctc_align_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t max_label_len) { return or_minus1(align_ws_bytes(B, T, V, max_label_len)); }
int64_t crf_ctc_align_logits_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t max_label_len) { return or_minus1(align_ws_bytes(B, T, V, max_label_len, true)); }
int crf_debug_align_ws_sections(int logits, int64_t B, int64_t T, int64_t V, int64_t max_label_len, int64_t *out, int n_out) {
    SideWs w;
    if (align_ws_bytes(B, T, V, max_label_len, logits != 0, &w) < 0) return -1;
    return copy_sections(w.sec, w.nsec, out, n_out);
}
const char *crf_debug_align_ws_section_names(void) {
    static const std::string s = join_names(kAlignWsNames, 2);
    return s.c_str();
}

int crf_ctc_align(const float *act, int time_major, int blank, const int32_t *labels, const int32_t *lab_off, const int32_t *lx,
                  const int32_t *ly, int64_t B, int64_t T, int64_t V, int64_t max_label_len, int32_t *pos, float *score,
                  int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    return align_call("crf_ctc_align", act, -1, time_major, blank, labels, lab_off, lx, ly, B, T, V, max_label_len, pos, score, invalid, ws, ws_bytes,
                      (hipStream_t)stream_);
}

int crf_ctc_align_logits(const void *act, int dtype, int time_major, int blank, const int32_t *labels, const int32_t *lab_off,
                         const int32_t *lx, const int32_t *ly, int64_t B, int64_t T, int64_t V, int64_t max_label_len, int32_t *pos,
                         float *score, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    if (dtype < 0) return bad_dtype("crf_ctc_align_logits");
    return align_call("crf_ctc_align_logits", act, dtype, time_major, blank, labels, lab_off, lx, ly, B, T, V, max_label_len, pos, score, invalid, ws,
                      ws_bytes, (hipStream_t)stream_);
}

int crf_ctc_score(const float *act, int time_major, int blank, const int32_t *labels, const int32_t *hyp_off, const int32_t *hyp_len,
                  const int32_t *hyp_utt, const int32_t *lx, int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len,
                  float *score, int32_t *invalid, void *stream_) {
    return score_call("crf_ctc_score", act, -1, time_major, blank, labels, hyp_off, hyp_len, hyp_utt, lx, B, H, T, V, max_hyp_len, score, invalid, nullptr,
                      0, (hipStream_t)stream_);
}

int64_t crf_ctc_score_logits_workspace_bytes(int64_t B, int64_t T, int64_t V) { return or_minus1(score_ws_bytes(B, T, V)); }

int crf_ctc_score_logits(const void *act, int dtype, int time_major, int blank, const int32_t *labels, const int32_t *hyp_off,
                         const int32_t *hyp_len, const int32_t *hyp_utt, const int32_t *lx, int64_t B, int64_t H, int64_t T, int64_t V,
                         int64_t max_hyp_len, float *score, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    if (dtype < 0) return bad_dtype("crf_ctc_score_logits");
    return score_call("crf_ctc_score_logits", act, dtype, time_major, blank, labels, hyp_off, hyp_len, hyp_utt, lx, B, H, T, V, max_hyp_len, score,
                      invalid, ws, ws_bytes, (hipStream_t)stream_);
}

int64_t crf_ctc_score_grad_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len) {
    return or_minus1(score_grad_ws_bytes(B, H, T, V, max_hyp_len));
}

int crf_ctc_score_grad(const float *act, int time_major, int blank, const int32_t *labels, const int32_t *hyp_off, const int32_t *hyp_len,
                       const int32_t *hyp_utt, const int32_t *lx, const float *weight, int64_t B, int64_t H, int64_t T, int64_t V,
                       int64_t max_hyp_len, float *score, int32_t *invalid, float *grad, void *ws, int64_t ws_bytes, void *stream_) {
    return score_grad_call("crf_ctc_score_grad", act, -1, time_major, blank, labels, hyp_off, hyp_len, hyp_utt, lx, weight, B, H, T, V, max_hyp_len,
                           score, invalid, grad, ws, ws_bytes, (hipStream_t)stream_);
}

int64_t crf_ctc_score_grad_logits_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t max_hyp_len) {
    return or_minus1(score_grad_ws_bytes(B, H, T, V, max_hyp_len, true));
}

int crf_ctc_score_grad_logits(const void *act, int dtype, int time_major, int blank, const int32_t *labels, const int32_t *hyp_off,
                              const int32_t *hyp_len, const int32_t *hyp_utt, const int32_t *lx, const float *weight, int64_t B, int64_t H,
                              int64_t T, int64_t V, int64_t max_hyp_len, float *score, int32_t *invalid, float *grad, void *ws,
                              int64_t ws_bytes, void *stream_) {
    if (dtype < 0) return bad_dtype("crf_ctc_score_grad_logits");
    return score_grad_call("crf_ctc_score_grad_logits", act, dtype, time_major, blank, labels, hyp_off, hyp_len, hyp_utt, lx, weight, B, H, T, V,
                           max_hyp_len, score, invalid, grad, ws, ws_bytes, (hipStream_t)stream_);
}

int64_t crf_ctc_score_rows_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, int dtype) {
    return or_minus1(rows_ws_bytes(false, B, H, T, V, len_cap, dtype));
}

int crf_ctc_score_rows(const void *act, int dtype, int time_major, int blank, const int32_t *hyps, int64_t hyp_stride, const int32_t *hyp_len,
                       const int32_t *hyp_utt, const int32_t *lx, int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, float *score,
                       int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    return score_rows_call(act, dtype, time_major, blank, hyps, hyp_stride, hyp_len, hyp_utt, lx, B, H, T, V, len_cap, score, invalid, ws, ws_bytes,
                           (hipStream_t)stream_);
}

int64_t crf_ctc_score_grad_rows_workspace_bytes(int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, int dtype) {
    return or_minus1(rows_ws_bytes(true, B, H, T, V, len_cap, dtype));
}

int crf_ctc_score_grad_rows(const void *act, int dtype, int time_major, int blank, const int32_t *hyps, int64_t hyp_stride,
                            const int32_t *hyp_len, const int32_t *hyp_utt, const int32_t *lx, const float *weight, int64_t B, int64_t H,
                            int64_t T, int64_t V, int64_t len_cap, float *score, int32_t *invalid, float *grad, void *ws, int64_t ws_bytes,
                            void *stream_) {
    return score_grad_rows_call(act, dtype, time_major, blank, hyps, hyp_stride, hyp_len, hyp_utt, lx, weight, B, H, T, V, len_cap, score, invalid,
                                grad, ws, ws_bytes, (hipStream_t)stream_);
}

int crf_debug_score_rows_ws_sections(int grad, int64_t B, int64_t H, int64_t T, int64_t V, int64_t len_cap, int dtype, int64_t *out, int n_out) {
    SideWs w;
    if (rows_ws_bytes(grad != 0, B, H, T, V, len_cap, dtype, &w) < 0) return -1;
    return copy_sections(w.sec, w.nsec, out, n_out);
}
const char *crf_debug_score_rows_ws_section_names(int grad) {
    static const std::string s[2] = {join_names(kRowsWsNames + kRwOff, kRwCount - kRwOff), join_names(kRowsWsNames, kRwCount)};
    return s[grad != 0].c_str();
}

int64_t crf_ctc_sample_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t K) { return or_minus1(sample_ws_bytes(B, T, V, K)); }

int crf_ctc_sample(const void *act, int dtype, int time_major, int blank, const int32_t *lx, int64_t B, int64_t T, int64_t V, int64_t K,
                   uint64_t seed, uint32_t offset, int greedy, int32_t *hyps, int32_t *hyp_len, int32_t *paths, void *ws, int64_t ws_bytes,
                   void *stream_) {
    if (!act || !lx || !hyps || !hyp_len || !ws) { set_error("crf_ctc_sample: null argument"); return CRF_ERR_ARG; }
    if (dtype < 0 || dtype > 2) return bad_dtype("crf_ctc_sample");
    const int64_t need = sample_ws_bytes(B, T, V, K);
    if (need < 0) return (int)-need;
    if (const int rc = check_blank(blank, V)) return rc;
    if (greedy && K != 1) { set_error("crf_ctc_sample: greedy takes K = 1, got " + std::to_string(K)); return CRF_ERR_ARG; }
    if (const int rc = check_ws(ws_bytes, need)) return rc;
    SampleParams p{};
    set_act(p, act, lx, B, T, V, blank, time_major);
    p.K = (int)K;
    p.seed_lo = (unsigned)(seed & 0xffffffffu); p.seed_hi = (unsigned)(seed >> 32); p.offset = offset;
    p.cls = (int *)ws; p.hyps = hyps; p.hyp_len = hyp_len; p.paths = paths;
    return with_dtype(dtype, [&](auto e) { return launch_sample<decltype(e)>(p, (hipStream_t)stream_, greedy != 0); });
}

int64_t crf_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t W, int64_t top_classes) {
    return or_minus1(beam_ws_bytes(B, T, V, W, top_classes));
}

int crf_ctc_beam(const void *act, int dtype, int time_major, int blank, int normalize, const int32_t *lx, int64_t B, int64_t T, int64_t V,
                 int64_t W, int64_t nbest, int64_t top_classes, int32_t *hyps, int32_t *hyp_len, float *score, int32_t *trace, void *ws,
                 int64_t ws_bytes, void *stream_) {
    return beam_call("crf_ctc_beam", act, dtype, time_major, blank, normalize, lx, B, T, V, W, nbest, top_classes, nullptr, false, 0.f, 0.f, hyps,
                     hyp_len, score, nullptr, trace, ws, ws_bytes, (hipStream_t)stream_);
}

int64_t crf_ctc_beam_lm_workspace_bytes(int64_t B, int64_t T, int64_t V, int64_t W, int64_t top_classes) {
    return or_minus1(beam_ws_bytes(B, T, V, W, top_classes));
}

int crf_ctc_beam_lm(const void *act, int dtype, int time_major, int blank, int normalize, const int32_t *lx, int64_t B, int64_t T, int64_t V,
                    int64_t W, int64_t nbest, int64_t top_classes, const crf_ngram_tables *lm, float alpha, float beta, int32_t *hyps,
                    int32_t *hyp_len, float *score, float *lm_score, int32_t *trace, void *ws, int64_t ws_bytes, void *stream_) {
    return beam_call("crf_ctc_beam_lm", act, dtype, time_major, blank, normalize, lx, B, T, V, W, nbest, top_classes, lm, true, alpha, beta, hyps,
                     hyp_len, score, lm_score, trace, ws, ws_bytes, (hipStream_t)stream_);
}

int64_t crf_ctc_beam_state_record_bytes(int64_t W, int64_t cap) {
    if (W < 1 || W > kBeamMaxW) { set_error("crf_ctc_beam_chunk: beam width " + std::to_string(W) + " outside [1, " + std::to_string(kBeamMaxW) + "]"); return -1; }
    if (cap < 1 || cap > kBeamStateMaxCap) { set_error("crf_ctc_beam_chunk: cap " + std::to_string(cap) + " outside [1, " + std::to_string(kBeamStateMaxCap) + "]"); return -1; }
    return beam_state_bytes(W, cap);
}

int64_t crf_ctc_beam_chunk_workspace_bytes(int64_t B, int64_t Tc, int64_t V, int64_t W, int64_t top_classes) {
    return or_minus1(beam_ws_bytes(B, Tc, V, W, top_classes));
}

int crf_ctc_beam_chunk(const void *act, int dtype, int time_major, int blank, int normalize, const int32_t *lx_chunk, int64_t B, int64_t Tc,
                       int64_t V, int64_t W, int64_t nbest, int64_t top_classes, const crf_ngram_tables *lm, float alpha, float beta,
                       const void *state_in, const int32_t *reset, void *state_out, int64_t cap, int32_t *hyps, int32_t *hyp_len, float *score,
                       float *lm_score, int32_t *trace, void *ws, int64_t ws_bytes, void *stream_) {
    const char *who = "crf_ctc_beam_chunk";
    const std::string w0 = std::string(who) + ": ";
    if (!state_out) { set_error(w0 + "null argument (state_out_dev)"); return CRF_ERR_ARG; }
    BeamChunkParams cp{};
    if (const int rc = beam_setup(who, act, dtype, time_major, blank, normalize, lx_chunk, B, Tc, V, W, nbest, top_classes, lm, lm != nullptr,
                                  lm ? alpha : 0.f, lm ? beta : 0.f, hyps, hyp_len, score, lm_score, trace, ws, ws_bytes, cp.q)) return rc;
    if (cap < 1 || cap > kBeamStateMaxCap) {
        set_error(w0 + "cap " + std::to_string(cap) + " outside [1, " + std::to_string(kBeamStateMaxCap) + "]"); return CRF_ERR_ARG;
    }
    const int64_t rec = beam_state_bytes(W, cap);
    if (state_in) {
        const uintptr_t a = (uintptr_t)state_in, o = (uintptr_t)state_out, n = (uintptr_t)(B * rec);
        if (a < o + n && o < a + n) { set_error(w0 + "state_out_dev overlaps state_in_dev (label rows move between slots)"); return CRF_ERR_ARG; }
    }
    if (((uintptr_t)state_out | (uintptr_t)state_in) & 7) { set_error(w0 + "the states must be 8-byte aligned"); return CRF_ERR_ARG; }
    cp.state_in = (const char *)state_in; cp.reset = reset; cp.state_out = (char *)state_out; cp.cap = (int)cap; cp.rec = rec;
    const bool with_lm = lm != nullptr;
    return with_dtype(dtype, [&](auto e) { return launch_beam_chunk<decltype(e)>(cp, with_lm, (hipStream_t)stream_); });
}

// HOST copies of the tables, no HIP call: the first offending entry by name
int crf_ngram_tables_check(const crf_ngram_tables *t) {
    const std::string who = "crf_ngram_tables_check: ";
    auto bad = [&](const std::string &m) { set_error(who + m); return CRF_ERR_ARG; };
    auto str = [](int64_t v) { return std::to_string(v); };
    if (!t) return bad("null argument");
    if (t->order < 1 || t->order > kNgramMaxOrder) return bad("order " + str(t->order) + " outside [1, " + str(kNgramMaxOrder) + "]");
    if (t->V < 1 || t->V > kBeamMaxV) return bad("V " + str(t->V) + " outside [1, " + str(kBeamMaxV) + "]");
    if (t->S < 1 || t->S > INT32_MAX) return bad("S " + str(t->S) + " outside [1, INT32_MAX]");
    if (t->A < 0 || t->A > INT32_MAX) return bad("A " + str(t->A) + " outside [0, INT32_MAX]");
    if (t->start < 0 || t->start >= t->S) return bad("start " + str(t->start) + " outside [0, S=" + str(t->S) + ")");
    if (!t->row_off || !t->bo_state || !t->bo_weight || !t->uni_logp || !t->uni_next || (t->A > 0 && (!t->arc_label || !t->arc_logp || !t->arc_next)))
        return bad("null table");
    const int64_t S = t->S, A = t->A, V = t->V;
    if (t->row_off[0] != 0) return bad("row_off[0] = " + str(t->row_off[0]) + " is not 0");
    for (int64_t s = 0; s < S; ++s)
        if (t->row_off[s + 1] < t->row_off[s]) return bad("row_off[" + str(s + 1) + "] = " + str(t->row_off[s + 1]) + " is below row_off[" + str(s) + "] = " + str(t->row_off[s]));
    if (t->row_off[S] != A) return bad("row_off[" + str(S) + "] = " + str(t->row_off[S]) + " is not A = " + str(A));
    if (t->row_off[1] != 0) return bad("row_off[1] = " + str(t->row_off[1]) + ": the root's row is the dense one, its sparse row is empty");
    for (int64_t s = 0; s < S; ++s) {
        if (t->row_off[s + 1] - t->row_off[s] > V) return bad("row " + str(s) + " holds " + str(t->row_off[s + 1] - t->row_off[s]) + " arcs, more than V = " + str(V));
        for (int64_t i = t->row_off[s]; i < t->row_off[s + 1]; ++i) {
            if (t->arc_label[i] < 0 || t->arc_label[i] >= V) return bad("arc_label[" + str(i) + "] = " + str(t->arc_label[i]) + " outside [0, V=" + str(V) + ")");
            if (i > t->row_off[s] && t->arc_label[i] <= t->arc_label[i - 1])
                return bad("arc_label[" + str(i) + "] = " + str(t->arc_label[i]) + " does not ascend in row " + str(s) + " (arc_label[" + str(i - 1) + "] = " + str(t->arc_label[i - 1]) + ")");
            if (t->arc_next[i] < 0 || t->arc_next[i] >= S) return bad("arc_next[" + str(i) + "] = " + str(t->arc_next[i]) + " outside [0, S=" + str(S) + ")");
            if (!std::isfinite(t->arc_logp[i])) return bad("arc_logp[" + str(i) + "] is not finite");
        }
    }
    for (int64_t s = 0; s < S; ++s) {
        if (t->bo_state[s] < 0 || (s > 0 ? t->bo_state[s] >= s : t->bo_state[s] != 0))
            return bad("bo_state[" + str(s) + "] = " + str(t->bo_state[s]) + " is not below its state (the root's is 0)");
        if (!std::isfinite(t->bo_weight[s])) return bad("bo_weight[" + str(s) + "] is not finite");
    }
    for (int64_t c = 0; c < V; ++c) {
        if (t->uni_next[c] < 0 || t->uni_next[c] >= S) return bad("uni_next[" + str(c) + "] = " + str(t->uni_next[c]) + " outside [0, S=" + str(S) + ")");
        if (!std::isfinite(t->uni_logp[c])) return bad("uni_logp[" + str(c) + "] is not finite");
    }
    return CRF_OK;
}

int crf_ctc_edit_distance(const int32_t *hyps, int64_t hyp_stride, const int32_t *hyp_len, const int32_t *hyp_utt, const int32_t *refs,
                          const int32_t *ref_off, const int32_t *ref_len, int64_t B, int64_t H, int64_t max_ref_len, int32_t *dist,
                          int32_t *ops, void *stream_) {
    const char *who = "crf_ctc_edit_distance";
    if (!hyps || !hyp_len || !hyp_utt || !refs || !ref_off || !ref_len || !dist) { set_error(std::string(who) + ": null argument"); return CRF_ERR_ARG; }
    if (B <= 0 || B > INT32_MAX || H <= 0 || H > INT32_MAX || hyp_stride <= 0 || hyp_stride > INT32_MAX || max_ref_len < 0) {
        set_error(std::string(who) + ": bad B/H/hyp_stride/max_ref_len"); return CRF_ERR_ARG;
    }
    if (H * hyp_stride > INT32_MAX) { set_error(std::string(who) + ": H * hyp_stride > INT32_MAX"); return CRF_ERR_ARG; }
    if (max_ref_len > kMaxCtcLabelLen) { set_error("reference length > " + std::to_string(kMaxCtcLabelLen) + " not supported by this build"); return CRF_ERR_UNSUPPORTED; }
    if (max_ref_len > kEditStripRows && hyp_stride > kEditStripMaxCols) {
        set_error(std::string(who) + ": hyp_stride " + std::to_string(hyp_stride) + " > " + std::to_string(kEditStripMaxCols) + " with references of more than " +
                  std::to_string(kEditStripRows) + " tokens not supported by this build");
        return CRF_ERR_UNSUPPORTED;
    }
    EditParams p{};
    p.hyps = hyps; p.hyp_len = hyp_len; p.hyp_utt = hyp_utt; p.refs = refs; p.ref_off = ref_off; p.ref_len = ref_len;
    p.B = (int)B; p.H = (int)H; p.stride = (int)hyp_stride; p.max_ref = (int)max_ref_len;
    p.dist = dist; p.ops = ops;
    return launch_edit(p, (hipStream_t)stream_);
}

int crf_ngram_score(const crf_ngram_tables *lm, const float *eos_logp, const int32_t *hyps, int64_t hyp_stride, const int32_t *hyp_len,
                    int64_t H, int use_start, int add_eos, float *score, int32_t *invalid, float *token_logp, int32_t *token_order,
                    void *stream_) {
    const std::string w0 = "crf_ngram_score: ";
    auto bad = [&](const std::string &m) { set_error(w0 + m); return CRF_ERR_ARG; };
    auto str = [](int64_t v) { return std::to_string(v); };
    if (!lm || !hyps || !hyp_len || !score) return bad("null argument");
    if (lm->S < 1 || lm->S > INT32_MAX || lm->A < 0 || lm->A > INT32_MAX || lm->order < 1 || lm->order > kNgramMaxOrder || lm->start < 0 ||
        lm->start >= lm->S || lm->V < 1 || lm->V > kBeamMaxV)
        return bad("bad LM tables: S " + str(lm->S) + ", A " + str(lm->A) + ", V " + str(lm->V) + ", order " + str(lm->order) + ", start " + str(lm->start));
    if (!lm->row_off || !lm->bo_state || !lm->bo_weight || !lm->uni_logp || !lm->uni_next ||
        (lm->A > 0 && (!lm->arc_label || !lm->arc_logp || !lm->arc_next))) return bad("null LM table");
    if (H < 0) return bad("H " + str(H) + " is negative");
    if (hyp_stride < 1 || hyp_stride > kNgramMaxStride) return bad("hyp_stride " + str(hyp_stride) + " outside [1, " + str(kNgramMaxStride) + "]");
    if (add_eos && !eos_logp) return bad("add_eos needs eos_logp_dev (a model without a </s> unigram has none)");
    if (H == 0) return CRF_OK;
    if ((H + kNgramScoreWaves - 1) / kNgramScoreWaves > INT32_MAX) return bad("H " + str(H) + " exceeds the grid");
    NgramScoreParams p{};
    p.lm.row_off = lm->row_off; p.lm.arc_label = lm->arc_label; p.lm.arc_logp = lm->arc_logp; p.lm.arc_next = lm->arc_next;
    p.lm.bo_state = lm->bo_state; p.lm.bo_weight = lm->bo_weight; p.lm.uni_logp = lm->uni_logp; p.lm.uni_next = lm->uni_next;
    p.lm.S = (int)lm->S; p.lm.A = (int)lm->A; p.lm.V = (int)lm->V; p.lm.order = lm->order; p.lm.start = lm->start;
    p.eos = eos_logp; p.hyps = hyps; p.hyp_len = hyp_len; p.H = H; p.stride = (int)hyp_stride;
    p.use_start = use_start != 0; p.add_eos = add_eos != 0;
    p.score = score; p.invalid = invalid; p.tok_logp = token_logp; p.tok_order = token_order;
    return launch_ngram_score(p, (hipStream_t)stream_);
}

int64_t crf_rnnt_workspace_bytes(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t compact_rows) {
    return or_minus1(rnnt_ws_bytes(N, T, U1, V, compact_rows));
}
int crf_debug_rnnt_ws_sections(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t compact_rows, int64_t *out, int n_out) {
    SideWs w;
    if (rnnt_ws_bytes(N, T, U1, V, compact_rows, &w) < 0) return -1;
    return copy_sections(w.sec, w.nsec, out, n_out);
}
const char *crf_debug_rnnt_ws_section_names(void) {
    static const std::string s = join_names(kRnntWsNames, kRtCount);
    return s.c_str();
}

int crf_rnnt_loss(const float *log_probs, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T, int64_t U1,
                  int64_t V, int64_t compact_rows, int64_t compact_labels, float *cost, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    return rnnt_loss_call("crf_rnnt_loss", log_probs, -1, blank, labels, lx, ly, N, T, U1, V, compact_rows, compact_labels, cost, invalid, ws, ws_bytes,
                          (hipStream_t)stream_);
}
int crf_rnnt_loss_logits(const void *logits, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T,
                         int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, float *cost, int32_t *invalid, void *ws, int64_t ws_bytes,
                         void *stream_) {
    if (dtype < 0) return bad_dtype("crf_rnnt_loss_logits");
    return rnnt_loss_call("crf_rnnt_loss_logits", logits, dtype, blank, labels, lx, ly, N, T, U1, V, compact_rows, compact_labels, cost, invalid, ws,
                          ws_bytes, (hipStream_t)stream_);
}
int crf_rnnt_grad(const float *log_probs, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T, int64_t U1,
                  int64_t V, int64_t compact_rows, int64_t compact_labels, const float *grad_output, float *grad, void *ws, int64_t ws_bytes,
                  void *stream_) {
    return rnnt_grad_call("crf_rnnt_grad", log_probs, -1, blank, labels, lx, ly, N, T, U1, V, compact_rows, compact_labels, grad_output, grad, ws,
                          ws_bytes, (hipStream_t)stream_);
}
int crf_rnnt_grad_logits(const void *logits, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T,
                         int64_t U1, int64_t V, int64_t compact_rows, int64_t compact_labels, const float *grad_output, void *grad, void *ws,
                         int64_t ws_bytes, void *stream_) {
    if (dtype < 0) return bad_dtype("crf_rnnt_grad_logits");
    return rnnt_grad_call("crf_rnnt_grad_logits", logits, dtype, blank, labels, lx, ly, N, T, U1, V, compact_rows, compact_labels, grad_output, grad, ws,
                          ws_bytes, (hipStream_t)stream_);
}

int64_t crf_rnnt_simple_workspace_bytes(int64_t N, int64_t T, int64_t U1, int64_t V) { return or_minus1(join_ws_bytes(N, T, U1, V)); }
int crf_debug_rnnt_simple_ws_sections(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t *out, int n_out) {
    SideWs w;
    if (join_ws_bytes(N, T, U1, V, &w) < 0) return -1;
    return copy_sections(w.sec, w.nsec, out, n_out);
}
const char *crf_debug_rnnt_simple_ws_section_names(void) {
    static const std::string s = join_names(kJoinWsNames, kJnCount);
    return s.c_str();
}
int crf_rnnt_simple_loss(const void *f, const void *g, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                         int64_t T, int64_t U1, int64_t V, float *cost, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    return join_loss_call("crf_rnnt_simple_loss", f, g, dtype, blank, labels, lx, ly, N, T, U1, V, cost, invalid, ws, ws_bytes, (hipStream_t)stream_);
}
int crf_rnnt_simple_grad(const void *f, const void *g, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N,
                         int64_t T, int64_t U1, int64_t V, const float *grad_output, void *grad_f, void *grad_g, void *ws, int64_t ws_bytes,
                         void *stream_) {
    return join_grad_call("crf_rnnt_simple_grad", f, g, dtype, blank, labels, lx, ly, N, T, U1, V, grad_output, grad_f, grad_g, ws, ws_bytes,
                          (hipStream_t)stream_);
}

int64_t crf_ctct_workspace_bytes(int64_t N, int64_t T, int64_t U1, int64_t V) { return or_minus1(ctct_ws_bytes(N, T, U1, V)); }
int crf_debug_ctct_ws_sections(int64_t N, int64_t T, int64_t U1, int64_t V, int64_t *out, int n_out) {
    SideWs w;
    if (ctct_ws_bytes(N, T, U1, V, &w) < 0) return -1;
    return copy_sections(w.sec, w.nsec, out, n_out);
}
const char *crf_debug_ctct_ws_section_names(void) {
    static const std::string s = join_names(kCtctWsNames, kCtCount);
    return s.c_str();
}
int crf_ctct_loss(const float *log_probs, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T, int64_t U1,
                  int64_t V, float *cost, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    return ctct_loss_call("crf_ctct_loss", log_probs, -1, blank, labels, lx, ly, N, T, U1, V, cost, invalid, ws, ws_bytes, (hipStream_t)stream_);
}
int crf_ctct_loss_logits(const void *logits, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T,
                         int64_t U1, int64_t V, float *cost, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    if (dtype < 0) return bad_dtype("crf_ctct_loss_logits");
    return ctct_loss_call("crf_ctct_loss_logits", logits, dtype, blank, labels, lx, ly, N, T, U1, V, cost, invalid, ws, ws_bytes, (hipStream_t)stream_);
}
int crf_ctct_grad(const float *log_probs, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T, int64_t U1,
                  int64_t V, const float *grad_output, float *grad, void *ws, int64_t ws_bytes, void *stream_) {
    return ctct_grad_call("crf_ctct_grad", log_probs, -1, blank, labels, lx, ly, N, T, U1, V, grad_output, grad, ws, ws_bytes, (hipStream_t)stream_);
}
int crf_ctct_grad_logits(const void *logits, int dtype, int blank, const int32_t *labels, const int32_t *lx, const int32_t *ly, int64_t N, int64_t T,
                         int64_t U1, int64_t V, const float *grad_output, void *grad, void *ws, int64_t ws_bytes, void *stream_) {
    if (dtype < 0) return bad_dtype("crf_ctct_grad_logits");
    return ctct_grad_call("crf_ctct_grad_logits", logits, dtype, blank, labels, lx, ly, N, T, U1, V, grad_output, grad, ws, ws_bytes,
                          (hipStream_t)stream_);
}

const char *crf_last_ngram_score_kernel(void) { return g_ngram_kernel; }
const char *crf_last_edit_kernel(void) { return g_edit_kernel; }
const char *crf_last_beam_kernel(void) { return g_beam_kernel; }
const char *crf_last_score_kernel(void) { return g_score_kernel; }
const char *crf_last_score_grad_kernel(void) { return g_score_grad_kernel; }
const char *crf_last_sample_kernel(void) { return g_sample_kernel; }

}  // extern "C"
