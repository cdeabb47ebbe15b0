// cat_amd/csrc/crf_host.hip -- the host side of the CTC-CRF loss, in the order of a call: the denominator kernel family is chosen once
// (DenFamily, choose_den_family), the workspace is laid down for it as a list of sections (ws_layout; the arrays inside the sections pb,
// xch and bsm come from one field list each), the kernels and the schedule are planned as data (CallPlan; the stage plan itself is host C++
// in stage_plan.cpp), the sections and fields are bound to the kernels' parameter blocks by name (bind_params), and a LossCall enqueues one
// of four stream schedules; then the C-ABI entry points of include/ctc_crf_hip.h.  (Forced alignment, hypothesis scores and sampling share
// nothing with the loss call: crf_host_ctc.hip; what both host units use -- section and field records, launch<>, with_nr -- is
// crf_host_util.h.)  The kernels live in one translation unit per family (cat_amd/build.py compiles them in parallel):
//   k_chain.hip      prep (e' = exp(logp - rowmax) * 2^64), metadata staging, streaming denominator chains, numerator (CTC) chains in fp64
//   k_fac_*.hip      register-resident denominator recursions on the factored layout of T o LM graphs (k_fac_body.h): the dominant kernels
//   k_res.hip        register-resident recursions, generic layout over K compute units
//   k_batch.hip      utterance-minor kernels for graphs beyond the registers (one launch per frame, or one persistent launch)
//   k_grad.hip       the grad pass (label posteriors from the stored rows; numerator half; fused combine)
//   k_robust.hip     log-domain fallbacks, forward/backward consistency check, finalize
// What is computed (semantics of the reference):
//   denominator  den_calculate.cu:63-261   alpha/beta over the den graph, logZ, arc posteriors -> labels
//   numerator    gpu_ctc_kernels.h:87-458  CTC alpha/beta on log-probs (blank 0), label posteriors
//   combine      ctc_crf/__init__.py:78-87 grad = c_den*gamma_den - c_ctc*gamma_ctc, loss likewise
// How: linear domain with an exact per-frame power-of-two rescale instead of per-arc log1p(exp()) (den_calculate.cu:29-35);
// the den graph factored through "pairs" p = (destination state, label):
//     forward   q_t[p] = sum_{arcs k in p} a_t[src_k] * w_k,   a_{t+1}[dst_p] = e_t[lab_p] * q_t[p]
//     backward  b_t[s] = sum_{arcs k out of s} w_k * z_t[pair_k],   z_t[p] = e_t[lab_p] * b_{t+1}[dst_p]
//     posterior gamma_den[t][v] = e_t[v] * sum_{p: lab_p = v} q_t[p] * b_{t+1}[dst_p] / Z     (no arc pass: two stored rows per frame)
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/ctc_crf_hip.h"
#include "crf_internal.h"

#include "crf_device.h"
#include "crf_kernels_decl.h"
#include "crf_host_util.h"
#include "stage_plan.h"

namespace crf {

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The workspace is a list of sections, every one laid down by WsLayout::add: name, offset and byte count are recorded in layout order, and
// every pointer of the kernels' parameter blocks is carved from those records (WsLayout::off), so the map crf_debug_ws_sections shows
// cannot drift from the layout the kernels use.  The enumerators, the names and the order all come from this one list.
#define CRF_WS_SECTIONS(X) \
    X(ep) X(mx) X(moff) X(invs) X(Q) X(BP) X(EQ) X(EB) X(CA) X(CB) X(ECA) X(ECB) X(pb) X(cbad) X(xch) X(row0) X(ept) X(Af) X(Zb) X(bsm) X(gvec) X(state) X(dump)
enum WsSec : int {
#define CRF_WS_ENUM(name) kWs_##name,
    CRF_WS_SECTIONS(CRF_WS_ENUM)
#undef CRF_WS_ENUM
    kWsCount
};
static const char *const kWsNames[kWsCount] = {
#define CRF_WS_NAME(name) #name,
    CRF_WS_SECTIONS(CRF_WS_NAME)
#undef CRF_WS_NAME
};
struct WsLayout {
    WsSection sec[kWsCount];     // in layout order: sec[k] is section k of CRF_WS_SECTIONS
    int nsec;
    int64_t total;               // = the running end of the layout while it is being made
    int64_t gap;
    int64_t xch_bytes;           // the exchange granules in front of the flag words of section xch
    int64_t state_stride, gvec_stride, dump_stride;
    // the next section: starts at the running end, which then moves past its bytes to the next multiple of 256 (+ the ws_gap bytes)
    void add(WsSec k, int64_t bytes) {
        if (k != nsec) abort();   // (the sections are laid down in the order of the list)
        sec[nsec++] = WsSection{kWsNames[k], total, bytes};
        total = al(total + bytes) + gap;
    }
    int64_t off(WsSec k) const { return sec[k].off; }
};

// The arrays inside three of the sections, X(name, element bytes, a, c): a * B + c elements (bsm: a * Bp + c), packed in list order.  The
// section's bytes and every pointer into it come from its list (fields_off; crf_debug_ws_fields shows the map).
//   pb     per-utterance results and marks (LossParams; [B] unless noted): cb_part [B][kResMaxK], redo [2][B]; 256 B bytes
//   xch    behind the granules (WsLayout::xch_bytes): the flag words of a call without a context's fine-grained block (crf_device.h kFlag*)
//   bsm    utterance-minor kernels (BatchParams): mxf, mxb [3][Bp]; bar = the persistent launch's grid barrier [kBatBarWords], its time-out
//          word (BatchParams::err) and 127 words more, ONE field: crf_batch_init_kernel clears all 640 words through `bar`
#define CRF_PB_FIELDS(X)                                                                                                                          \
    X(ctc_zc, 8, 1, 0) X(cb_mxs, 8, 1, 0) X(den_zs, 4, 1, 0) X(den_ez, 4, 1, 0) X(ctc_ez, 4, 1, 0) X(cost_alpha, 4, 1, 0) X(cost_beta, 4, 1, 0)     \
    X(cost_ctc, 4, 1, 0) X(invalid, 4, 1, 0) X(spare0, 4, 1, 0) X(cb_part, 4, kResMaxK, 0) X(cb_F, 4, 1, 0) X(spare1, 4, 7 - kResMaxK, 0)          \
    X(redo, 4, 2, 0) X(redo_ctc, 4, 1, 0) X(ctc_logdom, 4, 1, 0) X(spare2, 4, 40, 0)
#define CRF_XCH_FIELDS(X) X(flags, 4, 0, kFlagWords) X(spare0, 8, 1, 0)
#define CRF_BSM_FIELDS(X) X(mxf, 4, 3, 0) X(mxb, 4, 3, 0) X(Ef, 4, 1, 0) X(Fb, 4, 1, 0) X(zs, 4, 1, 0) X(zb, 4, 1, 0) X(spare0, 4, 2, 0) X(bar, 4, 0, 640)
constexpr int kBatBarWords = 512;
static_assert(kResMaxK <= 7, "cb_part and cb_F share the eight floats per utterance in front of redo");
#define CRF_FIELD_REC(name, elem, a, c) {#name, elem, a, c},
#define CRF_PB_ENUM(name, ...) kPb_##name,
#define CRF_XCH_ENUM(name, ...) kXch_##name,
#define CRF_BSM_ENUM(name, ...) kBsm_##name,
enum PbField : int { CRF_PB_FIELDS(CRF_PB_ENUM) kPbCount };
enum XchField : int { CRF_XCH_FIELDS(CRF_XCH_ENUM) kXchCount };
enum BsmField : int { CRF_BSM_FIELDS(CRF_BSM_ENUM) kBsmCount };
static const WsField kPbFields[kPbCount] = {CRF_PB_FIELDS(CRF_FIELD_REC)};
static const WsField kXchFields[kXchCount] = {CRF_XCH_FIELDS(CRF_FIELD_REC)};
static const WsField kBsmFields[kBsmCount] = {CRF_BSM_FIELDS(CRF_FIELD_REC)};
#undef CRF_PB_ENUM
#undef CRF_XCH_ENUM
#undef CRF_BSM_ENUM
#undef CRF_FIELD_REC

// the register-resident kernels are used whenever the graph fits them (res.K > 0) and V fits their
// emission-row prefetch; CRF_NO_RESIDENT=1 at graph creation forces the streaming kernels
static size_t res_lds_bytes(const HostGraph *h, int V, int dir, int rows_cu_max);
static bool use_resident(const HostGraph *h, int64_t V) {
    // (the two fixed 64 KiB state-vector buffers leave 32 KiB for the CU's row table and the emission rows: a K = 1 layout
    // with ~6 k+ rows, or a call with far more classes than the den_lm has labels, takes the next kernel family instead)
    return h && h->dev.res.K > 0 && V <= (int64_t)kEpRegsR * kResThreads && h->dev.res.f.G <= kResGmax && h->dev.res.b.G <= kResGmax &&
           std::max(res_lds_bytes(h, (int)V, 0, h->res_rows_cu_f), res_lds_bytes(h, (int)V, 1, h->res_rows_cu_b)) <= (size_t)160 * 1024;
}

// the factored layout (one CU per recursion) is preferred whenever the graph has it; CRF_NO_FACTORED=1 at
// graph creation keeps the generic resident kernels
static size_t fac_lds_bytes(const HostGraph *h, int V, int dir);
static bool use_factored(const HostGraph *h, int64_t V) {
    // (the layout was budgeted for the graph's own label range, res_layout.cpp: a call with far more classes than the den_lm
    // has labels may not fit the LDS any more and takes the next kernel family)
    return h && h->dev.fac.ok && V <= (int64_t)kEpRegsR * kResThreads &&
           std::max(fac_lds_bytes(h, (int)V, 0), fac_lds_bytes(h, (int)V, 1)) <= (size_t)160 * 1024;
}

static int pair2_mode(const HostGraph *h, int64_t B, int64_t V);

// LDS of the robust fallback kernels (the larger of the two directions)
static size_t robust_lds_bytes(const HostGraph *h, int V, bool gv) {
    const size_t tail = (size_t)rup64(V) * 8 + 2 * kChainWaves * 4 + 16 * 8 + 64;
    if (gv) return tail;
    return std::max((size_t)2 * rup64(h->dev.S) + h->dev.Pr, (size_t)4 * h->dev.Pr) * 8 + tail;   // (fp64 logarithms: den_forward_robust / den_backward_robust)
}

// The denominator kernels of a call, chosen ONCE from the graph, B, V and the switches (read per call): the workspace is laid down for this
// family, the plan and the launches read it (CallPlan::fam).  The enumerators are what crf_den_kernels returns.
enum DenKind : int { kDenNone = -1, kDenStreaming = 0, kDenResident = 1, kDenFactored = 2, kDenBatch = 3 };
struct DenFamily {
    DenKind kind = kDenNone;     // none: a numerator-only call (no graph)
    bool gv = false;             // streaming kernels: the state vectors do not fit the LDS and live in the workspace (section gvec)
    bool gv_robust = false;      // the robust fallback kernels keep their vectors in global memory too
    int p2mode = 0;              // two utterances per workgroup: 0 no, 1 on the main factored layout, 2 on HostGraph::facp (pair2_mode)
    const FacDev *FX = nullptr;  // factored: the layout this call works with -- the main one, or (p2mode 2) the second one
    int UL = 0; int64_t Bp = 0;  // utterance-minor layout (large graphs): utterances per group, B rounded up to it
    int64_t Rq = 0, Rb = 0;      // row strides of Q / BP
    bool fac() const { return kind == kDenFactored; }
    bool res() const { return kind == kDenFactored || kind == kDenResident; }   // register-resident kernels of either layout
    bool bat() const { return kind == kDenBatch; }
    bool pair2() const { return p2mode != 0; }
};
static DenFamily choose_den_family(const HostGraph *h, int64_t B, int64_t V) {
    DenFamily f;
    bool fac = use_factored(h, V), res = fac || use_resident(h, V);
    // graphs that fit neither register-resident layout take the utterance-minor kernels (CRF_NO_BATCH=1: the streaming
    // kernels instead; CRF_FORCE_BATCH=1: every graph, for tests)
    const bool force_bat = opt_on(kOpt_force_batch);
    const bool bat = h && h->dev.bat.ok && (force_bat || (!res && !opt_on(kOpt_no_batch)));
    if (bat) res = fac = false;
    f.kind = !h ? kDenNone : bat ? kDenBatch : fac ? kDenFactored : res ? kDenResident : kDenStreaming;
    // utterances per group: as wide as the batch allows (an arc is fetched once per group); 32 instead of 64 when a group's state
    // vector [S][64] would not stay in an XCD's 4 MiB L2 next to the arc stream (> ~2.25 MB) -- but never narrower than 32 for
    // that reason: every group reads the whole arc stream again and narrower gathers are partial lines (measured: S = 16 385,
    // B = 64: UL 64 / 32 / 16 -> 31.6 / 29.7 / 34.5 ms; config #5 with B = 64, where not even [S][8] fits: UL 64 / 32 / 8 -> 379 /
    // 271 / 569 ms).  CRF_BAT_UL overrides, for sweeps.
    f.UL = B > 32 ? 64 : B > 16 ? 32 : B > 8 ? 16 : 8;
    if (h && f.UL == 64 && std::max<int64_t>(h->dev.S, h->dev.P) * f.UL * 4 > (int64_t)(2.25 * 1024 * 1024)) f.UL = 32;
    { const int v = opt(kOpt_bat_ul, 0); if (v == 8 || v == 16 || v == 32 || v == 64) f.UL = v; }
    f.Bp = (B + f.UL - 1) / f.UL * f.UL;
    f.p2mode = fac ? pair2_mode(h, B, V) : 0;
    f.FX = fac ? (f.p2mode == 2 ? &h->facp : &h->dev.fac) : nullptr;
    // (rows are at least Pr wide: the robust fallback stores them in pair order, whatever layout the fast kernels use)
    f.Rq = h ? std::max<int64_t>(fac ? f.FX->Rq : res ? h->dev.res.f.R : h->dev.Pr, h->dev.Pr) : 0;
    f.Rb = h ? std::max<int64_t>(fac ? f.FX->Rbp : res ? h->dev.res.b.R : h->dev.Pr, h->dev.Pr) : 0;
    f.gv = h && !res && !bat && std::max((size_t)3 * rup64(h->dev.S), (size_t)4 * h->dev.Pr) * 4 + 2 * (size_t)rup64((int)V) * 4 + 1024 > 160 * 1024;
    f.gv_robust = h && robust_lds_bytes(h, (int)V, false) > 160 * 1024;
    return f;
}

// the sections of a call of this family and shape, and nothing else
static WsLayout ws_layout(const DenFamily &fam, const HostGraph *h, int64_t B, int64_t T, int64_t V, int64_t Sc) {
    WsLayout w{};
    w.gap = ws_gap_bytes();
    const bool fac = fam.fac(), res = fam.res(), bat = fam.bat();
    const FacDev *FX = fam.FX;
    w.add(kWs_ep, B * T * V * 4);
    w.add(kWs_mx, B * T * 4);
    w.add(kWs_moff, B * T * 4);   // fused log_softmax only (crf_loss_fwd_bwd_logits)
    w.add(kWs_invs, B * T * 4);
    const int64_t qb = bat ? T * (int64_t)h->dev.P * fam.Bp : 0;   // utterance-minor rows [T][P][Bp]
    w.add(kWs_Q, std::max(B * T * fam.Rq, qb) * 4);
    w.add(kWs_BP, std::max(B * T * fam.Rb, qb) * 4);
    w.add(kWs_EQ, B * T * 4);
    w.add(kWs_EB, B * T * 4);
    w.add(kWs_CA, B * T * Sc * 8);
    w.add(kWs_CB, B * T * Sc * 8);
    w.add(kWs_ECA, B * T * 4);
    w.add(kWs_ECB, B * T * 4);
    w.add(kWs_pb, fields_off(kPbFields, kPbCount, B));
    w.add(kWs_cbad, B * T * 4);   // frames of the numerator marked for the log-domain fallback
    // tagged granules [2 slots] of both directions, then one XCD-id word per CU of every recursion
    w.xch_bytes = (res && !fac && h->dev.res.K > 1) ? al((B * 2 * ((int64_t)h->dev.res.f.G + h->dev.res.b.G) + 2 * B * kResMaxK) * 8)
                : (fac && FX->K > 1) ? al((B * 2 * ((int64_t)FX->f.G + FX->b.G) + 2 * B * kResMaxK) * 8) : 0;
    w.add(kWs_xch, w.xch_bytes + fields_off(kXchFields, kXchCount, B));   // granules | CRF_XCH_FIELDS
    w.add(kWs_row0, res ? B * fam.Rb * 4 : 0);
    w.add(kWs_ept, bat ? T * V * fam.Bp * 4 : 0);
    w.add(kWs_Af, bat ? 2 * ((int64_t)h->dev.S + (h->fb.ok ? h->fb.NU : 0)) * fam.Bp * 4 : 0);   // (+ the U entries of factored streams)
    w.add(kWs_Zb, bat ? 2 * (int64_t)h->dev.P * fam.Bp * 4 : 0);
    w.add(kWs_bsm, bat ? fields_off(kBsmFields, kBsmCount, fam.Bp) : 0);
    // (floats per utterance: the streaming kernels' fp32 vectors, or the log-domain fallback's fp64 ones -- forward A[2][Sp] + Ql[Pr], backward Z[2][Pr] + BPst[2][Pr])
    w.gvec_stride = h ? std::max<int64_t>(3 * (int64_t)rup64(h->dev.S) + 5 * (int64_t)h->dev.Pr, 2 * (2 * (int64_t)rup64(h->dev.S) + 5 * (int64_t)h->dev.Pr)) : 0;
    w.add(kWs_gvec, (fam.gv || fam.gv_robust) ? B * w.gvec_stride * 4 : 0);
    // factored recursions launched in segments park their state vector + exponent here: [2 dir][B][stride]
    w.state_stride = fac ? rup64(std::max(FX->f.G, FX->b.G)) + 64 : 0;
    w.add(kWs_state, 2 * B * w.state_stride * 4);
    // two utterances per workgroup: one dump row per (direction, pair) for the row stores of an utterance that has ended
    w.dump_stride = fac ? al(std::max(fam.Rq, fam.Rb)) : 0;
    w.add(kWs_dump, fac ? 2 * ((B + 1) / 2) * w.dump_stride * 4 : 0);
    return w;
}

static size_t res_lds_bytes(const HostGraph *h, int V, int dir, int rows_cu_max) {
    const int G = dir == 0 ? h->dev.res.f.G : h->dev.res.b.G;
    (void)G;
    return (size_t)2 * kResXB + ((size_t)rows_cu_max + 2 * (size_t)rup64(V + 1) + 2 * kResWaves + 2 * kResWaves + 16) * sizeof(float);
}

static size_t chain_lds_bytes(const HostGraph *h, int V, int Sc, int role, bool gv = false) {
    const size_t tail = 2 * kChainWaves + 2 * kChainWaves + 16;  // wmax + 16 doubles + slack
    size_t fl;
    if (role == 0) fl = (gv ? 0 : (size_t)3 * rup64(h->dev.S)) + 2 * rup64(V) + tail;
    else if (role == 1) fl = (gv ? 0 : (size_t)4 * h->dev.Pr) + 2 * rup64(V) + tail;
    else fl = (size_t)2 * (2 * Sc + 3 * kChainWaves) + Sc + 16;  // doubles counted as 2 floats
    return fl * sizeof(float);
}

// ---------------------------------------------------------------------------------------------
// Per-(device, caller stream) context: ONE side stream, the fork/join events and a few flag words.
// A call needs two streams at most -- the caller's (denominator recursions: forward and backward are one grid) and
// one side stream (numerator recursions, then the grad pass that follows the recursions in stages).  Nothing is
// shared between two caller streams or two devices, so calls on different streams / from different host threads do
// not touch each other's events or counters; calls on ONE stream are ordered by the stream (the counters of call
// n+1 are cleared by its prep kernel, which runs after call n has joined everything back into that stream).
// ---------------------------------------------------------------------------------------------
constexpr int kFlagInts = 2048;
static_assert(kStageFrames == kGDFrames && kFlagStage + kMaxStages <= kFlagFallback && kFlagFallback + 2 <= kFlagWords, "stage_plan.h plans for the grad kernels' blocks; the stage counters lie between the named flag words");
struct DevCtx {
    std::mutex mu;            // one call at a time is ENQUEUED through a context (host side only; nothing waits on the GPU)
    int dev = 0;
    hipStream_t owner{};
    hipStream_t side{};       // null: no side stream that runs beside the owner was found -> everything on the owner's stream
    hipStream_t aux{};        // a third stream that runs beside the owner's (numerator fallback chains beside the grad stages), or null
    hipEvent_t ev_a{}, ev_b{};
    int *seen = nullptr;      // pinned host word the log-domain numerator chains write the call number to (read without a sync: a hint)
    int *hostw = nullptr;     // pinned, mapped host words: [0] = seen (when there is a third stream), [4] = the one-launch grad pass has timed out
    bool gd_fallback = false; // ... and this context has gone back to one grad launch per stage
    int call_id = 0;
    hipEvent_t fork{}, join{}, ev[kMaxStages]{}, evb[kMaxStages]{};
    int *flags = nullptr;     // fine-grained (uncached, cross-XCD coherent) words: crf_device.h kFlagErr, kFlagStarted, kFlagStage ..., kFlagProbe
    bool warned = false;
    int reprobes = 0;         // probes for a side stream after the first one found none (reprobe_side: at calls 256, 1 024, 4 096)
    int side_kind = 0, side_tries = 0;   // find_beside: what kind of stream the side stream is, how many candidates were probed
    char side_desc[96] = "none";
};
static std::mutex g_ctx_mu;
static std::vector<DevCtx *> g_ctxs;

// Do two streams run side by side?  HIP maps every stream of the process onto GPU_MAX_HW_QUEUES (default 4) hardware
// queues; two streams on one queue run their kernels one after the other.  Two single-wave kernels shake hands through
// fine-grained memory: each raises its flag and waits (bounded, ~5 ms) for the other's.  Both see the other only if
// they were resident at the same time.
__global__ void crf_probe_kernel(int *flags, int me, int other) {
    __hip_atomic_store(flags + me, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    int saw = 0;
    for (int spins = 0; spins < 2500 && !saw; ++spins) {   // ~2 us per spin: bounded at ~5 ms
        saw = __hip_atomic_load(flags + other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (!saw) __builtin_amdgcn_s_sleep(64);
    }
    __hip_atomic_store(flags + 2 + me, saw ? 1 : 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A stream that runs BESIDE `owner`, or null.  HIP (ROCclr) gives every stream one of GPU_MAX_HW_QUEUES (default 4) HSA queues PER
// PRIORITY -- a new stream takes the queue with the fewest users -- and a stream created with a CU mask gets a queue of its own.
// In a trainer process the pools are crowded before this library is loaded (torch's stream pool: 32 streams per priority as soon as
// c10d asks for one; RCCL's own), so the least-used queue may well be the owner's, and a candidate that is destroyed gives its
// slot back: the next one lands on the same queue again (rounds 2 - 3 probed six candidates that way and found all six behind the
// owner in every process that had initialised RCCL).  Hence: failed candidates stay alive until one passes -- each pushes the
// next one to another queue --, then the other priorities' pools (low first: the side stream's work is the filler, the owner's den
// grid is the critical path), then a CU-masked stream with every CU enabled.  Switch `side_kind` (1 plain, 2 high, 3 low, 4 masked)
// restricts the search to one kind.
enum { kSideNone = 0, kSidePlain, kSideHigh, kSideLow, kSideMask };
static const char *const kSideNames[] = {"none", "plain", "priority-high", "priority-low", "cu-mask"};
static hipStream_t make_candidate(int kind, int dev) {
    hipStream_t s{};
    hipError_t e = hipErrorInvalidValue;
    if (kind == kSidePlain) {
        e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    } else if (kind == kSideHigh || kind == kSideLow) {
        int least = 0, greatest = 0;   // (numerically lower = higher priority)
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
            e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, kind == kSideHigh ? greatest : least);
    } else if (kind == kSideMask) {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) {
            std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0xffffffffu);
            if (ncu % 32) mask.back() = (1u << (ncu % 32)) - 1u;
            e = hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data());
        }
    }
    if (e != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return s;
}
static bool runs_beside(hipStream_t owner, hipStream_t cand, int *flags) {
    int res[4] = {0, 0, 0, 0};
    // (a first launch on a new stream may pay for its queue's set-up: get that out of the way, or the owner's probe kernel
    // gives up before the candidate's has started -- the kernel below shakes hands with itself)
    int *const warm = flags + kFlagProbeWarm, *const hs = flags + kFlagProbe;
    bool ran = launch<crf_probe_kernel>("crf_probe_kernel", dim3(1), dim3(1), 0, cand, warm, 0, 0) == CRF_OK;
    ran = ran && hipStreamSynchronize(cand) == hipSuccess && hipMemset(hs, 0, sizeof(res)) == hipSuccess;
    ran = ran && launch<crf_probe_kernel>("crf_probe_kernel", dim3(1), dim3(1), 0, owner, hs, 0, 1) == CRF_OK;
    ran = ran && launch<crf_probe_kernel>("crf_probe_kernel", dim3(1), dim3(1), 0, cand, hs, 1, 0) == CRF_OK;
    ran = ran && hipStreamSynchronize(cand) == hipSuccess && hipStreamSynchronize(owner) == hipSuccess &&
          hipMemcpy(res, hs, sizeof(res), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ran) (void)hipGetLastError();
    return ran && res[2] == 1 && res[3] == 1;
}
static hipStream_t find_beside(hipStream_t owner, int *flags, int dev, int *kind_out, int *tries_out) {
    static const struct { int kind, count; } plan[] = {{kSidePlain, 8}, {kSideLow, 2}, {kSideHigh, 2}, {kSideMask, 1}};
    const int only = opt(kOpt_side_kind, 0);
    std::vector<hipStream_t> failed;
    hipStream_t found{};
    int tries = 0;
    for (const auto &ph : plan) {
        if (only > 0 && ph.kind != only) continue;
        // hipExtStreamCreateWithCUMask has no flags argument: the stream it makes is a BLOCKING one, i.e. it synchronises implicitly with the
        // legacy null stream -- beside the null stream (torch's default) the two probe kernels can never overlap, the candidate would only
        // cost its time-out.  (Beside any other owner it is a last resort with that caveat: null-stream work of the process orders with it.)
        if (ph.kind == kSideMask && owner == nullptr && only != kSideMask) continue;
        for (int i = 0; i < ph.count && !found; ++i) {
            hipStream_t cand = make_candidate(ph.kind, dev);
            if (!cand) break;
            ++tries;
            if (runs_beside(owner, cand, flags)) { found = cand; *kind_out = ph.kind; }
            else failed.push_back(cand);
        }
        if (found) break;
    }
    for (hipStream_t s : failed) (void)hipStreamDestroy(s);
    *tries_out = tries;
    if (!found) *kind_out = kSideNone;
    return found;
}

static int get_ctx(hipStream_t owner, DevCtx **out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= kMaxDev) { set_error("hipGetDevice failed"); return CRF_ERR_HIP; }
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (DevCtx *c : g_ctxs)
        if (c->dev == dev && c->owner == owner) { *out = c; return CRF_OK; }
    DevCtx *c = new DevCtx();
    c->dev = dev; c->owner = owner;
    // Words that one kernel polls while another, on a different XCD, updates them must not be cached in the poller's
    // L2 (the per-XCD L2s are not coherent with each other): fine-grained device memory is uncached in L2.
    void *fl = nullptr;
    if (hipExtMallocWithFlags(&fl, kFlagInts * sizeof(int), hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); fl = nullptr; }
    c->flags = (int *)fl;
    if ((e = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->join, hipEventDisableTiming)) != hipSuccess) {
        set_error(std::string("event create: ") + hipGetErrorString(e));
        delete c;
        return CRF_ERR_HIP;
    }
    for (int i = 0; i < kMaxStages; ++i) {
        (void)hipEventCreateWithFlags(&c->ev[i], hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&c->evb[i], hipEventDisableTiming);
    }
    {
        void *hp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) { c->hostw = (int *)hp; for (int i = 0; i < 16; ++i) c->hostw[i] = 0; }
        else (void)hipGetLastError();
    }
    // The side stream: the first candidate that demonstrably runs beside the owner's stream (once per context; the owner's
    // stream is drained first so that both probe kernels start at once).  find_beside() keeps the candidates that failed
    // alive until one passes, and tries streams of other priorities (queue pools of their own) and a CU-masked stream (a
    // queue of its own) when no plain stream does.  Switch `no_side_stream` skips it (everything then runs on the caller's
    // stream, one kernel after the other).
    const bool want_side = !opt_on(kOpt_no_side_stream);
    const bool trust = opt_on(kOpt_trust_side);   // (counter passes of a profiler run one kernel at a time: the probe cannot succeed there)
    if (want_side && c->flags && !trust) {
        (void)hipStreamSynchronize(owner);
        c->side = find_beside(owner, c->flags, dev, &c->side_kind, &c->side_tries);
    } else if (want_side) {   // no fine-grained memory for the probe: take a stream on trust
        if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); c->side = nullptr; }
        c->side_kind = c->side ? kSidePlain : kSideNone;
    }
    if (want_side && !c->side && !c->warned) {
        fprintf(stderr, "[ctc_crf_hip] no stream of this process runs beside the caller's stream (%d candidates probed: plain, other "
                        "priorities, CU-masked): the loss runs its kernels one after the other on the caller's stream -- correct, but slower\n",
                c->side_tries);
        c->warned = true;
    }
    // A third stream for work that may take long beside the staged grad pass (the numerator's log-domain chains): it must not sit
    // behind the owner's stream (the den grid), which is all the probe asks; sharing a queue with the side stream only delays it.
    if (c->side && c->flags && !trust &&
        hipEventCreateWithFlags(&c->ev_a, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->ev_b, hipEventDisableTiming) == hipSuccess) {
        (void)hipStreamSynchronize(owner);
        int kind = 0, tries = 0;
        c->aux = find_beside(owner, c->flags, dev, &kind, &tries);
        if (c->aux && c->hostw) c->seen = c->hostw;
    }
    snprintf(c->side_desc, sizeof(c->side_desc), "%s (candidate %d)%s", kSideNames[c->side_kind], c->side_tries, c->aux ? " + third stream" : "");
    g_ctxs.push_back(c);
    *out = c;
    return CRF_OK;
}

// A context whose probe found no stream beside the caller's (a device shared with another busy process at that moment can make the
// two single-wave probe kernels miss each other) asks again every 256 calls instead of staying on the serial schedule for good.
// (at most three more probes, at calls 256, 1 024 and 4 096: a process that cannot have a second queue at all -- GPU_MAX_HW_QUEUES=1 --
// must not pay a dozen candidates' time-outs every 256 steps for the rest of the run; never while the caller's stream is being captured)
static void reprobe_side(DevCtx *cx, hipStream_t stream) {
    if (cx->side || !cx->flags || opt_on(kOpt_no_side_stream) || opt_on(kOpt_trust_side) || cx->reprobes >= 3 ||
        cx->call_id + 1 != (256 << (2 * cx->reprobes))) return;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    ++cx->reprobes;
    if (cap != hipStreamCaptureStatusNone) return;
    (void)hipStreamSynchronize(stream);
    cx->side = find_beside(stream, cx->flags, cx->dev, &cx->side_kind, &cx->side_tries);
    snprintf(cx->side_desc, sizeof(cx->side_desc), "%s (candidate %d, found at call %d)", kSideNames[cx->side_kind], cx->side_tries, cx->call_id + 1);
}

// Grids whose workgroups WAIT FOR EACH OTHER (layouts over K > 1 CUs per recursion: every workgroup of a launch spins on its
// peers) are sized to fill the device; two callers enqueueing such grids on different streams at once could each become
// partially resident and wait for peers that are not (the bounded spins would then time out into the error word).  They are
// chained per device: a caller's co-resident launch waits (stream-level, on an event) for the previous caller's.
struct CoresChain { std::mutex mu; hipEvent_t ev{}; bool have = false; hipStream_t last{}; };
static CoresChain g_cores[kMaxDev];
struct CoresGuard {
    CoresChain *c = nullptr; hipStream_t st{};
    CoresGuard(bool needed, int dev, hipStream_t s) : st(s) {
        if (!needed || dev < 0 || dev >= kMaxDev) return;
        c = &g_cores[dev];
        c->mu.lock();
        if (c->have && c->last != st) (void)hipStreamWaitEvent(st, c->ev, 0);
    }
    ~CoresGuard() {
        if (!c) return;
        if (!c->have) c->have = hipEventCreateWithFlags(&c->ev, hipEventDisableTiming) == hipSuccess;
        if (c->have) { (void)hipEventRecord(c->ev, st); c->last = st; }
        c->mu.unlock();
    }
};


// optional per-kernel timing (crf_profile_enable / crf_profile_read)
struct Prof {
    bool on = false, have = false;
    hipEvent_t ev[16]{};  // start/stop per slot 0..6, [14],[15] whole call
    bool made = false, used[8]{};
};
static thread_local Prof g_prof;
static thread_local int g_call_streams = 1;          // crf_last_call_streams
static thread_local const char *g_side_desc = "none";   // crf_last_side_stream
static thread_local const int *g_last_err_word = nullptr;   // error word (+ kFlagFallback: fallback counts) of this thread's last call -- crf_last_fallback_counts
static thread_local const char *g_den_kernel = "";   // template instantiation of the denominator recursions' kernel in the last call (crf_last_den_kernel)
static void prof_mark(int slot, bool stop, hipStream_t st) {
    if (!g_prof.on) return;
    if (!g_prof.made) {
        for (auto &e : g_prof.ev) (void)hipEventCreate(&e);
        g_prof.made = true;
    }
    (void)hipEventRecord(g_prof.ev[2 * slot + (stop ? 1 : 0)], st);
    g_prof.used[slot] = true;
}

// streaming denominator recursions, forward + backward in one grid (profile slots 1 and 2 both time this launch)
template <bool GV>
static int launch_den_pair(const LossParams &p, size_t lds, hipStream_t st) {
    g_den_kernel = GV ? "crf_den_pair_kernel<true>" : "crf_den_pair_kernel<false>";
    prof_mark(1, false, st); prof_mark(2, false, st);
    const int rc = launch<crf_den_pair_kernel<GV>>("crf_den_pair_kernel", dim3((unsigned)(2 * p.B)), dim3(kChainThreads), lds, st, p);
    prof_mark(1, true, st); prof_mark(2, true, st);
    return rc;
}
// numerator chains, forward + backward in one grid (profile slots 3 and 4); states per thread from the longest label sequence
static int launch_ctc_pair(const LossParams &p, size_t lds, hipStream_t st, int64_t max_label_len) {
    const dim3 grid((unsigned)(2 * p.B)), block(kCtcThreads);
    prof_mark(3, false, st); prof_mark(4, false, st);
    const int rc = with_nr(2 * max_label_len + 1, kCtcThreads, [&](auto nr, int) {
        return launch<crf_ctc_pair_kernel<decltype(nr)::value>>("crf_ctc_pair_kernel", grid, block, lds, st, p);
    });
    prof_mark(3, true, st); prof_mark(4, true, st);
    return rc ? rc : launch<crf_ctc_check_kernel>("crf_ctc_check_kernel", dim3((unsigned)p.B), dim3(256), 0, st, p);
}

static ResParams res_params(const LossParams &lp, int dir, int b0) {
    const ResDev &R = lp.g.res;
    ResParams p{};
    p.L = dir == 0 ? R.f : R.b;
    p.K = R.K; p.B = lp.B; p.T = lp.T; p.V = lp.V; p.b0 = b0;
    p.rows_cu_max = dir == 0 ? lp.res_lds_rows_f : lp.res_lds_rows_b;
    p.Rout = dir == 0 ? lp.Rq : lp.Rb; p.Gf = R.f.G; p.Gb = R.b.G;
    p.lx = lp.lx; p.ep = lp.ep; p.mx = lp.moff;   // (the resident kernels use it for the log-likelihood offset only)
    p.Out = dir == 0 ? lp.Q : lp.BP; p.Eout = dir == 0 ? lp.EQ : lp.EB; p.Row0 = lp.Row0;
    p.xch = lp.xch; p.err = lp.err;
    p.x_start = R.x_start; p.x_end = R.x_end; p.den_zs = lp.den_zs; p.cost_alpha = lp.cost_alpha; p.den_ez = lp.den_ez;
    p.z_lab = R.z_lab; p.z_end = R.z_end; p.brow_start = R.brow_start; p.brow_end = R.brow_end; p.bcsr = R.bcsr;
    p.cb_part = lp.cb_part; p.cb_mxs = lp.cb_mxs; p.cb_F = lp.cb_F; p.redo = lp.redo;
    return p;
}
// generic register-resident recursions of the utterances [b0, b0 + nb): 2 * nb * K workgroups, forward first
static int launch_res_pair(const LossParams &lp, size_t lds, int b0, int nb, hipStream_t st) {
    const ResParams pf = res_params(lp, 0, b0), pb = res_params(lp, 1, b0);
    return launch<crf_res_pair_kernel>(g_den_kernel = "crf_res_pair_kernel", dim3((unsigned)(2 * nb * lp.g.res.K)), dim3(kResThreads), lds, st, pf, pb);
}

static size_t fac_lds_bytes(const HostGraph *h, int V, int dir) {
    const FacDev &F = h->dev.fac;
    const FacDirDev &L = dir == 0 ? F.f : F.b;
    const int nw = F.threads / kWave;
    const int trows = F.K > 1 ? std::max(L.cu_row[1] - L.cu_row[0], L.cu_row[2] - L.cu_row[1]) : L.R;   // two CUs: each holds its own rows' constants only
    const size_t table = F.rcl ? (size_t)(trows + 64) * (dir == 0 ? 8 : 16) : (size_t)L.R * 16;   // row constants (fac_chain_body)
    return (size_t)2 * rup64(L.G) * 4 + table +
           ((size_t)2 * rup64(V + 1) + 2 * nw + 2 * nw + 16) * sizeof(float);
}
// ... of the two-utterance kernels (fac_chain_body2): float2 state vectors and emission rows, the same row table
static size_t fac2u_lds_bytes(const FacDev &F, int V, int dir) {
    const FacDirDev &L = dir == 0 ? F.f : F.b;
    const size_t table = F.rcl ? (size_t)(L.R + 64) * (dir == 0 ? 8 : 16) : (dir == 1 ? (size_t)L.R * 8 : (size_t)0);
    return (size_t)2 * rup64(L.G) * 8 + table + (size_t)2 * rup64(V + 1) * 8 + 24 * 4 + (F.threads / kWave) * 8 + 64;
}
// Two utterances per workgroup?  -> 0: no; 1: on the main layout (its 768-thread geometries, as they are); 2: on the second layout
// (HostGraph::facp, 512 threads x 30 chunks: built beside a main layout of another geometry).  Switch fac_pair2 = 1 forces it for any
// batch, 0 forbids it.  One CU per recursion only, and both float2 vectors must fit the LDS.
//   main layout, 768 threads (round 3): the pair kernel's frame is 3.65 us against 1.98 us for one utterance -- 126 of a thread's 168
//   registers hold arcs, 26 - 39 dwords spill -- so it wins only where the one-utterance grid no longer fits the device at once
//   (2 B > CUs): B = 256: 10.1 against 10.5 ms per step; B = 128: 5.9 against 5.3; B = 96: 5.7 against 4.4.
//   second layout (round 5; 512 threads x 30 chunks, no spills inside the frame loop): the frame for two utterances is 3.25 us -- still
//   1.9 x the one-utterance frame: with eight waves the kernel is bound by what ONE wave can issue (30 chunks x 12 instructions + two
//   epilogues per slice, ~4.3 cycles each), not by the LDS whose gathers it halves.  Measured (metric graph, ms per step, this kernel /
//   the one-utterance kernel; profiles/round5_ab_two_utterances_512.txt): B = 64 5.08 / 2.81, B = 96 5.18 / 3.95, B = 128 5.39 / 4.92,
//   B = 192 7.83 / 8.77, B = 256 9.2 - 9.4 / 9.46 -- it pays where the one-utterance grid needs two rounds of the device: 2 B > CUs.
static int pair2_mode(const HostGraph *h, int64_t B, int64_t V) {
    const FacDev &F = h->dev.fac;
    const int sw = opt(kOpt_fac_pair2, -1);
    if (sw == 0 || !F.ok || F.K != 1) return 0;
    const int ncu = h->ncu > 0 ? h->ncu : 256;
    if (h->facp.ok && std::max(fac2u_lds_bytes(h->facp, (int)V, 0), fac2u_lds_bytes(h->facp, (int)V, 1)) <= (size_t)160 * 1024 &&
        V <= (int64_t)kEpRegsR * kResThreads) {
        if (sw == 1 || 2 * B > ncu) return 2;
        return 0;
    }
    if (F.threads != kFac3Threads) return 0;
    if (std::max(fac2u_lds_bytes(F, (int)V, 0), fac2u_lds_bytes(F, (int)V, 1)) > (size_t)160 * 1024) return 0;
    return (sw == 1 || 2 * B > ncu) ? 1 : 0;
}
static FacParams fac_params(const LossParams &lp, int dir, int *started, int i0, int i1, float *state, int nb, const int *bound, int *stage_cnt) {
    const FacDev &F = lp.g.fac;
    FacParams p{};
    p.L = dir == 0 ? F.f : F.b;
    p.bx_idx = F.bx_idx; p.bx_w = F.bx_w; p.nbx = F.nbx; p.bx_se = F.bx_se;
    p.B = lp.B; p.T = lp.T; p.V = lp.V; p.Rout = dir == 0 ? lp.Rq : lp.Rb; p.NT = F.NT; p.Rf = F.f.R;
    p.lx = lp.lx; p.ep = lp.ep; p.mx = lp.moff;   // (the resident kernels use it for the log-likelihood offset only)
    p.Out = dir == 0 ? lp.Q : lp.BP; p.Eout = dir == 0 ? lp.EQ : lp.EB; p.Row0 = lp.Row0;
    p.started = started; p.i0 = i0; p.i1 = i1; p.state = state;
    p.nb = nb; p.stage_cnt = stage_cnt;
    for (int k = 0; k < kMaxStages; ++k) p.bound[k] = (bound && k < nb) ? bound[k] : 0;
    p.frow_meta = F.frow_meta; p.x_start = F.x_start; p.x_end = F.x_end;
    p.den_zs = lp.den_zs; p.cost_alpha = lp.cost_alpha; p.den_ez = lp.den_ez;
    p.brow_meta = F.brow_meta; p.z_lab = F.z_lab; p.z_end = F.z_end; p.brow_start = F.brow_start; p.brow_end = F.brow_end;
    p.cb_part = lp.cb_part; p.cb_mxs = lp.cb_mxs; p.cb_F = lp.cb_F; p.redo = lp.redo;
    p.npair = (lp.B + 1) / 2; p.dump = lp.dump; p.dump_stride = lp.dump_stride;
    p.K = F.K; p.b0 = 0; p.nbu = lp.B; p.Gf = F.f.G; p.Gb = F.b.G; p.xch = lp.xch; p.err = lp.err; p.xlist = F.xlist; for (int k = 0; k < 3; ++k) p.xlist_off[k] = F.xlist_off[k];
    return p;
}
// factored recursions over TWO CUs each, utterances [b0, b0 + nbu): every workgroup of a launch must be resident at once
// (its peer spins on it), so the caller launches groups of at most CUs / 4 utterances
static int launch_fac2_pair(const LossParams &lp, size_t lds, hipStream_t st, int b0, int nbu) {
    FacParams pf = fac_params(lp, 0, nullptr, 0, lp.T, nullptr, 0, nullptr, nullptr);
    FacParams pb = fac_params(lp, 1, nullptr, 0, lp.T, nullptr, 0, nullptr, nullptr);
    pf.b0 = pb.b0 = b0; pf.nbu = pb.nbu = nbu;
    const dim3 grid((unsigned)(2 * nbu * 2));
    if (lp.g.fac.threads == kFac4Threads)   // 1024 threads x 15 chunks, four waves per SIMD (round 4)
        return launch<crf_fac2_pair_kernel<kFac4Threads, kFac4NCH, CRF_FAC4_NB_ML, CRF_FAC4_NB_ML>>(
            g_den_kernel = "crf_fac2_pair_kernel<1024,15," CRF_STR(CRF_FAC4_NB_ML) "," CRF_STR(CRF_FAC4_NB_ML) ">", grid, dim3(kFac4Threads), lds, st, pf, pb);
    return launch<crf_fac2_pair_kernel<kFac3Threads, kFac3ArcCh, CRF_FAC3_NB_F, CRF_FAC3_NB_B>>(
        g_den_kernel = "crf_fac2_pair_kernel<768,20,4,4>", grid, dim3(kFac3Threads), lds, st, pf, pb);
}
// (a den kernel's name as crf_last_den_kernel reports it: the kernel, FLAG, the other template arguments as written at the instantiation)
#define CRF_DEN_NAME(KERNEL_, ARGS_) (FLAG ? KERNEL_ "<true," ARGS_ ">" : KERNEL_ "<false," ARGS_ ">")
// factored recursions, iterations [i0, i1) of both directions as one grid of 2B workgroups; FLAG: publish stage counters
// (both directions bump the same counters: a stage is complete at 2B) and store the rows write-through
template <bool FLAG>
static int launch_fac_pair(const LossParams &lp, size_t lds, hipStream_t st, int *started, int i0, int i1, float *fstate, float *bstate,
                           int nb = 0, const int *bound = nullptr, int *stage_cnt = nullptr) {
    const FacDev &F = lp.g.fac;
    const bool g3 = F.threads == kFac3Threads, ml = F.multilane != 0, adt = F.addtid != 0;
    const FacParams pf = fac_params(lp, 0, started, i0, i1, fstate, nb, bound, stage_cnt);
    const FacParams pb = fac_params(lp, 1, started, i0, i1, bstate, nb, bound, stage_cnt);
    const dim3 grid((unsigned)(2 * lp.B)), b3(kFac3Threads), b4(kFac4Threads);
    // 768 threads, row constants in the LDS table: 20 chunks of arcs per thread (F.rcl == 1), or all 21 slots (== 2: graphs that need them)
    if (g3 && F.rcl == 1 && !ml)
        return launch<crf_fac_pair_kernel<FLAG, kFac3Threads, kFac3ArcCh, CRF_FAC3_NB_F, CRF_FAC3_NB_B, false, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "768,20,4,4,false,true"), grid, b3, lds, st, pf, pb);
    if (g3 && F.rcl == 1)
        return launch<crf_fac_pair_kernel<FLAG, kFac3Threads, kFac3ArcCh, CRF_FAC3_NB_F, CRF_FAC3_NB_B, true, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "768,20,4,4,true,true"), grid, b3, lds, st, pf, pb);
    if (g3 && F.rcl == 2 && !ml)
        return launch<crf_fac_pair_kernel<FLAG, kFac3Threads, kFac3LNCH, CRF_FAC3_NB_F, CRF_FAC3_NB_B, false, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "768,21,4,4,false,true"), grid, b3, lds, st, pf, pb);
    if (g3 && F.rcl == 2)
        return launch<crf_fac_pair_kernel<FLAG, kFac3Threads, kFac3LNCH, CRF_FAC3_NB_F, CRF_FAC3_NB_B, true, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "768,21,4,4,true,true"), grid, b3, lds, st, pf, pb);
    // 1024 threads: four waves per SIMD (the planner's first choice)
    // (the last template argument: next-vector stores by ds_write_addtid_b32, the planner's choice per graph -- FacDev::addtid)
    if (F.threads == kFac4Threads && ml && adt)
        return launch<crf_fac_pair_kernel<FLAG, kFac4Threads, kFac4NCH, CRF_FAC4_NB_ML, CRF_FAC4_NB_ML, true, true, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "1024," CRF_STR(CRF_FAC4_NCH) "," CRF_STR(CRF_FAC4_NB_ML) "," CRF_STR(CRF_FAC4_NB_ML) ",true,true,true"), grid, b4, lds, st, pf, pb);
    if (F.threads == kFac4Threads && ml)
        return launch<crf_fac_pair_kernel<FLAG, kFac4Threads, kFac4NCH, CRF_FAC4_NB_ML, CRF_FAC4_NB_ML, true, true, false>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "1024," CRF_STR(CRF_FAC4_NCH) "," CRF_STR(CRF_FAC4_NB_ML) "," CRF_STR(CRF_FAC4_NB_ML) ",true,true,false"), grid, b4, lds, st, pf, pb);
    if (F.threads == kFac4Threads && adt)
        return launch<crf_fac_pair_kernel<FLAG, kFac4Threads, kFac4NCH, CRF_FAC4_NB, CRF_FAC4_NB, false, true, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "1024," CRF_STR(CRF_FAC4_NCH) "," CRF_STR(CRF_FAC4_NB) "," CRF_STR(CRF_FAC4_NB) ",false,true,true"), grid, b4, lds, st, pf, pb);
    if (F.threads == kFac4Threads)
        return launch<crf_fac_pair_kernel<FLAG, kFac4Threads, kFac4NCH, CRF_FAC4_NB, CRF_FAC4_NB, false, true, false>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "1024," CRF_STR(CRF_FAC4_NCH) "," CRF_STR(CRF_FAC4_NB) "," CRF_STR(CRF_FAC4_NB) ",false,true,false"), grid, b4, lds, st, pf, pb);
    // 768 threads, row constants in registers
    if (g3 && ml)
        return launch<crf_fac_pair_kernel<FLAG, kFac3Threads, kFac3NCH, CRF_FAC3_NB_F, CRF_FAC3_NB_B, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "768,21,4,4,true,false"), grid, b3, lds, st, pf, pb);
    if (g3)
        return launch<crf_fac_pair_kernel<FLAG, kFac3Threads, kFac3NCH, CRF_FAC3_NB_F, CRF_FAC3_NB_B, false>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "768,21,4,4,false,false"), grid, b3, lds, st, pf, pb);
    return launch<crf_fac_pair_kernel<FLAG, kResThreads, kResNCH, kResBatch, kResBatch, true>>(
        g_den_kernel = CRF_DEN_NAME("crf_fac_pair_kernel", "512,30,6,6,true,false"), grid, dim3(kResThreads), lds, st, pf, pb);
}

// ... two utterances per workgroup: 2 * ceil(B / 2) workgroups
template <bool FLAG>
static int launch_fac_pair2(const LossParams &lp, size_t lds, hipStream_t st, int *started, int nb = 0, const int *bound = nullptr, int *stage_cnt = nullptr) {
    const FacDev &F = lp.g.fac;
    const bool ml = F.multilane != 0;
    const FacParams pf = fac_params(lp, 0, started, 0, lp.T, nullptr, nb, bound, stage_cnt);
    const FacParams pb = fac_params(lp, 1, started, 0, lp.T, nullptr, nb, bound, stage_cnt);
    const dim3 grid((unsigned)(2 * pf.npair)), b3(kFac3Threads);
    if (F.threads == kResThreads) {   // the second layout (HostGraph::facp): 512 threads x 30 chunks, row table, implicit entries
        if (!F.imp || !F.rcl) { set_error("two-utterance kernel on 512 threads: not the second layout"); return CRF_ERR_ARG; }
        if (!ml)
            return launch<crf_fac_pair2_kernel<FLAG, kResThreads, kResNCH, CRF_FAC5_NB2, CRF_FAC5_NB2, false, true>>(
                g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "512,30," CRF_STR(CRF_FAC5_NB2) "," CRF_STR(CRF_FAC5_NB2) ",false,true"), grid, dim3(kResThreads), lds, st, pf, pb);
        return launch<crf_fac_pair2_kernel<FLAG, kResThreads, kResNCH, CRF_FAC5_NB2, CRF_FAC5_NB2, true, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "512,30," CRF_STR(CRF_FAC5_NB2) "," CRF_STR(CRF_FAC5_NB2) ",true,true"), grid, dim3(kResThreads), lds, st, pf, pb);
    }
    // 768 threads: row constants in the LDS table (20 chunks of arcs, or all 21 slots), else in registers
    if (F.rcl == 1 && !ml)
        return launch<crf_fac_pair2_kernel<FLAG, kFac3Threads, kFac3ArcCh, CRF_FAC3_NB2, CRF_FAC3_NB2, false, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "768,20," CRF_STR(CRF_FAC3_NB2) "," CRF_STR(CRF_FAC3_NB2) ",false,true"), grid, b3, lds, st, pf, pb);
    if (F.rcl == 1)
        return launch<crf_fac_pair2_kernel<FLAG, kFac3Threads, kFac3ArcCh, CRF_FAC3_NB2, CRF_FAC3_NB2, true, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "768,20," CRF_STR(CRF_FAC3_NB2) "," CRF_STR(CRF_FAC3_NB2) ",true,true"), grid, b3, lds, st, pf, pb);
    if (F.rcl == 2 && !ml)
        return launch<crf_fac_pair2_kernel<FLAG, kFac3Threads, kFac3LNCH, CRF_FAC3_NB2, CRF_FAC3_NB2, false, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "768,21," CRF_STR(CRF_FAC3_NB2) "," CRF_STR(CRF_FAC3_NB2) ",false,true"), grid, b3, lds, st, pf, pb);
    if (F.rcl == 2)
        return launch<crf_fac_pair2_kernel<FLAG, kFac3Threads, kFac3LNCH, CRF_FAC3_NB2, CRF_FAC3_NB2, true, true>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "768,21," CRF_STR(CRF_FAC3_NB2) "," CRF_STR(CRF_FAC3_NB2) ",true,true"), grid, b3, lds, st, pf, pb);
    if (ml)
        return launch<crf_fac_pair2_kernel<FLAG, kFac3Threads, kFac3NCH, CRF_FAC3_NB2, CRF_FAC3_NB2, true, false>>(
            g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "768,21," CRF_STR(CRF_FAC3_NB2) "," CRF_STR(CRF_FAC3_NB2) ",true,false"), grid, b3, lds, st, pf, pb);
    return launch<crf_fac_pair2_kernel<FLAG, kFac3Threads, kFac3NCH, CRF_FAC3_NB2, CRF_FAC3_NB2, false, false>>(
        g_den_kernel = CRF_DEN_NAME("crf_fac_pair2_kernel", "768,21," CRF_STR(CRF_FAC3_NB2) "," CRF_STR(CRF_FAC3_NB2) ",false,false"), grid, b3, lds, st, pf, pb);
}
#undef CRF_DEN_NAME


}  // namespace crf

using namespace crf;

extern "C" {

int64_t crf_workspace_bytes(const crf_graph *g, int64_t B, int64_t T, int64_t V, int64_t max_label_len) {
    const HostGraph *h = g ? g->h : nullptr;
    return ws_layout(choose_den_family(h, B, V), h, B, T, V, rup64((int)(2 * max_label_len + 1))).total;
}

int crf_den_kernels(const crf_graph *g, int64_t B, int64_t T, int64_t V) {
    (void)T;
    if (!g || !g->h) { set_error("null graph"); return -1; }
    return choose_den_family(g->h, B, V).kind;
}

int crf_debug_ws_sections(const crf_graph *g, int64_t B, int64_t T, int64_t V, int64_t max_label_len, int64_t *out, int n_out) {
    const HostGraph *h = g ? g->h : nullptr;
    const WsLayout w = ws_layout(choose_den_family(h, B, V), h, B, T, V, rup64((int)(2 * max_label_len + 1)));
    return copy_sections(w.sec, w.nsec, out, n_out);
}
const char *crf_debug_ws_section_names(void) {
    static const std::string s = join_names(kWsNames, kWsCount);
    return s.c_str();
}

// the field lists of the sections pb, xch (behind the granules) and bsm
static int ws_field_list(const char *section, const WsField **f) {
    const std::string s = section ? section : "";
    if (s == "pb") { *f = kPbFields; return kPbCount; }
    if (s == "xch") { *f = kXchFields; return kXchCount; }
    if (s == "bsm") { *f = kBsmFields; return kBsmCount; }
    set_error("crf_debug_ws_fields: section '" + s + "' has no field list (pb, xch, bsm)");
    return -1;
}
int crf_debug_ws_fields(const char *section, int64_t n, int64_t *out, int n_out) {
    const WsField *f = nullptr;
    const int nf = ws_field_list(section, &f);
    for (int k = 0; k < nf && out && 3 * k + 2 < n_out; ++k) {
        out[3 * k] = fields_off(f, k, n); out[3 * k + 1] = fields_off(f, k + 1, n) - out[3 * k]; out[3 * k + 2] = f[k].elem;
    }
    return nf;
}
const char *crf_debug_ws_field_names(const char *section) {
    static thread_local std::string s;
    const WsField *f = nullptr;
    const int nf = ws_field_list(section, &f);
    if (nf < 0) return nullptr;
    s.clear();
    for (int k = 0; k < nf; ++k) { if (k) s += ','; s += f[k].name; }
    return s.c_str();
}

static int loss_impl(const crf_graph *g, const float *logp, int fused, int in_dtype, const int32_t *labels, const int32_t *lab_off,
                     const int32_t *lx, const int32_t *ly, int64_t B, int64_t T, int64_t V,
                     int64_t max_label_len, float c_den, float c_ctc, float *grad, float *loss,
                     float *costs_den, float *costs_beta, float *costs_ctc, int32_t *invalid, void *ws,
                     int64_t ws_bytes, void *stream_, int time_major = 0, int blank = 0);

int crf_loss_fwd_bwd(const crf_graph *g, const float *logp, const int32_t *labels, const int32_t *lab_off,
                     const int32_t *lx, const int32_t *ly, int64_t B, int64_t T, int64_t V,
                     int64_t max_label_len, float c_den, float c_ctc, float *grad, float *loss,
                     float *costs_den, float *costs_beta, float *costs_ctc, int32_t *invalid, void *ws,
                     int64_t ws_bytes, void *stream_) {
    return loss_impl(g, logp, 0, 0, labels, lab_off, lx, ly, B, T, V, max_label_len, c_den, c_ctc, grad, loss, costs_den, costs_beta,
                     costs_ctc, invalid, ws, ws_bytes, stream_);
}

int crf_loss_fwd_bwd_logits(const crf_graph *g, const void *logits, int dtype, const int32_t *labels, const int32_t *lab_off,
                            const int32_t *lx, const int32_t *ly, int64_t B, int64_t T, int64_t V,
                            int64_t max_label_len, float c_den, float c_ctc, float *grad, float *loss,
                            float *costs_den, float *costs_beta, float *costs_ctc, int32_t *invalid, void *ws,
                            int64_t ws_bytes, void *stream_) {
    if (dtype < 0 || dtype > 2) { set_error("crf_loss_fwd_bwd_logits: dtype must be 0 (f32), 1 (bf16) or 2 (f16)"); return CRF_ERR_ARG; }
    if (c_ctc == 0.f) { set_error("crf_loss_fwd_bwd_logits: the fused log_softmax needs the numerator pass (c_ctc != 0)"); return CRF_ERR_UNSUPPORTED; }
    return loss_impl(g, (const float *)logits, 1, dtype, labels, lab_off, lx, ly, B, T, V, max_label_len, c_den, c_ctc, grad, loss,
                     costs_den, costs_beta, costs_ctc, invalid, ws, ws_bytes, stream_);
}

int crf_ctc_fwd_bwd(const float *act, int time_major, int blank, const int32_t *labels, const int32_t *lab_off, const int32_t *lx,
                    const int32_t *ly, int64_t B, int64_t T, int64_t V, int64_t max_label_len, float c_ctc, float *grad, float *loss,
                    float *costs_ctc, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    if (c_ctc == 0.f) { set_error("crf_ctc_fwd_bwd: c_ctc is zero"); return CRF_ERR_ARG; }
    return loss_impl(nullptr, act, 0, 0, labels, lab_off, lx, ly, B, T, V, max_label_len, 0.f, c_ctc, grad, loss, nullptr, nullptr,
                     costs_ctc, invalid, ws, ws_bytes, stream_, time_major, blank);
}

int crf_ctc_fwd_bwd_logits(const void *act, int dtype, int time_major, int blank, const int32_t *labels, const int32_t *lab_off,
                           const int32_t *lx, const int32_t *ly, int64_t B, int64_t T, int64_t V, int64_t max_label_len, float c_ctc,
                           float *grad, float *loss, float *costs_ctc, int32_t *invalid, void *ws, int64_t ws_bytes, void *stream_) {
    if (dtype < 0 || dtype > 2) { set_error("crf_ctc_fwd_bwd_logits: dtype must be 0 (f32), 1 (bf16) or 2 (f16)"); return CRF_ERR_ARG; }
    if (c_ctc == 0.f) { set_error("crf_ctc_fwd_bwd_logits: c_ctc is zero"); return CRF_ERR_ARG; }
    return loss_impl(nullptr, (const float *)act, 1, dtype, labels, lab_off, lx, ly, B, T, V, max_label_len, 0.f, c_ctc, grad, loss, nullptr,
                     nullptr, costs_ctc, invalid, ws, ws_bytes, stream_, time_major, blank);
}

// ---------------------------------------------------------------------------------------------
// The loss call in parts: the arguments are checked (check_loss_args), the kernels, LDS sizes and the schedule are chosen as data
// (CallPlan: plan_kernels from the graph and the shape alone, plan_schedule with the facts of the device and the context), the workspace
// is carved into LossParams (bind_params), and a LossCall enqueues one of four stream schedules -- utterance-minor, staged, two streams,
// one stream -- followed by the fallbacks and finalize.
// ---------------------------------------------------------------------------------------------
struct LossArgs {
    const crf_graph *g; const float *logp; int fused, in_dtype;
    const int32_t *labels, *lab_off, *lx, *ly;
    int64_t B, T, V, max_label_len;
    float c_den, c_ctc, *grad, *loss, *costs_den, *costs_beta, *costs_ctc;
    int32_t *invalid; void *ws; int64_t ws_bytes; int time_major, blank;
};
// what a call's schedule depends on beside its arguments: plain values, read once per call
struct DevFacts {
    int ncu = 256;            // compute units of the context's device
    bool have_flags = false, have_side = false, have_aux = false;   // DevCtx::flags, side, aux
    bool segments = false;    // hipStreamWaitValue32 has been refused in this process
    bool gd_fallback = false; // DevCtx::gd_fallback
    int call_id = 0, seen = 0;   // this call's number; the call that last ran the numerator's log-domain chains (DevCtx::seen: a racing word, ONE read per call)
};
struct CallPlan {
    // the denominator family (choose_den_family), kernels and sizes, from the graph and the shape alone (plan_kernels)
    const HostGraph *h;
    DenFamily fam;
    bool den, ctc;
    int Sc, gnc, gcap, robust_env;
    bool grad_stage, gd_wide, gd_wide6, fast_den, fast_ctc;
    size_t lds_den, lds_ctc, lds_grad;  // dynamic LDS of the den recursions (whichever family), the numerator chains, the generic grad kernel
    // the schedule (plan_schedule)
    int ncu; int64_t den_wgs; bool have_flags, serial, no_overlap, segmode, staged, per_stage, ctc_wants_aux, par3;
    StagePlan stages;
};
static std::atomic<bool> g_use_segments{false};      // set when hipStreamWaitValue32 is refused

static CallPlan plan_kernels(const HostGraph *h, const DenFamily &fam, int64_t V, int64_t max_label_len, int Sc, bool den, bool ctc) {
    CallPlan pl{};
    pl.h = h; pl.fam = fam; pl.den = den; pl.ctc = ctc; pl.Sc = Sc;
    const bool res = fam.res(), gv = fam.gv, fac = fam.fac(), bat = fam.bat();   // (den is false without a graph, and then so are these)
    if (den && !res && !bat) pl.lds_den = std::max(chain_lds_bytes(h, (int)V, pl.Sc, 0, gv), chain_lds_bytes(h, (int)V, pl.Sc, 1, gv));
    if (res && !fac) pl.lds_den = std::max(res_lds_bytes(h, (int)V, 0, h->res_rows_cu_f), res_lds_bytes(h, (int)V, 1, h->res_rows_cu_b));
    if (fac) pl.lds_den = fam.pair2() ? std::max(fac2u_lds_bytes(*fam.FX, (int)V, 0), fac2u_lds_bytes(*fam.FX, (int)V, 1))
                                   : std::max(fac_lds_bytes(h, (int)V, 0), fac_lds_bytes(h, (int)V, 1));
    pl.lds_ctc = chain_lds_bytes(h, (int)V, pl.Sc, 2);
    const int gnc_all = den ? std::max(std::max(h->dev.NC, h->dev.res.NC), std::max(h->dev.fac.ok ? h->dev.fac.NC : 0, h->facp.ok ? h->facp.NC : 0)) : 0;
    // the generic grad kernel stages the two rows of a frame in LDS when they fit, else gathers them from L2
    pl.grad_stage = !den || bat || ((size_t)rup64((int)fam.Rq) + rup64((int)fam.Rb) + rup64(gnc_all) + 2 * (size_t)rup64((int)V)) * 4 <= 150 * 1024;
    pl.lds_grad = ((den && !bat && pl.grad_stage ? (size_t)rup64((int)fam.Rq) + rup64((int)fam.Rb) : 0) + rup64(bat ? 0 : gnc_all) + 2 * (size_t)rup64((int)V)) * sizeof(float);
    // The denominator half of the grad pass has a streaming kernel (index pairs in registers, rows
    // prefetched); it needs 16-bit row indices, rows of <= kGDRowRegs*256 floats and <= 2 chunks per thread.
    pl.gnc = den ? (fac ? fam.FX->NC : res ? h->dev.res.NC : h->dev.NC) : 0;
    pl.gcap = fac ? fam.FX->chunk_cap : kChunk;       // entries per chunk of the grad pass's pair lists
    pl.gd_wide = den && (fam.Rq > 4 * kGDRowRegs * kGDThreads || fam.Rb > 4 * kGDRowRegs * kGDThreads);   // 512-thread grad workgroups
    // (rows of up to 12 288 floats since round 6 -- 512 threads x 6 row registers: a den_lm with a state per seen bigram history has ~5.3 k forward rows
    // at 72 tokens, Rq = Rb = 10 752, 5 % beyond the 10 240 of five registers, and took the generic grad kernel: 10.8 ms of a 17.5 ms step)
    pl.gd_wide6 = den && (fam.Rq > 8 * kGDRowRegs * kGDThreads || fam.Rb > 8 * kGDRowRegs * kGDThreads);
    pl.fast_den = den && fam.Rq <= 8 * 6 * kGDThreads && fam.Rb <= 8 * 6 * kGDThreads && fam.Rq % 4 == 0 && fam.Rb % 4 == 0 && (!pl.gd_wide6 || (pl.gnc <= 2 * kGDThreads && pl.gcap != 8)) &&
                  pl.gnc <= 4 * kGDThreads && V <= kGDEpRegs * kGDThreads && !opt_on(kOpt_no_fast_grad);
    // numerator half of the grad pass: streaming kernel when the vocabulary fits its registers
    pl.fast_ctc = ctc && V <= kGCVRegs * kGCThreads && 2 * max_label_len + 1 <= kGCRegs * kGCThreads &&
                  !opt_on(kOpt_no_fast_grad);
    // CRF_ROBUST: 0 = never run the robust fallback, 1 = every utterance takes it (tests, or "safe mode"); default: the
    // utterances the fast kernels flag
    pl.robust_env = opt(kOpt_robust, -1);   // (read per call: tests switch it)
    return pl;
}

// every early return of a call, before any HIP call; fills the workspace layout and the device-independent part of the plan
static int check_loss_args(const LossArgs &a, WsLayout &w, CallPlan &pl) {
    const int64_t B = a.B, T = a.T, V = a.V;
    const bool den = a.c_den != 0.f, ctc = a.c_ctc != 0.f;
    if (!a.logp || !a.lx || !a.grad || !a.loss || !a.ws) { set_error("null argument"); return CRF_ERR_ARG; }
    if (B <= 0 || T <= 0 || V <= 0 || B * T > INT32_MAX) { set_error("bad B/T/V"); return CRF_ERR_ARG; }
    if (!den && !ctc) { set_error("c_den and c_ctc are both zero"); return CRF_ERR_ARG; }
    if (den && (!a.g || !a.g->h)) { set_error("denominator requested without a graph"); return CRF_ERR_ARG; }
    if (ctc && (!a.labels || !a.lab_off || !a.ly || a.max_label_len < 0)) { set_error("numerator requested without labels"); return CRF_ERR_ARG; }
    // The blank's column and the row layout are options of the numerator alone: a den_lm fixes the blank at 0 (label = ilabel - 1),
    // and the denominator kernels read [B][T][V] rows.  (Labels are device memory here: the callers check them.)
    if (a.blank < 0 || a.blank >= V) { set_error("blank " + std::to_string(a.blank) + " outside [0, V=" + std::to_string(V) + ")"); return CRF_ERR_ARG; }
    if (den && a.blank != 0) { set_error("a blank other than 0 is for numerator-only calls: a den_lm fixes the blank at 0"); return CRF_ERR_UNSUPPORTED; }
    if (a.time_major && den) { set_error("time-major activations are for numerator-only calls (no den_lm)"); return CRF_ERR_UNSUPPORTED; }
    const HostGraph *h = den ? a.g->h : nullptr;
    if (den && V <= h->dev.max_label) {
        set_error("den_lm has label " + std::to_string(h->dev.max_label) + " but log_probs has only V=" + std::to_string(V) + " classes");
        return CRF_ERR_ARG;
    }
    if (V > kMaxVocab) { set_error("V > " + std::to_string(kMaxVocab) + " not supported by this build"); return CRF_ERR_UNSUPPORTED; }
    const int Sc = rup64((int)(2 * (ctc ? a.max_label_len : 0) + 1));
    if (ctc && a.max_label_len > kMaxCtcLabelLen) { set_error("label length > " + std::to_string(kMaxCtcLabelLen) + " not supported by this build"); return CRF_ERR_UNSUPPORTED; }
    const DenFamily fam = choose_den_family(h, B, V);
    w = ws_layout(fam, h, B, T, V, Sc);
    if (a.ws_bytes < w.total) { set_error("workspace too small: need " + std::to_string(w.total)); return CRF_ERR_WORKSPACE; }
    pl = plan_kernels(h, fam, V, a.max_label_len, Sc, den, ctc);
    if (fam.fac() && T * std::max<int64_t>(V, std::max(fam.Rq, fam.Rb)) >= ((int64_t)1 << 32)) {   // (the factored frame loop adds 32-bit row offsets)
        set_error("T * max(V, row length) >= 2^32 not supported by the factored kernels"); return CRF_ERR_UNSUPPORTED;
    }
    if (std::max(pl.lds_den, ctc ? pl.lds_ctc : 0) > 160 * 1024 || pl.lds_grad > 160 * 1024) {
        set_error("graph too large for this build (states=" + std::to_string(h ? h->S : 0) + ")");
        return CRF_ERR_UNSUPPORTED;
    }
    return CRF_OK;
}

static void plan_schedule(CallPlan &pl, int64_t B, int64_t T, const DevFacts &f) {
    pl.ncu = f.ncu; pl.have_flags = f.have_flags;
    pl.serial = opt_on(kOpt_serial_chains) || !f.have_side;              // no side stream: everything in order on the caller's stream
    // Factored den kernels: 2B workgroups, one CU each.  While that is at most half of the chip, everything else
    // runs BESIDE them on the other half, on the side stream: numerator chains, their grad half, and the den half of
    // the grad pass.  The den half of the grad pass needs rows of BOTH recursions, which work towards each other; it
    // is released in stages: the recursions bump a counter at every stage bound, the grad launch of stage k is queued
    // behind a STREAM-level wait on that counter and takes the 16-frame blocks the stage completed.
    // (A grad pass that SPINS on progress counters of the running den kernels is faster still on a quiet device,
    // but with many launches queued ahead the den kernels were observed to stop for seconds while the waiting
    // workgroups kept their queue busy -- one kernel must never wait for another.)
    pl.no_overlap = opt_on(kOpt_no_overlap);   // diagnostics
    // how stage k of the grad pass is released: a stream-level wait on a counter the running recursions bump
    // (default), or -- CRF_SEGMENTS=1, and automatically if hipStreamWaitValue32 is refused -- by cutting the
    // recursions into one launch per stage with an event after each (~40 us per relaunch, state parked in HBM)
    pl.segmode = f.segments || opt_on(kOpt_segments);
    const int stages_env = opt(kOpt_stages, 0);
    const int pieces = stages_env > 0 ? stages_env : (pl.segmode ? 4 : 12);   // measured: 4 / 8 / 12 pieces -> call 4.06 / 3.98 / 3.93 ms (flags)
    pl.den_wgs = pl.fam.pair2() ? 2 * ((B + 1) / 2) : 2 * B;
    // (the two-utterance kernel has no segment relaunches: where stream-level waits are refused it runs unstaged)
    pl.staged = pl.fam.fac() && pl.fam.FX->K == 1 && pl.ctc && pl.fast_den && pl.fast_ctc && !pl.serial && !pl.no_overlap && f.have_flags && !(pl.fam.pair2() && pl.segmode) && pl.den_wgs * 100 <= (int64_t)f.ncu * kStageFill;   // (B = 80: 4.16 -> 3.56 ms, B = 96: 4.37 -> 4.26, B = 112 at 90 %: 5.33 -> 5.57)
    // Stage bounds.  Nothing can be released before the two recursions have met, so the first stage ends at half of
    // the frames or later; after that a piece of `piece` iterations releases 2 * piece / 16 frame blocks per
    // utterance.  The grad pass has half of the chip and is bandwidth-bound there (~2 TB/s against the 2.2 TB/s the
    // two recursions produce), with a fixed cost per stage (launch, the workgroups' set-up, partial rounds); what is
    // left when the recursions end is its backlog plus the last stage.  Measured (B=64, T=1500, recursions 2.95 ms):
    // pieces of 32 / 48 / 64 / 96 / 128 / 192 / 256 / 384 iterations -> step 3.88 / 3.62 / 3.42 / 3.38 / 3.33 / 3.35 /
    // 3.41 / 3.53 ms; pieces that shrink towards the end (256,192,128,96,64 ...) were no better than equal ones.
    // CRF_PIECE / CRF_STAGES override (segment mode: 4 pieces, each relaunch costs ~40 us).
    pl.stages = StagePlan{};   // one stage: everything behind the recursions
    pl.stages.bound[1] = (int)T;
    // (a context whose one-launch grad pass has timed out goes back to one grad launch per stage: DevCtx::gd_fallback)
    pl.per_stage = opt_on(kOpt_gd_stage_launches) || f.gd_fallback;
    if (pl.staged && T >= 256) pl.stages = plan_grad_stages(T, pl.segmode, stages_env, pieces, pl.per_stage ? 1 : 0);
    // Did a recent call need the numerator's log-domain fallback?  (the third stream costs the call ~20 us of event traffic whether or not an
    // utterance is marked -- B = 64, T = 1 500: 3.172 -> 3.192 ms -- so it is taken when one of this context's last 16 calls ran the log-domain
    // chains: they write the call's number to a pinned host word, read without any synchronisation, once per call; `aux_stream` 1 / 0 forces
    // it on / off)
    const int aux_env = opt(kOpt_aux_stream, -1);
    pl.ctc_wants_aux = aux_env >= 0 ? aux_env != 0 : (f.seen > 0 && f.call_id - f.seen <= 16);
    // Three streams (round 5, switch grad_par3; OFF): the numerator half of the grad pass (side stream) and the staged den half (third stream)
    // run BESIDE each other and both ADD into gradient rows the prep kernel has zeroed (0 + x + y: two addends per element, the same bits
    // in either order).  The idea: on one stream the stages queue behind the numerator chains and their grad half, and graphs whose
    // recursions are shorter than that (S = 513: recursions 1.25 ms, step 1.92) wait for them.  Measured SLOWER everywhere
    // (profiles/round5_ab_three_streams.txt: metric 2.79 -> 2.85 ms, S = 513 1.92 -> 2.01, V = 217 3.39 -> 3.51, estimated S = 3 006 2.44 -> 2.78):
    // the stage workgroups then share the free CUs with the numerator chains -- a serial fp64 latency chain whose frames get longer -- and
    // what the stages gain by starting early the chains lose.  Not when a recent call needed the numerator's log-domain fallback (the
    // third stream then carries its chains), nor in segment mode.
    pl.par3 = pl.staged && !pl.segmode && f.have_aux && !(pl.robust_env != 0 && pl.ctc_wants_aux) && opt(kOpt_grad_par3, 0) != 0;
}

// the workspace carved into the kernels' parameter block
static LossParams bind_params(const LossArgs &a, const WsLayout &w, const CallPlan &pl, const DevCtx *cx, int call_id) {
    const int64_t B = a.B, T = a.T, V = a.V;
    const HostGraph *h = pl.h;
    const bool den = pl.den, ctc = pl.ctc, res = pl.fam.res(), fac = pl.fam.fac();
    LossParams p{};
    if (den) p.g = h->dev;
    if (pl.fam.FX) p.g.fac = *pl.fam.FX;
    p.logp = a.logp; p.labels = a.labels; p.lab_off = a.lab_off; p.lx = a.lx; p.ly = a.ly;
    p.B = (int)B; p.T = (int)T; p.V = (int)V; p.Sc = pl.Sc;
    p.xs_b = a.time_major ? V : T * V; p.xs_t = a.time_major ? B * V : V;
    p.blank = a.blank;
    p.c_den = a.c_den; p.c_ctc = a.c_ctc;
    char *base = (char *)a.ws;
    p.ep = (float *)(base + w.off(kWs_ep)); p.mx = (float *)(base + w.off(kWs_mx));
    p.fused = a.fused; p.in_dtype = a.in_dtype;
    p.moff = a.fused ? (float *)(base + w.off(kWs_moff)) : p.mx; p.inv_s = (float *)(base + w.off(kWs_invs));
    p.Q = (float *)(base + w.off(kWs_Q)); p.BP = (float *)(base + w.off(kWs_BP));
    p.Rq = (int)pl.fam.Rq; p.Rb = (int)pl.fam.Rb; p.res = fac ? 2 : res ? 1 : 0; p.grad_stage = pl.grad_stage ? 1 : 0;
    if (fac) {
        const FacDev &F = *pl.fam.FX;
        p.gq = F.gq; p.gb = F.gb; p.gchunk = F.chunk_off; p.glab = F.lab_chunk_off; p.gNC = F.NC;
    } else if (den) {
        p.gq = res ? h->dev.res.gq : h->dev.perm; p.gb = res ? h->dev.res.gb : h->dev.perm;
        p.gchunk = res ? h->dev.res.chunk_off : h->dev.chunk_off; p.glab = res ? h->dev.res.lab_chunk_off : h->dev.lab_chunk_off;
        p.gNC = res ? h->dev.res.NC : h->dev.NC;
    }
    if (res && !fac) { p.res_lds_rows_f = h->res_rows_cu_f; p.res_lds_rows_b = h->res_rows_cu_b; }
    p.EQ = (int *)(base + w.off(kWs_EQ)); p.EB = (int *)(base + w.off(kWs_EB));
    p.CA = (double *)(base + w.off(kWs_CA)); p.CB = (double *)(base + w.off(kWs_CB));
    p.ECA = (int *)(base + w.off(kWs_ECA)); p.ECB = (int *)(base + w.off(kWs_ECB));
    const auto pb = [&](PbField k) { return (void *)(base + w.off(kWs_pb) + fields_off(kPbFields, k, B)); };   // (CRF_PB_FIELDS)
    p.ctc_zc = (double *)pb(kPb_ctc_zc); p.cb_mxs = (double *)pb(kPb_cb_mxs);
    p.cb_part = (float *)pb(kPb_cb_part); p.cb_F = (int *)pb(kPb_cb_F);
    p.redo = (int *)pb(kPb_redo); p.redo_ctc = (int *)pb(kPb_redo_ctc); p.ctc_logdom = (int *)pb(kPb_ctc_logdom);
    p.ctc_bad = (int *)(base + w.off(kWs_cbad));
    p.force_redo = (den && pl.robust_env == 1) ? 1 : 0;
    p.force_redo_ctc = (ctc && (pl.robust_env == 1 || opt_on(kOpt_robust_ctc))) ? 1 : 0;
    p.ctc_tilt = std::min(400, std::max(0, opt(kOpt_ctc_tilt, 100)));
    p.xch = (unsigned long long *)(base + w.off(kWs_xch));
    p.Row0 = (float *)(base + w.off(kWs_row0));
    p.dump = (float *)(base + w.off(kWs_dump)); p.dump_stride = (int)w.dump_stride;
    p.gvec = (float *)(base + w.off(kWs_gvec));
    p.gvec_stride = w.gvec_stride;
    p.den_zs = (float *)pb(kPb_den_zs); p.den_ez = (int *)pb(kPb_den_ez); p.ctc_ez = (int *)pb(kPb_ctc_ez);
    p.cost_alpha = (float *)pb(kPb_cost_alpha); p.cost_beta = (float *)pb(kPb_cost_beta); p.cost_ctc = (float *)pb(kPb_cost_ctc); p.invalid = (int *)pb(kPb_invalid);
    p.grad = a.grad; p.loss = a.loss; p.out_den = a.costs_den; p.out_beta = a.costs_beta; p.out_ctc = a.costs_ctc;
    p.out_invalid = a.invalid;
    // error word, start counter and stage counters live in fine-grained memory (get_ctx), where the prep kernel clears them; a context
    // without it has the words behind the granules of section xch (CRF_XCH_FIELDS), cleared with the section
    int *const ws_flags = (int *)(base + w.off(kWs_xch) + w.xch_bytes + fields_off(kXchFields, kXch_flags, B));
    p.err = (cx->flags ? cx->flags : ws_flags) + kFlagErr;
    p.clear = cx->flags; p.nclear = cx->flags ? kFlagWords : 0;
    p.call_id = call_id; p.ctc_seen = cx->seen;
    p.gd_timeout_host = cx->hostw ? cx->hostw + 4 : nullptr;
    p.gd_nb = pl.stages.nstage + 1;
    static_assert(sizeof(LossParams::gd_bound) == sizeof(StagePlan::bound) && sizeof(FacParams::bound) == sizeof(StagePlan::bound) &&
                  sizeof(LossParams::gd_poff) == sizeof(GradGrid::poff) && sizeof(LossParams::gd_fpb) == sizeof(GradGrid::fpb), "the parameter blocks hold a whole plan");
    for (int k = 0; k <= pl.stages.nstage; ++k) p.gd_bound[k] = pl.stages.bound[k];   // (the words behind the last bound stay zero)
    p.zero_grad = pl.par3 ? 1 : 0;
    return p;
}

// the utterance-minor kernel is chosen at run time over UL x factored and launched through a pointer (no dynamic LDS: no marks)
static const void *bat_kernel(bool persist, int UL, bool bfac) {
#define CRF_BAT_FN(K) (UL == 64 ? (bfac ? (const void *)K<64, 4, true> : (const void *)K<64, 4, false>)    \
                     : UL == 32 ? (bfac ? (const void *)K<32, 4, true> : (const void *)K<32, 4, false>)    \
                     : UL == 16 ? (bfac ? (const void *)K<16, 4, true> : (const void *)K<16, 4, false>)    \
                                : (bfac ? (const void *)K<8, 4, true> : (const void *)K<8, 4, false>))
    return persist ? CRF_BAT_FN(crf_batch_persist_kernel) : CRF_BAT_FN(crf_batch_frame_kernel);
#undef CRF_BAT_FN
}
static const char *bat_kernel_name(bool persist, int UL, bool bfac) {
    static const char *const kBatNames[2][4][2] = {
        {{"crf_batch_frame_kernel<8,4,false>", "crf_batch_frame_kernel<8,4,true>"}, {"crf_batch_frame_kernel<16,4,false>", "crf_batch_frame_kernel<16,4,true>"},
         {"crf_batch_frame_kernel<32,4,false>", "crf_batch_frame_kernel<32,4,true>"}, {"crf_batch_frame_kernel<64,4,false>", "crf_batch_frame_kernel<64,4,true>"}},
        {{"crf_batch_persist_kernel<8,4,false>", "crf_batch_persist_kernel<8,4,true>"}, {"crf_batch_persist_kernel<16,4,false>", "crf_batch_persist_kernel<16,4,true>"},
         {"crf_batch_persist_kernel<32,4,false>", "crf_batch_persist_kernel<32,4,true>"}, {"crf_batch_persist_kernel<64,4,false>", "crf_batch_persist_kernel<64,4,true>"}}};
    return kBatNames[persist ? 1 : 0][UL == 64 ? 3 : UL == 32 ? 2 : UL == 16 ? 1 : 0][bfac ? 1 : 0];
}

// One call being enqueued.  Two streams at most (three with the context's third stream): the caller's and one side stream of this
// (device, caller stream)'s context.  Forward and backward recursions are one grid each (denominator pair, numerator pair); the two grids
// are independent.
struct LossCall {
    const LossArgs &a;
    const WsLayout &w;
    const CallPlan &pl;
    DevCtx *cx;
    hipStream_t stream, side;   // side == stream: everything in order on the caller's stream
    LossParams p;
    bool forked = false, side_used = false;
    bool ctc_pass1 = false;   // the numerator's log-domain fallback has run in this call (staged schedule)

    int *started() const { return p.err + kFlagStarted; }   // workgroups of the den kernels that hold a CU (cleared with the error word)
    // factored recursions launched in segments park their state vectors here
    float *fstate() const { return (float *)((char *)a.ws + w.off(kWs_state)); }
    float *bstate() const { return fstate() + a.B * w.state_stride; }

    int fork_side() {   // the side stream starts behind everything queued on the caller's stream so far
        if (pl.serial || forked) return CRF_OK;
        if (const int rc = wait_behind(side, cx->fork, stream, "fork")) return rc;
        forked = side_used = true;
        if (g_call_streams < 2) g_call_streams = 2;
        return CRF_OK;
    }
    int join_side() {   // the caller's stream continues behind everything queued on the side stream so far
        if (pl.serial || !side_used) return CRF_OK;
        if (const int rc = wait_behind(stream, cx->join, side, "join")) return rc;
        forked = false;
        return CRF_OK;
    }
    // stream `waiter` continues behind what is queued on `on` so far, through event `ev`
    static int wait_behind(hipStream_t waiter, hipEvent_t ev, hipStream_t on, const char *what) {
        hipError_t e;
        if ((e = hipEventRecord(ev, on)) != hipSuccess || (e = hipStreamWaitEvent(waiter, ev, 0)) != hipSuccess) {
            set_error(std::string(what) + ": " + hipGetErrorString(e)); return CRF_ERR_HIP;
        }
        return CRF_OK;
    }

    int launch_grad_den(hipStream_t st, int stage, bool persist = false) {
        const int64_t B = a.B, T = a.T, V = a.V;
        p.gd_stage = stage;
        const size_t l = ((size_t)rup64((int)pl.fam.Rq + 1) + rup64((int)pl.fam.Rb + 1) + 4 * rup64((int)V) + kGDFrames + rup64(pl.gnc)) * sizeof(float);
        dim3 gg((unsigned)((T + kGDFrames - 1) / kGDFrames), (unsigned)B);
        p.gd_nf = 0;
        p.gd_persist = 0;
        if (persist) {   // the stages `stage` .. nstage in one launch (see the kernel): 2 * nf candidates per utterance and stage, stage-major
            p.gd_persist = 1;
            p.gd_cnt = cx->flags + kFlagStage;
            p.gd_target = (int)(2 * B);
            const GradGrid grid = plan_grad_grid(pl.stages, stage, B);
            std::copy(grid.poff.begin(), grid.poff.end(), p.gd_poff);
            std::copy(grid.fpb.begin(), grid.fpb.end(), p.gd_fpb);
            gg = dim3((unsigned)grid.workgroups, 1);
        } else if (stage > 1) {   // (stage 1 is the middle of every utterance: all blocks are candidates)
            p.gd_nf = (p.gd_bound[stage] - p.gd_bound[stage - 1] + kGDFrames - 1) / kGDFrames + 3;
            if (2 * p.gd_nf < (int)gg.x) gg.x = (unsigned)(2 * p.gd_nf); else p.gd_nf = 0;
        }
        const char *const name = "crf_grad_den_kernel";
        const dim3 b1(kGDThreads), b2(2 * kGDThreads);
        if (pl.gcap == 8)                // chunk lists cut at 8 entries (many labels with few pairs each): 512 threads, two chunks each
            return launch<crf_grad_den_kernel<2, 2, 2 * kGDThreads, 8>>(name, gg, b2, l, st, p);
        if (pl.gnc > 2 * kGDThreads)     // more than 512 label chunks (graphs over hundreds of classes: V = 500 has ~8 pairs per label,
                                         // one chunk each): 512 threads with two chunks each
            return launch<crf_grad_den_kernel<2, 2, 2 * kGDThreads>>(name, gg, b2, l, st, p);
        if (pl.gd_wide6)                 // rows of 10 241 .. 12 288 floats: 512 threads with six row registers each
            return launch<crf_grad_den_kernel<1, 2, 2 * kGDThreads, kChunk, 6, 1>>(name, gg, b2, l, st, p);
        if (pl.gd_wide && pl.fam.Rq <= 32 * kGDThreads && pl.fam.Rb <= 32 * kGDThreads)
            // rows of 5121 .. 8192 floats: 512 threads with four row registers each, held to 128 VGPRs so that a CU takes TWO workgroups (the
            // five-register form below compiles to 148 VGPRs: one workgroup, eight waves, per CU -- the estimated S = 6836 graph ran on that)
            return launch<crf_grad_den_kernel<1, 2, 2 * kGDThreads, kChunk, 4, 4>>(name, gg, b2, l, st, p);
        if (pl.gd_wide)                  // rows of more than 5120 floats: 512 threads per workgroup (one chunk per thread up to 512 chunks)
            return launch<crf_grad_den_kernel<1, 2, 2 * kGDThreads>>(name, gg, b2, l, st, p);
        if (pl.gnc <= kGDThreads && V <= kGDThreads)   // small vocabulary
            return launch<crf_grad_den_kernel<1, 1>>(name, gg, b1, l, st, p);
        if (pl.gnc <= kGDThreads)
            return launch<crf_grad_den_kernel<1, kGDEpRegs>>(name, gg, b1, l, st, p);
        return launch<crf_grad_den_kernel<2, kGDEpRegs>>(name, gg, b1, l, st, p);
    }
    int launch_grad_generic(int phase, hipStream_t st, const char *name) {
        p.grad_phase = phase;
        return launch<crf_grad_kernel>(name, dim3((unsigned)((a.T + kGradFrames - 1) / kGradFrames), (unsigned)a.B), dim3(kGradThreads), pl.lds_grad, st, p);
    }
    int launch_grad_ctc(int phase, hipStream_t st) {  // phase 2: subtract from the den half; 0: plain CTC (writes)
        if (!pl.fast_ctc) return launch_grad_generic(phase, st, "crf_grad(ctc)");
        p.grad_phase = phase;
        const size_t l = (size_t)4 * rup64((int)a.V) * sizeof(float) + kGCFrames * sizeof(double) + 64;
        const dim3 gg((unsigned)((a.T + kGCFrames - 1) / kGCFrames), (unsigned)a.B);
        const int Sxm = 2 * (int)a.max_label_len + 1;
        if (Sxm <= 2 * kGCThreads) return launch<crf_grad_ctc_kernel<2>>("crf_grad(ctc)", gg, dim3(kGCThreads), l, st, p);
        if (Sxm <= 4 * kGCThreads) return launch<crf_grad_ctc_kernel<4>>("crf_grad(ctc)", gg, dim3(kGCThreads), l, st, p);
        return launch<crf_grad_ctc_kernel<kGCRegs>>("crf_grad(ctc)", gg, dim3(kGCThreads), l, st, p);
    }
    // The grad pass on `st` behind recursions that have ended: the streaming kernels of the halves the call has, else the generic kernel.
    // phase 0: both halves; 1: the den half alone (the caller adds launch_grad_ctc(2) when the numerator's chains have ended too)
    int grad_after_recursions(hipStream_t st, int phase) {
        if (pl.den && pl.fast_den) {
            const int rc = launch_grad_den(st, 0);
            return (rc || phase != 0 || !pl.ctc) ? rc : launch_grad_ctc(2, st);
        }
        if (!pl.den && pl.fast_ctc) return launch_grad_ctc(0, st);
        return launch_grad_generic(phase, st, phase ? "crf_grad_kernel(den)" : "crf_grad_kernel");
    }
    // Numerator fallback: utterances with frames the grad pass marked (or whose scaled chain lost its mass) redo their chains in the
    // log domain, then the marked frames' posteriors are subtracted from the rows; the other utterances' workgroups leave at once --
    // two near-empty launches.  Pass 1 runs right behind the numerator's grad half on the side stream of the staged schedule, i.e.
    // BESIDE the denominator recursions (V = 500: 1.2 ms that followed the call's last grad launch); pass 2 at the end of every call
    // takes what is marked and was not redone in pass 1.
    int launch_robust_ctc_chains(hipStream_t st, int pass) {
        const dim3 grid((unsigned)(2 * a.B)), block(kCtcThreads);
        p.ctc_pass = pass;
        return with_nr(2 * a.max_label_len + 1, kCtcThreads, [&](auto nr, int) {
            return launch<crf_robust_ctc_kernel<decltype(nr)::value>>("crf_robust_ctc_kernel", grid, block, pl.lds_ctc, st, p);
        });
    }
    int launch_robust_ctc_fix(hipStream_t st, int pass) {
        p.ctc_pass = pass;
        return launch<crf_robust_ctc_fix_kernel>("crf_robust_ctc_fix_kernel", dim3((unsigned)((a.T + kGCFrames - 1) / kGCFrames), (unsigned)a.B), dim3(kGradThreads),
                                                 (size_t)rup64((int)a.V) * sizeof(float), st, p);
    }
    int launch_robust_ctc(hipStream_t st, int pass) {
        const int rc = launch_robust_ctc_chains(st, pass);
        return rc ? rc : launch_robust_ctc_fix(st, pass);
    }
    // forward log Z = backward log Z?  (crf_den_check_kernel: behind every launch of the recursions, on their stream -- in the staged schedule
    // it runs while the side stream finishes the grad pass -- and in front of the fallback kernels, which take what it flags)
    int launch_den_check(hipStream_t st) {
        if (!pl.den || pl.robust_env == 0) return CRF_OK;
        return launch<crf_den_check_kernel>("crf_den_check_kernel", dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, st, p, (pl.fam.res() || pl.fam.fac()) ? 1 : 0);
    }
    // the denominator recursions of the whole batch on `st` (every layout; both directions per launch)
    int launch_den(hipStream_t st, bool with_check = true) {
        const int B = (int)a.B;
        const HostGraph *h = pl.h;
        int rc = CRF_OK;
        if (!pl.fam.fac() && !pl.fam.res()) {   // streaming kernels (launch_den_pair marks the profile slots itself)
            rc = pl.fam.gv ? launch_den_pair<true>(p, pl.lds_den, st) : launch_den_pair<false>(p, pl.lds_den, st);
            return (rc || !with_check) ? rc : launch_den_check(st);
        }
        prof_mark(1, false, st); prof_mark(2, false, st);
        {
            const CoresGuard cores((pl.fam.fac() && pl.fam.FX->K > 1) || (pl.fam.res() && !pl.fam.fac() && h->dev.res.K > 1), cx->dev, st);
            if (pl.fam.fac() && pl.fam.FX->K > 1) {
                const int grp = std::max(1, pl.ncu / 4);
                for (int b0 = 0; b0 < B && !rc; b0 += grp) rc = launch_fac2_pair(p, pl.lds_den, st, b0, std::min(grp, B - b0));
            } else if (pl.fam.fac() && pl.fam.pair2()) {
                rc = launch_fac_pair2<false>(p, pl.lds_den, st, started());
            } else if (pl.fam.fac()) {
                rc = launch_fac_pair<false>(p, pl.lds_den, st, started(), 0, (int)a.T, fstate(), bstate());
            } else {
                // K CUs per utterance and direction exchange the state vector through L2 every frame.  With K > 1 every
                // workgroup of a launch must be resident at once (its peers spin on it): groups of at most CUs/(2K) utterances.
                const int K = h->dev.res.K;
                const int grp = K > 1 ? std::max(1, pl.ncu / (2 * K)) : B;
                for (int b0 = 0; b0 < B && !rc; b0 += grp) rc = launch_res_pair(p, pl.lds_den, b0, std::min(grp, B - b0), st);
            }
            prof_mark(1, true, st); prof_mark(2, true, st);
            if (!rc && with_check) rc = launch_den_check(st);
        }
        return rc;
    }

    // the prep kernel on the caller's stream (e' rows, metadata, the cleared flag words)
    int start() {
        const int64_t frames = a.B * a.T;
        for (bool &u : g_prof.used) u = false;
        prof_mark(7, false, stream);
        prof_mark(0, false, stream);
        const int rc = a.V <= 256 ? launch<crf_prep_kernel<16>>("crf_prep_kernel", dim3((unsigned)((frames + 15) / 16)), dim3(256), 0, stream, p)
                                  : launch<crf_prep_kernel<64>>("crf_prep_kernel", dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, stream, p);
        prof_mark(0, true, stream);
        if (rc) return rc;
        if (pl.fam.res() && (w.xch_bytes > 0 || !pl.have_flags)) {  // exchange granules (tags) and the error word start at zero in every call
            if (hipMemsetAsync(p.xch, 0, (size_t)w.sec[kWs_xch].bytes, stream) != hipSuccess) { set_error("hipMemsetAsync(xch)"); return CRF_ERR_HIP; }
        }
        return CRF_OK;
    }

    int run_batch();
    int run_staged();
    int run_staged_par3();
    int run_two_streams();
    int run_one_stream();
    int run_fallbacks_and_finalize();
};

// Utterance-minor denominator (large graphs): one launch per frame on the caller's stream, forward step of
// frame j and backward step of frame T - j together; the numerator pair runs beside them on the side stream.
int LossCall::run_batch() {
    const int64_t B = a.B, T = a.T, V = a.V;
    const HostGraph *h = pl.h;
    char *base = (char *)a.ws;
    int rc;
    hipError_t e;
    BatchParams bp{};
    bp.g = h->dev.bat; bp.start_lin = h->dev.start_lin; bp.end_lin = h->dev.end_lin;
    bp.S = h->dev.S; bp.P = h->dev.P; bp.B = (int)B; bp.Bp = (int)pl.fam.Bp; bp.T = (int)T; bp.V = (int)V; bp.max_label = h->dev.max_label;
    bp.lx = a.lx; bp.ep = p.ep; bp.moff = p.moff;
    bp.ept = (float *)(base + w.off(kWs_ept)); bp.Af = (float *)(base + w.off(kWs_Af)); bp.Zb = (float *)(base + w.off(kWs_Zb));
    bp.Q = p.Q; bp.BP = p.BP;
    const auto bsm = [&](BsmField k) { return (void *)(base + w.off(kWs_bsm) + fields_off(kBsmFields, k, pl.fam.Bp)); };   // (CRF_BSM_FIELDS)
    bp.mxf = (unsigned *)bsm(kBsm_mxf); bp.mxb = (unsigned *)bsm(kBsm_mxb); bp.Ef = (int *)bsm(kBsm_Ef); bp.Fb = (int *)bsm(kBsm_Fb);
    bp.zs = (float *)bsm(kBsm_zs); bp.zb = (float *)bsm(kBsm_zb);
    bp.bar = (unsigned *)bsm(kBsm_bar); bp.err = (int *)(bp.bar + kBatBarWords);
    bp.den_zs = p.den_zs; bp.cost_alpha = p.cost_alpha; bp.cost_beta = p.cost_beta; bp.den_ez = p.den_ez; bp.redo = p.redo;
    bp.grad = a.grad; bp.c_den = a.c_den;
    const unsigned ngrp = (unsigned)(pl.fam.Bp / pl.fam.UL);
    bp.ngrp = (int)ngrp;
    // one task per wave, ONE round of workgroups (a second round with a fraction of the device doubled the launch):
    // the tasks wanted per direction follow from the occupancy the runtime reports, shared by the combos
    const int64_t ncombo = 2 * (int64_t)ngrp;
    const bool bfac = stream_fac(a.g->h, pl.fam.UL);                  // factored streams (T o LM graphs, groups of >= 32 utterances)
    // ALL frames in one persistent launch (round 6) when its grid is co-resident by the runtime's own count -- switch bat_persist: 0 =
    // one launch per frame (rounds 2 - 5; also the fallback), 1 = persistent (default)
    const bool want_persist = opt(kOpt_bat_persist, 1) != 0;
    int wg_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg_cu, bat_kernel(want_persist, pl.fam.UL, bfac), kBatThreads, 0) != hipSuccess || wg_cu < 1) { (void)hipGetLastError(); wg_cu = want_persist ? 0 : 2; }
    bool persist = want_persist && wg_cu >= 1;
    if (want_persist && !persist) wg_cu = 2;
    // ... times 70 %: a launch is bound by the L2s and the fabric, not by the CUs, and fewer, longer tasks pay the task set-up
    // (three dependent trips to a cold L2) less often.  Measured, S = 16 385 / B = 64 (repeatable to 0.3 %): 100 / 85 / 70 /
    // 60 / 55 / 45 / 35 % -> 30.7 / 29.5 / 28.8 / 30.6 / 31.8 / 28.5 / 31.3 ms per step (the dips: workgroups per XCD just
    // above a multiple of its 32 CUs); config #5 at B = 8: 100 / 70 / 50 % -> 145.3 / 143.6 / 152.6 ms.  CRF_BAT_FILL overrides.
    const int fill_env = opt(kOpt_bat_fill, 0);
    const int64_t fill = fill_env > 0 && fill_env <= 100 ? fill_env : 70;
    const int64_t slots = (int64_t)pl.ncu * wg_cu;            // workgroups the device holds at once
    const int want = (int)std::max<int64_t>(16, (int64_t)pl.ncu * wg_cu * kBatWaves * 15 / 16 * fill / 100 / ncombo);
    const StreamDev *sdv = nullptr;
    if ((rc = ensure_stream_tables(a.g->h, pl.fam.UL, want, &sdv))) return rc;
    if ((sdv->fac != 0) != bfac) { set_error("arc streams: factored / plain mismatch"); return CRF_ERR_ARG; }
    bp.SX = h->dev.S + sdv->NU; bp.x_start = sdv->x_start;
    bp.st = *sdv;
    // 8 * nslot workgroups (block b -> XCD b % 8, slot b / 8): every combo gets at least one wave per task of its arc
    // stream (crf_batch_frame_kernel: a combo has nslot * nk or about nslot / ncx workgroups)
    const int64_t tasks_max = std::max({(int64_t)sdv->f.ntasks, (int64_t)sdv->b.ntasks, (int64_t)1});
    const int64_t wg_combo = (tasks_max + kBatWaves - 1) / kBatWaves + ((sdv->f.nrest > 64 || sdv->b.nrest > 64) ? (std::max(sdv->f.nrest, sdv->b.nrest) + 4 * kBatWaves - 1) / (4 * kBatWaves) : 0);
    const unsigned nslot = (unsigned)(ncombo < 8 ? (wg_combo + (8 / ncombo) - 1) / (8 / ncombo) : wg_combo * ((ncombo + 7) / 8));
    const unsigned G = 8 * nslot;
    if (persist && (int64_t)G > slots) persist = false;        // (the grid barrier needs every workgroup resident)
    // The numerator chains run BESIDE the per-frame launches (side stream) but BEHIND the persistent launch, beside the grad pass: a
    // co-resident grid sized for the device's slots must not share them -- with the chains' 2 B workgroups on the CUs, G = 416 of 512
    // slots no longer fitted at once (S = 12 289, B = 64: a CU that holds a chain workgroup has LDS for one workgroup of this kernel,
    // not two), the rest of the grid waited for the chains, and the runtime time-sliced the queues: 1.7 ms per frame instead of 13 us
    // and barrier time-outs (profiles/round6_ab_persistent_batch.txt)
    if (pl.ctc && !persist) {
        if ((rc = fork_side())) return rc;
        if ((rc = launch_ctc_pair(p, pl.lds_ctc, side, a.max_label_len))) return rc;
    }
    if (opt_on(kOpt_verbose)) fprintf(stderr, "[ctc_crf_hip] utterance-minor: UL %d, %d combos, tasks %d / %d, rest rows %d / %d, grid %u of %lld slots (%d per CU), %s\n", (int)pl.fam.UL, (int)ncombo,
                                      sdv->f.ntasks, sdv->b.ntasks, sdv->f.nrest, sdv->b.nrest, G, (long long)slots, wg_cu, persist ? "one persistent launch" : "one launch per frame");
    prof_mark(1, false, stream); prof_mark(2, false, stream);
#define CRF_BAT_UL(KERNEL, GRID, ...)                                                                          \
    (pl.fam.UL == 64   ? launch<KERNEL<64>>(#KERNEL, GRID, dim3(kBatThreads), 0, stream, __VA_ARGS__)                \
     : pl.fam.UL == 32 ? launch<KERNEL<32>>(#KERNEL, GRID, dim3(kBatThreads), 0, stream, __VA_ARGS__)                \
     : pl.fam.UL == 16 ? launch<KERNEL<16>>(#KERNEL, GRID, dim3(kBatThreads), 0, stream, __VA_ARGS__)                \
                  : launch<KERNEL<8>>(#KERNEL, GRID, dim3(kBatThreads), 0, stream, __VA_ARGS__))
    if ((rc = CRF_BAT_UL(crf_batch_transpose_kernel, dim3((unsigned)((V + 63) / 64), (unsigned)T, ngrp), bp))) return rc;
    if ((rc = launch<crf_batch_init_kernel>("crf_batch_init_kernel", dim3((unsigned)(((int64_t)bp.SX * pl.fam.Bp + kBatThreads - 1) / kBatThreads)), dim3(kBatThreads), 0, stream, bp))) return rc;
    g_den_kernel = bat_kernel_name(persist, pl.fam.UL, bfac);
    {
        void *args[] = {(void *)&bp};
        const void *fn = bat_kernel(persist, pl.fam.UL, bfac);
        if (persist) {
            // (co-resident grids of two callers must not interleave: each could become partially resident and wait for the rest)
            CoresGuard guard(true, cx->dev, stream);
            bp.j = 0;
            if ((e = hipLaunchKernel(fn, dim3(G), dim3(kBatThreads), args, 0, stream)) != hipSuccess) { set_error(std::string("crf_batch_persist_kernel: ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
        } else {
            for (int j = 0; j <= (int)T; ++j) {   // (4: batches of gathers in flight per wave; 2 measured 6 % slower, 8 needs more registers than a wave has)
                bp.j = j;
                if ((e = hipLaunchKernel(fn, dim3(G), dim3(kBatThreads), args, 0, stream)) != hipSuccess) { set_error(std::string("crf_batch_frame_kernel: ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
            }
        }
    }
    if (pl.ctc && persist) {
        if ((rc = fork_side())) return rc;
        if ((rc = launch_ctc_pair(p, pl.lds_ctc, side, a.max_label_len))) return rc;
    }
    if ((rc = CRF_BAT_UL(crf_batch_zsum_kernel, dim3((unsigned)((h->dev.S + 255) / 256), 1, ngrp), bp))) return rc;
    if ((rc = launch<crf_batch_cost_kernel>("crf_batch_cost_kernel", dim3((unsigned)B), dim3(kBatThreads), 0, stream, bp))) return rc;
    prof_mark(1, true, stream); prof_mark(2, true, stream);
    if ((rc = launch_den_check(stream))) return rc;
    prof_mark(5, false, stream);
    if ((rc = CRF_BAT_UL(crf_batch_grad_kernel, dim3((unsigned)T, 1, ngrp), bp))) return rc;
#undef CRF_BAT_UL
    if ((rc = join_side())) return rc;
    if (pl.ctc && (rc = launch_grad_ctc(2, stream))) return rc;
    prof_mark(5, true, stream);
    return CRF_OK;
}

// Staged: caller's stream: the denominator pair.  Side stream, behind a short bounded start gate: numerator pair, its
// grad half (writes -c_ctc * gamma_ctc), then the den half of the grad pass stage by stage (adds gamma_den).
int LossCall::run_staged() {
    const int64_t B = a.B;
    const int nstage = pl.stages.nstage;
    int *const stage_cnt = cx->flags + kFlagStage;
    int rc;
    hipError_t e;
    if ((rc = fork_side())) return rc;
    prof_mark(1, false, stream); prof_mark(2, false, stream);
    if (pl.fam.pair2()) {
        if ((rc = launch_fac_pair2<true>(p, pl.lds_den, stream, started(), nstage + 1, pl.stages.bound.data(), stage_cnt))) return rc;
    } else if (!pl.segmode) {
        if ((rc = launch_fac_pair<true>(p, pl.lds_den, stream, started(), 0, (int)a.T, fstate(), bstate(), nstage + 1, pl.stages.bound.data(), stage_cnt))) return rc;
    } else {
        for (int k = 0; k < nstage; ++k) {
            if ((rc = launch_fac_pair<false>(p, pl.lds_den, stream, started(), pl.stages.bound[k], pl.stages.bound[k + 1], fstate(), bstate()))) return rc;
            if ((e = hipEventRecord(cx->ev[k], stream)) != hipSuccess) { set_error(std::string("hipEventRecord(segment): ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
        }
    }
    prof_mark(1, true, stream); prof_mark(2, true, stream);
    if ((rc = launch_den_check(stream))) return rc;
    // hold the numerator back (briefly, bounded) until the den workgroups have their CUs
    if ((rc = launch<crf_gate_kernel>("crf_gate_kernel", dim3(1), dim3(1), 0, side, started(), (int)pl.den_wgs))) return rc;
    if ((rc = launch_ctc_pair(p, pl.lds_ctc, side, a.max_label_len))) return rc;
    prof_mark(5, false, side);
    if ((rc = launch_grad_ctc(pl.par3 ? 3 : 0, side))) return rc;
    if (pl.par3) return run_staged_par3();
    // Numerator fallback, pass 1.  The chains of the marked utterances can take as long as the scaled ones did (T = 3 000, L = 500,
    // every utterance marked: 3 ms): on the third stream they run beside the grad stages instead of in front of them, and the
    // marked frames' posteriors are subtracted behind the last stage (the stages ADD gamma_den: the order does not matter).
    // Enqueued BEFORE the stage waits of the side stream: whatever hardware queues the three streams share, the chains' packets
    // precede the wait for their event.
    bool aux_fix = false;
    ctc_pass1 = pl.robust_env != 0;
    if (pl.robust_env != 0) {
        // (the third stream is taken when a recent call of this context ran the log-domain chains: CallPlan::ctc_wants_aux)
        if (cx->aux && pl.ctc_wants_aux && hipEventRecord(cx->ev_a, side) == hipSuccess && hipStreamWaitEvent(cx->aux, cx->ev_a, 0) == hipSuccess) {
            if ((rc = launch_robust_ctc_chains(cx->aux, 1))) return rc;
            if ((e = hipEventRecord(cx->ev_b, cx->aux)) != hipSuccess) { set_error(std::string("hipEventRecord(aux): ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
            aux_fix = true;
            g_call_streams = 3;
        } else {
            (void)hipGetLastError();
            if ((rc = launch_robust_ctc_chains(side, 1))) return rc;
        }
    }
    p.grad_den_acc = 1;
    // (one launch for the stages 2 ..: behind stage 1's wait -- every recursion has run half of its frames, every den workgroup is resident)
    const bool gd_one = !pl.segmode && nstage >= 3 && !pl.per_stage;
    for (int k = 0; k < nstage; ++k) {
        if (gd_one && k == 1) { if ((rc = launch_grad_den(side, 2, true))) return rc; break; }
        if (!pl.segmode) {
            if ((e = hipStreamWaitValue32(side, stage_cnt + k + 1, (uint32_t)(2 * B), hipStreamWaitValueGte, 0xffffffffu)) != hipSuccess) {
                // not available here: from the next call on, segments.  This call: wait for the recursions to END
                (void)hipGetLastError();
                g_use_segments = true;
                if ((rc = wait_behind(side, cx->ev[0], stream, "hipStreamWaitEvent"))) return rc;
            }
        } else if ((e = hipStreamWaitEvent(side, cx->ev[k], 0)) != hipSuccess) {
            set_error(std::string("hipStreamWaitEvent(segment): ") + hipGetErrorString(e)); return CRF_ERR_HIP;
        }
        if ((rc = launch_grad_den(side, k + 1))) return rc;
    }
    // The marked frames' posteriors are subtracted at ONE place whichever stream ran the chains -- behind the last stage -- so that
    // the order of the float additions into `grad` (and with it every bit of the gradient) does not depend on the unsynchronised
    // hint above (round-3 advisor: with the chains on the side stream the subtraction used to precede the stages).
    if (aux_fix && (e = hipStreamWaitEvent(side, cx->ev_b, 0)) != hipSuccess) { set_error(std::string("hipStreamWaitEvent(aux): ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
    if (ctc_pass1 && (rc = launch_robust_ctc_fix(side, 1))) return rc;
    prof_mark(5, true, side);
    return join_side();   // the last grad launch is behind every stage of the recursions
}
// ... with the den half of the grad pass on the THIRD stream (CallPlan::par3), stage by stage behind the same stream-level waits, adding with
// atomics; the side stream goes on with the numerator (fallback chains, if any) and takes the third stream back in behind it
int LossCall::run_staged_par3() {
    int rc;
    hipError_t e;
    if ((e = hipStreamWaitEvent(cx->aux, cx->fork, 0)) != hipSuccess) { set_error(std::string("hipStreamWaitEvent(aux fork): ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
    p.grad_den_acc = 2;
    for (int k = 0; k < pl.stages.nstage; ++k) {
        if ((e = hipStreamWaitValue32(cx->aux, cx->flags + kFlagStage + k + 1, (uint32_t)(2 * a.B), hipStreamWaitValueGte, 0xffffffffu)) != hipSuccess) {
            // not available here: from the next call on, segments (and no third stream).  This call: wait for the recursions to END
            (void)hipGetLastError();
            g_use_segments = true;
            if ((rc = wait_behind(cx->aux, cx->ev[0], stream, "hipStreamWaitEvent"))) return rc;
        }
        if ((rc = launch_grad_den(cx->aux, k + 1))) return rc;
    }
    if ((e = hipEventRecord(cx->ev_b, cx->aux)) != hipSuccess) { set_error(std::string("hipEventRecord(aux): ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
    g_call_streams = 3;
    ctc_pass1 = pl.robust_env != 0;
    if (ctc_pass1 && (rc = launch_robust_ctc_chains(side, 1))) return rc;
    if ((e = hipStreamWaitEvent(side, cx->ev_b, 0)) != hipSuccess) { set_error(std::string("hipStreamWaitEvent(aux): ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
    // (the marked frames' posteriors are subtracted behind BOTH halves: a plain read-modify-write of rows nobody adds to any more)
    if (ctc_pass1 && (rc = launch_robust_ctc_fix(side, 1))) return rc;
    prof_mark(5, true, side);
    return join_side();
}

// Denominator pair on the caller's stream, numerator pair beside it on the side stream -- unless the den
// workgroups own every CU (register-resident layouts with 2B (x K) >= CUs): then the numerator recursions run
// beside the DEN HALF of the grad pass instead (HBM-bound, small workgroups that share CUs happily).
int LossCall::run_two_streams() {
    const HostGraph *h = pl.h;
    int rc;
    const int ctc_after_env = opt(kOpt_ctc_after, -1);
    // (factored, one CU per recursion: the den grid leaves ncu - den_wgs CUs free -- B = 96: 64 of them -- and the numerator
    // chains, four workgroups to a CU, run there beside it, behind the start gate so that the den workgroups get their CUs first)
    const bool fac1 = pl.fam.fac() && pl.fam.FX->K == 1;
    // (round 5: not only when the den grid owns EVERY CU.  Between the staged schedule's limit -- three quarters of the CUs -- and a full device the
    // chains ran beside the recursions on the few CUs they leave, 2 B chain workgroups on 256 - 2 B CUs, and took longer than the recursions: B = 100 /
    // 104 / 112 / 120 4.40 / 4.54 / 4.82 / 5.16 ms per step; behind them, beside the den half of the grad pass: 4.28 / 4.38 / 4.48 / 4.61,
    // profiles/round5_ab_grad_one_launch.txt)
    const bool after = ctc_after_env >= 0 ? ctc_after_env != 0 : fac1 ? pl.den_wgs * 100 > (int64_t)pl.ncu * kStageFill : (pl.fam.res() && h->dev.res.K > 1);
    if (after) {
        // (the consistency check BEHIND the fork: the numerator chains -- a latency chain that wants its workgroups resident at once -- are
        // released by the end of the recursions and get the CUs first; with the check in front of the fork the grad launch below, which
        // follows it on this stream without an event in between, filled the device first: B = 128 ctc chains 1.5 -> 2.4 ms)
        if ((rc = launch_den(stream, false))) return rc;
        if ((rc = fork_side())) return rc;            // numerator pair starts when the den recursions have drained
        if ((rc = launch_den_check(stream))) return rc;
        if ((rc = launch_ctc_pair(p, pl.lds_ctc, side, a.max_label_len))) return rc;
        prof_mark(5, false, stream);
        if ((rc = grad_after_recursions(stream, 1))) return rc;
        if ((rc = join_side())) return rc;
        if ((rc = launch_grad_ctc(2, stream))) return rc;
        prof_mark(5, true, stream);
        return CRF_OK;
    }
    if ((rc = fork_side())) return rc;
    if (fac1 && pl.have_flags) {   // the chains behind the start gate
        if ((rc = launch_den(stream))) return rc;
        if ((rc = launch<crf_gate_kernel>("crf_gate_kernel", dim3(1), dim3(1), 0, side, started(), (int)pl.den_wgs))) return rc;
        if ((rc = launch_ctc_pair(p, pl.lds_ctc, side, a.max_label_len))) return rc;
    } else {
        if ((rc = launch_ctc_pair(p, pl.lds_ctc, side, a.max_label_len))) return rc;
        if ((rc = launch_den(stream))) return rc;
    }
    if ((rc = join_side())) return rc;
    prof_mark(5, false, stream);
    if ((rc = grad_after_recursions(stream, 0))) return rc;
    prof_mark(5, true, stream);
    return CRF_OK;
}

// one stream: den only (gpu_den), numerator only (gpu_ctc / WARP_CTC_LOSS), or no side stream available
int LossCall::run_one_stream() {
    int rc;
    if (pl.den && (rc = launch_den(stream))) return rc;
    if (pl.ctc && (rc = launch_ctc_pair(p, pl.lds_ctc, stream, a.max_label_len))) return rc;
    prof_mark(5, false, stream);
    if ((rc = grad_after_recursions(stream, 0))) return rc;
    prof_mark(5, true, stream);
    return CRF_OK;
}

int LossCall::run_fallbacks_and_finalize() {
    const HostGraph *h = pl.h;
    int rc;
    bool fin_folded = false;
    if (pl.den && pl.robust_env != 0) {
        // Fallback for utterances whose scaled-fp32 recursion lost all its mass: redone in a per-frame log-shifted form
        // (crf_robust_den_kernel).  Workgroups of unflagged utterances leave at once -- two near-empty launches per call.
        const bool rgv = pl.fam.gv_robust;
        const size_t lr = robust_lds_bytes(h, (int)a.V, rgv);
        const dim3 grid((unsigned)(2 * a.B)), block(kChainThreads);
        if ((rc = rgv ? launch<crf_robust_den_kernel<true>>("crf_robust_den_kernel", grid, block, lr, stream, p)
                      : launch<crf_robust_den_kernel<false>>("crf_robust_den_kernel", grid, block, lr, stream, p))) return rc;
        const size_t lg = (size_t)rup64(h->dev.NC) * 4 + (size_t)rup64((int)a.V) * 12 + 64;
        // (the call's sums in this launch unless the numerator's second fallback pass, which rewrites costs, is still to come)
        fin_folded = !(pl.ctc && pl.robust_env != 0 && !ctc_pass1) && !opt_on(kOpt_no_fin_fold) && !g_prof.on;
        p.fin_fold = fin_folded ? 1 : 0;
        rc = launch<crf_robust_grad_kernel>("crf_robust_grad_kernel", dim3(16, (unsigned)a.B), dim3(kGradThreads), lg, stream, p);
        p.fin_fold = 0;
        if (rc) return rc;
    }
    // (the staged schedule's pass 1 ran behind the only kernel that marks frames: nothing is left for a second pass there)
    if (pl.ctc && pl.robust_env != 0 && !ctc_pass1 && (rc = launch_robust_ctc(stream, 2))) return rc;
    prof_mark(6, false, stream);
    rc = fin_folded ? CRF_OK : launch<crf_finalize_kernel>("crf_finalize_kernel", dim3(1), dim3(256), 0, stream, p);
    prof_mark(6, true, stream);
    prof_mark(7, true, stream);
    g_prof.have = g_prof.on;
    return rc;
}

static int loss_impl(const crf_graph *g, const float *logp, int fused, int in_dtype, const int32_t *labels, const int32_t *lab_off,
                     const int32_t *lx, const int32_t *ly, int64_t B, int64_t T, int64_t V,
                     int64_t max_label_len, float c_den, float c_ctc, float *grad, float *loss,
                     float *costs_den, float *costs_beta, float *costs_ctc, int32_t *invalid, void *ws,
                     int64_t ws_bytes, void *stream_, int time_major, int blank) {
    const LossArgs a{g, logp, fused, in_dtype, labels, lab_off, lx, ly, B, T, V, max_label_len, c_den, c_ctc, grad, loss,
                     costs_den, costs_beta, costs_ctc, invalid, ws, ws_bytes, time_major, blank};
    hipStream_t stream = (hipStream_t)stream_;
    WsLayout w{};
    CallPlan pl{};
    int rc;
    if ((rc = check_loss_args(a, w, pl))) return rc;
    DevCtx *cx = nullptr;
    if ((rc = get_ctx(stream, &cx))) return rc;
    std::lock_guard<std::mutex> call_lock(cx->mu);
    reprobe_side(cx, stream);
    DevFacts f;
    f.call_id = ++cx->call_id;
    g_call_streams = 1;
    g_side_desc = cx->side_desc;
    (void)hipDeviceGetAttribute(&f.ncu, hipDeviceAttributeMultiprocessorCount, cx->dev);
    // The one-launch grad pass's workgroups wait inside the kernel for the recursions' stage counters (bounded: ~2 s of wall clock).  A time-out --
    // a den launch that aborted, a device shared with a process whose kernels keep the recursions off their CUs -- is written to a pinned host word;
    // a context that has seen one goes back to one grad launch per stage behind stream-level waits (round 4's schedule: nothing waits on the
    // GPU) for good (round-5 advisor)
    if (cx->hostw && !cx->gd_fallback && ((volatile int *)cx->hostw)[4] != 0) {
        cx->gd_fallback = true;
        fprintf(stderr, "[ctc_crf_hip] the one-launch grad pass timed out waiting for the denominator recursions in an earlier call (its loss was NaN): "
                        "this context now launches the grad pass stage by stage behind stream-level waits\n");
    }
    f.have_flags = cx->flags != nullptr; f.have_side = cx->side != nullptr; f.have_aux = cx->aux != nullptr;
    f.segments = g_use_segments.load(); f.gd_fallback = cx->gd_fallback;
    f.seen = cx->seen ? *(volatile int *)cx->seen : 0;
    plan_schedule(pl, B, T, f);
    LossCall c{a, w, pl, cx, stream, pl.serial ? stream : cx->side, bind_params(a, w, pl, cx, f.call_id)};
    g_last_err_word = c.p.err;
    if ((rc = c.start())) return rc;
    if (pl.fam.bat()) rc = c.run_batch();
    else if (pl.staged) rc = c.run_staged();
    else if (pl.den && pl.ctc && !pl.serial) rc = c.run_two_streams();
    else rc = c.run_one_stream();
    return rc ? rc : c.run_fallbacks_and_finalize();
}

int crf_stage_i32(int32_t *dst_dev, const int32_t *src_pinned_host, int64_t n, void *stream) {
    if (n <= 0) return CRF_OK;
    if (!dst_dev || !src_pinned_host) { set_error("crf_stage_i32: null pointer"); return CRF_ERR_ARG; }
    return launch<crf_stage_i32_kernel>("crf_stage_i32", dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst_dev, src_pinned_host, n);
}

int crf_timing_read(unsigned long long *out, int n) {
#ifdef CRF_TIMING
    if (!out || n <= 0) return 0;
    if (n > 16384) n = 16384;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tm), (size_t)n * sizeof(unsigned long long)) != hipSuccess) return 0;
    return n;
#else
    (void)out; (void)n;
    return 0;  // not a timing build
#endif
}

int crf_last_fallback_counts(int32_t *out2, void *stream) {
    if (!out2) { set_error("crf_last_fallback_counts: null pointer"); return CRF_ERR_ARG; }
    out2[0] = out2[1] = -1;
    if (!g_last_err_word) { set_error("crf_last_fallback_counts: no call in this thread yet"); return CRF_ERR_ARG; }
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(out2, g_last_err_word + kFlagFallback, 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_error(std::string("crf_last_fallback_counts: ") + hipGetErrorString(e)); return CRF_ERR_HIP; }
    return CRF_OK;
}

const char *crf_build_switches(void) {
    return "FAC4_NB=" CRF_STR(CRF_FAC4_NB) " FAC4_NB_ML=" CRF_STR(CRF_FAC4_NB_ML) " FAC5_NB2=" CRF_STR(CRF_FAC5_NB2) " FAC3_NB2=" CRF_STR(CRF_FAC3_NB2)
           " FAC3_NB_F=" CRF_STR(CRF_FAC3_NB_F) " FAC3_NB_B=" CRF_STR(CRF_FAC3_NB_B) " FAC3L_NCH=" CRF_STR(CRF_FAC3L_NCH) " FAC4_NCH=" CRF_STR(CRF_FAC4_NCH)
           " GD_FRAMES=" CRF_STR(CRF_GD_FRAMES)
#ifdef CRF_TIMING
           " TIMING=1"
#endif
        ;
}

const char *crf_last_den_kernel(void) { return g_den_kernel; }
int crf_last_call_streams(void) { return g_call_streams; }
const char *crf_last_side_stream(void) { return g_side_desc; }

void crf_profile_enable(int on) { g_prof.on = on != 0; if (!on) g_prof.have = false; }

int crf_profile_read(float *ms_out, int n) {
    if (!ms_out || n <= 0 || !g_prof.have) return 0;
    int w = 0;
    for (int s = 0; s < 8 && s < n; ++s, ++w) {
        ms_out[s] = -1.f;
        if (!g_prof.used[s]) continue;
        if (hipEventSynchronize(g_prof.ev[2 * s + 1]) != hipSuccess) continue;
        float ms = -1.f;
        if (hipEventElapsedTime(&ms, g_prof.ev[2 * s], g_prof.ev[2 * s + 1]) == hipSuccess) ms_out[s] = ms;
    }
    return w;
}

}  // extern "C"
