// cat_amd/csrc/k_beam_body.h -- THE frame step of the LM-free prefix beam search, a device function on the slots' fields (a BeamSlot in
// the caller's registers): called per frame by crf_beam_search_kernel (k_beam.hip, the whole utterance) and by crf_beam_chunk_kernel
// (k_beam_chunk.hip, a chunk of frames with the beam carried across calls), so any split of an utterance's frames into chunks runs
// the whole call's operations in the whole call's order.  Steps 1 and 2 (beam_frame_merges) are shared with the search under an n-gram LM
// (k_beam_lm_body.h) as well.  The frame's words (vj, cj: pair `lane` of E_t, -inf / -1 for lanes >= C; xb: the blank's value) are the
// caller's, so that it can fetch the next frame's while this one is worked on.
//
// One wave, slot k of the beam in lane k: pb, pnb (fp64, sums as the score gradient takes them: fp64 maximum and result, fp32 exp / log
// of the difference), the prefix' 64-bit id, its parent's id, its last label and its length.  Lane j holds pair j of the frame (C <= 64).
// Per frame:
//   1. each slot looks its last label e up among the C classes (C uniform compares): position and x[e], or none -- the stay's repeat;
//   2. merges: for each live slot k with a parent (a uniform loop over the W slots), the slot whose id is k's parent id gives the mass of
//      its extension by e_k to k's stay and strikes that extension from its own list: W x W id compares a frame, and a prefix that left
//      the beam and came back still finds its child, because the child keeps the parent's ID, not its slot;
//   3. every slot has three candidates: its stay, its extension by e itself (base pb), and the HEAD of its other extensions -- base +
//      x[c] over the frame's sorted list is sorted too, so the list is a 64-bit mask of struck positions and its lowest zero.  W rounds:
//      the lanes' best meet in a wave maximum of the fp64 score (DPP on an order-preserving integer image: no LDS round trip), ties go
//      to a stay, then to the lowest slot; the winner becomes slot r of the new beam -- slot r notes the winner's lane, kind, class and
//      score, and takes its fields from that lane in ONE gather behind the rounds -- and moves on to its next candidate (a new head's
//      class and value come by readlane, the place being uniform).  A maximum of -inf ends the frame: the beam may hold fewer than W.
//   4. the trace word of every slot is stored (parent slot + 64 (class + 1), -1 for an empty slot).
#pragma once
#include "k_beam_common.h"

namespace crf {

// slot `lane` of the beam
struct BeamSlot {
    int alive;
    double pb, pnb;
    beam_u64 id, pid;
    int e, len;
};
// the empty prefix in slot 0, nothing in the others: the start of a search
__device__ __forceinline__ void beam_slot_fresh(BeamSlot &s, int lane) {
    s.alive = lane == 0;
    s.pb = lane == 0 ? 0.0 : -__builtin_huge_val();
    s.pnb = -__builtin_huge_val();
    s.id = 0x243F6A8885A308D3ull; s.pid = 0;
    s.e = -2; s.len = 0;                        // (no last label: -2 matches neither a class nor a filler pair)
}

// what steps 1 and 2 leave of a frame in slot `lane`: the place and value of its last label among the frame's classes (-1, -inf: none),
// tot = lse(pb, pnb), the stay's pb' and pnb' (merges included), the struck places of its extension list, and whether the extension by
// e itself (base pb) is still a candidate
struct BeamFrame {
    int pos;
    float ve;
    double tot, spb, spnb;
    beam_u64 mask;
    bool rep_ok;
};
// steps 1 and 2: acoustic mass only, so the search under an LM takes them as they are (prefixes are label sequences: both sides of a
// merge carry the same lm)
__device__ __forceinline__ BeamFrame beam_frame_merges(const BeamSlot &b, const float vj, const int cj, const float xb, const int lane,
                                                       const int W, const int C) {
    const double kNegInf = -__builtin_huge_val();
    BeamFrame f;
    // 1. the last label among the frame's classes
    f.pos = -1;
    f.ve = -INFINITY;
    for (int j = 0; j < C; ++j) {
        const int c = beam_bcast(cj, j);
        const float v = beam_bcast(vj, j);
        if (c == b.e) { f.pos = j; f.ve = v; }
    }
    f.tot = beam_lse2(b.pb, b.pnb);
    f.spb = b.alive ? (double)xb + f.tot : kNegInf;
    f.spnb = (b.alive && f.pos >= 0) ? (double)f.ve + b.pnb : kNegInf;
    f.mask = C >= 64 ? 0ull : ~0ull << C;                   // struck positions of the extension list
    if (f.pos >= 0) f.mask |= 1ull << f.pos;
    f.rep_ok = b.alive && f.pos >= 0;                       // the extension by e itself: base pb
    // 2. merges into the slots whose parent is in the beam
    double madd = kNegInf;
    for (int k = 0; k < W; ++k) {
        const int kpos = beam_bcast(f.pos, k);
        if (!beam_bcast(b.alive, k) || beam_bcast(b.len, k) == 0 || kpos < 0) continue;    // (uniform)
        const beam_u64 kp = beam_bcast(b.pid, k);
        const int ke = beam_bcast(b.e, k);
        const float kv = beam_bcast(f.ve, k);
        const bool match = b.alive && b.id == kp;
        const beam_u64 bal = __ballot(match);
        if (!bal) continue;
        double contrib = kNegInf;
        if (match) {
            if (ke == b.e) { contrib = (double)kv + b.pb; f.rep_ok = false; }
            else { contrib = (double)kv + f.tot; f.mask |= 1ull << kpos; }
        }
        const double cb = beam_bcast(contrib, __ffsll((long long)bal) - 1);
        if (lane == k) madd = cb;
    }
    f.spnb = beam_lse2(f.spnb, madd);
    return f;
}

// one frame, steps 1 to 4; tr_row: the W trace words of this frame
__device__ __forceinline__ void beam_frame_step(BeamSlot &b, const float vj, const int cj, const float xb, const int lane, const int W,
                                                const int C, int *tr_row) {
    const double kNegInf = -__builtin_huge_val();
    const BeamFrame f = beam_frame_merges(b, vj, cj, xb, lane, W, C);
    const double s_stay = b.alive ? beam_lse2(f.spb, f.spnb) : kNegInf;
    const double s_rep = f.rep_ok ? (double)f.ve + b.pb : kNegInf;
    bool stay_ok = b.alive != 0, rep_ok = f.rep_ok;
    beam_u64 mask = f.mask;
    int h = ~mask ? __ffsll((long long)~mask) - 1 : 64;
    // 3. W rounds of the best candidate; slot r keeps where it came from, the fields follow in one gather behind the rounds
    int hc = __shfl(cj, h & 63);                            // the head of the list: its class and value
    float hv = __shfl(vj, h & 63);
    int src = -1, n_kind = 0, n_c = -1;
    double n_s = kNegInf;
    for (int r = 0; r < W; ++r) {
        const double s_list = (b.alive && h < 64) ? (double)hv + f.tot : kNegInf;
        const double rr = rep_ok ? s_rep : kNegInf;
        const bool rep_first = rr > s_list || (rr == s_list && b.e < hc);
        const double sx = rep_first ? rr : s_list;
        double s = stay_ok ? s_stay : kNegInf;
        int kind = 0;                                       // 0 stay, 1 extension by e, 2 head of the list
        if (sx > s) { s = sx; kind = rep_first ? 1 : 2; }
        const double mx = beam_wave_max(s);
        if (!(mx > kNegInf)) break;                         // (uniform; NaN ends the frame too)
        const bool top = s == mx;
        const beam_u64 bs = __ballot(top && kind == 0);
        const beam_u64 bal = bs ? bs : __ballot(top);
        if (!bal) break;
        const int m = __ffsll((long long)bal) - 1;
        const int c = kind == 0 ? -1 : kind == 1 ? b.e : hc;
        const int b_kind = beam_bcast(kind, m), b_c = beam_bcast(c, m);
        if (lane == r) { src = m; n_kind = b_kind; n_c = b_c; n_s = mx; }
        // the winner moves on to its next candidate (b_kind and the new head's place are uniform: readlanes, no LDS round trip)
        if (b_kind == 2) {
            const beam_u64 nmask = mask | (1ull << (h & 63));
            const int nh = ~nmask ? __ffsll((long long)~nmask) - 1 : 64;
            const int hm = beam_bcast(nh, m);
            const int c2 = beam_bcast(cj, hm & 63);
            const float v2 = beam_bcast(vj, hm & 63);
            if (lane == m) { mask = nmask; h = nh; hc = c2; hv = v2; }
        } else if (lane == m) {
            if (kind == 0) stay_ok = false; else rep_ok = false;
        }
    }
    // 4. the trace row, the new beam: slot r's fields from its parent's lane
    if (lane < W) tr_row[lane] = src >= 0 ? src + 64 * (n_c + 1) : -1;
    {
        const int sl = src >= 0 ? src : lane;
        const double g_spb = __shfl(f.spb, sl), g_spnb = __shfl(f.spnb, sl);
        const beam_u64 g_id = __shfl(b.id, sl), g_pid = __shfl(b.pid, sl);
        const int g_e = __shfl(b.e, sl), g_len = __shfl(b.len, sl);
        const bool st = n_kind == 0;
        const int alive = src >= 0;
        b.alive = alive;
        b.pb = alive && st ? g_spb : kNegInf;
        b.pnb = !alive ? kNegInf : st ? g_spnb : n_s;       // (an extension's pnb' is its score)
        b.id = !alive ? 0ull : st ? g_id : beam_mix(g_id, n_c);
        b.pid = !alive ? 0ull : st ? g_pid : g_id;
        b.e = !alive ? -2 : st ? g_e : n_c;
        b.len = !alive ? 0 : g_len + (st ? 0 : 1);
    }
}

}  // namespace crf
