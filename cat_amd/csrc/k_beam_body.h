// cat_amd/csrc/k_beam_body.h -- one frame of the LM-free prefix beam search as a device function: steps 1 to 4 of k_beam.hip's
// crf_beam_search_kernel (the last label among the frame's classes, the merges, the W rounds of the best candidate, the trace row and
// the new beam), operation for operation, for the kernels that carry a beam across calls (k_beam_chunk.hip).  A COPY: k_beam.hip keeps its
// own text, because calling this function from crf_beam_search_kernel changed that kernel's code (the merge loop's block layout and the
// scalar registers behind it: profiles/beam_chunk_resource_usage.txt), and the whole-utterance kernels stay what they are.  A change of
// the step goes into both; tests/test_gpu_ctc_beam_stream.py holds the copy to the original bit for bit, one frame per call included.
// The slots' fields are the caller's registers; the frame's words (vj, cj: pair `lane` of E_t, -inf / -1 for lanes >= C; xb: the blank's
// value) are the caller's too, so that it can fetch the next frame's while this one is worked on.
#pragma once
#include "k_beam_common.h"

namespace crf {

// slot `lane` of the beam, as crf_beam_search_kernel keeps it
struct BeamSlot {
    int alive;
    double pb, pnb;
    beam_u64 id, pid;
    int e, len;
};
// the empty prefix in slot 0, nothing in the others (k_beam.hip's start)
__device__ __forceinline__ void beam_slot_fresh(BeamSlot &s, int lane) {
    s.alive = lane == 0;
    s.pb = lane == 0 ? 0.0 : -__builtin_huge_val();
    s.pnb = -__builtin_huge_val();
    s.id = 0x243F6A8885A308D3ull; s.pid = 0;
    s.e = -2; s.len = 0;                        // (no last label: -2 matches neither a class nor a filler pair)
}

// tr_row: the W trace words of this frame
__device__ __forceinline__ void beam_frame_step(BeamSlot &b, const float vj, const int cj, const float xb, const int lane, const int W,
                                                const int C, int *tr_row) {
    const double kNegInf = -__builtin_huge_val();
    int alive = b.alive;
    double pb = b.pb, pnb = b.pnb;
    beam_u64 id = b.id, pid = b.pid;
    int e = b.e, len = b.len;
    // 1. the last label among the frame's classes
    int pos = -1;
    float ve = -INFINITY;
    for (int j = 0; j < C; ++j) {
        const int c = beam_bcast(cj, j);
        const float v = beam_bcast(vj, j);
        if (c == e) { pos = j; ve = v; }
    }
    const double tot = beam_lse2(pb, pnb);
    const double spb = alive ? (double)xb + tot : kNegInf;
    double spnb = (alive && pos >= 0) ? (double)ve + pnb : kNegInf;
    beam_u64 mask = C >= 64 ? 0ull : ~0ull << C;           // struck positions of the extension list
    if (pos >= 0) mask |= 1ull << pos;
    bool rep_ok = alive && pos >= 0;                        // the extension by e itself: base pb
    // 2. merges into the slots whose parent is in the beam
    double madd = kNegInf;
    for (int k = 0; k < W; ++k) {
        const int kpos = beam_bcast(pos, k);
        if (!beam_bcast(alive, k) || beam_bcast(len, k) == 0 || kpos < 0) continue;    // (uniform)
        const beam_u64 kp = beam_bcast(pid, k);
        const int ke = beam_bcast(e, k);
        const float kv = beam_bcast(ve, k);
        const bool match = alive && id == kp;
        const beam_u64 bal = __ballot(match);
        if (!bal) continue;
        double contrib = kNegInf;
        if (match) {
            if (ke == e) { contrib = (double)kv + pb; rep_ok = false; }
            else { contrib = (double)kv + tot; mask |= 1ull << kpos; }
        }
        const double cb = beam_bcast(contrib, __ffsll((long long)bal) - 1);
        if (lane == k) madd = cb;
    }
    spnb = beam_lse2(spnb, madd);
    const double s_stay = alive ? beam_lse2(spb, spnb) : kNegInf;
    const double s_rep = rep_ok ? (double)ve + pb : kNegInf;
    bool stay_ok = alive != 0;
    int h = ~mask ? __ffsll((long long)~mask) - 1 : 64;
    // 3. W rounds of the best candidate; slot r keeps where it came from, the fields follow in one gather behind the rounds
    int hc = __shfl(cj, h & 63);                            // the head of the list: its class and value
    float hv = __shfl(vj, h & 63);
    int src = -1, n_kind = 0, n_c = -1;
    double n_s = kNegInf;
    for (int r = 0; r < W; ++r) {
        const double s_list = (alive && h < 64) ? (double)hv + tot : kNegInf;
        const double rr = rep_ok ? s_rep : kNegInf;
        const bool rep_first = rr > s_list || (rr == s_list && e < hc);
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
        const int c = kind == 0 ? -1 : kind == 1 ? e : hc;
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
        const double g_spb = __shfl(spb, sl), g_spnb = __shfl(spnb, sl);
        const beam_u64 g_id = __shfl(id, sl), g_pid = __shfl(pid, sl);
        const int g_e = __shfl(e, sl), g_len = __shfl(len, sl);
        const bool st = n_kind == 0;
        alive = src >= 0;
        pb = alive && st ? g_spb : kNegInf;
        pnb = !alive ? kNegInf : st ? g_spnb : n_s;         // (an extension's pnb' is its score)
        id = !alive ? 0ull : st ? g_id : beam_mix(g_id, n_c);
        pid = !alive ? 0ull : st ? g_pid : g_id;
        e = !alive ? -2 : st ? g_e : n_c;
        len = !alive ? 0 : g_len + (st ? 0 : 1);
    }
    b.alive = alive; b.pb = pb; b.pnb = pnb; b.id = id; b.pid = pid; b.e = e; b.len = len;
}

}  // namespace crf
