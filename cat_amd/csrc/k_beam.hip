// cat_amd/csrc/k_beam.hip -- CTC prefix beam search on the GPU (LM-free): the W best label sequences of every utterance under the prefix
// recursion of include/ctc_crf_hip.h (crf_ctc_beam), with the trace that spells them.  Host side: crf_ctc_beam (crf_host_ctc.hip).
//
// Row stage (crf_beam_row_kernel<E>): one wave per row (n, t), t < lx[n]; 4 rows per workgroup up to kBeamRowsV classes, beyond one.  The
// row is read ONCE into LDS (V words per wave; lane l owns the entries v = l, l + 64, ...; one wave, whose LDS operations complete in
// order: no barrier), with normalize its lse = m + log sum exp(x^ - m) (fp32, each lane its own entries in order, the lanes' sums in
// a butterfly) is taken; then every lane finds the best of its entries once (ascending v: the lowest index of its maximum) and keeps it as a
// key (the value's order-preserving integer image, ~index), and C rounds take the wave maximum of the keys (DPP, no LDS round trip) --
// the largest value at its lowest index: equal values to the lower index -- strike the winner's entry (-inf) and find that lane's next
// best with the whole wave (lane i reads the entries own + 64 i, + 4096, ..: one LDS read per lane instead of a walk over the column by
// one lane; the first version walked every column in every round: 9.8 ms at N = 64, V = 5 000).  Round j gives pair j of E_t;
// where nothing above -inf is left (or only NaN) the pair is (class -1, -inf): an extension at -inf is no candidate, so it changes nothing.
// Workspace: val[n T + t][0] = x^[blank] - lse, val[..][1 + j] = x^[c_j] - lse, cls[..][1 + j] = c_j (cls[..][0] = blank), C + 1 words a row.
//
// Beam stage (crf_beam_search_kernel): ONE wave per utterance, slot k of the beam in lane k, all state in registers: pb, pnb (fp64, sums
// as the score gradient takes them: fp64 maximum and result, fp32 exp / log of the difference), the prefix' 64-bit id, its parent's id,
// its last label and its length.  Lane j holds pair j of the frame (C <= 64); the next frame's C + 1 words are fetched while this frame is
// worked on (unconditional loads, frame and lane clamped).  Per frame:
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
// Back-trace, same launch behind a barrier: the trace rows come back through LDS 64 frames at a time, lane r < nbest follows rank r from
// frame lx - 1 down and stores a label wherever a class was appended (its length is known: the labels land at their final places), then
// the tails take the blank, and with a caller's trace buffer the rows t >= lx take -1.  Every output word is written by one plain store.
#include "k_beam_common.h"   // the wave helpers, shared with k_beam_lm.hip

namespace crf {

template <typename E>
__global__ __launch_bounds__(256) void crf_beam_row_kernel(BeamParams p) {
    extern __shared__ float beam_rows[];       // [waves of the workgroup][V]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, R = blockDim.x >> 6;
    const int64_t f = (int64_t)blockIdx.x * R + w;
    if (f >= (int64_t)p.B * p.T) return;       // (no barrier in this kernel: waves leave on their own)
    const int n = (int)(f / p.T), t = (int)(f % p.T);
    if (t >= p.lx[n]) return;
    const int V = p.V, C = p.C, RS = C + 1;
    const E *row = (const E *)p.x + ((int64_t)n * p.xs_b + (int64_t)t * p.xs_t);
    float *xr = beam_rows + (size_t)w * V;
    float m = -INFINITY;
#pragma unroll 4
    for (int v = lane; v < V; v += 64) {
        const float x = lat_ld<E>((const char *)(row + v));
        xr[v] = x;
        m = fmaxf(m, x);
    }
    const float xb = lat_ld<E>((const char *)(row + p.blank));
    float lse = 0.f;
    if (p.normalize) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (m == -INFINITY) m = 0.f;
        float s = 0.f;
        for (int v = lane; v < V; v += 64) s += expf(xr[v] - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        lse = m + logf(s);
    }
    if (lane == (p.blank & 63)) xr[p.blank] = -INFINITY;   // the blank is no class of E_t
    // every lane's best entry as a key (value image, ~index): the wave maximum of the keys is the largest value at its lowest index
    unsigned kh, kl;
    {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = lane; v < V; v += 64) {
            const float x = xr[v];
            if (x > bv) { bv = x; bi = v; }    // (ascending v: the lowest index of the lane's maximum; NaN never wins)
        }
        kh = beam_ord(bv); kl = ~(unsigned)bi;
    }
    float myv = -INFINITY;
    int myc = -1;
    for (int j = 0; j < C; ++j) {
        const unsigned mh = beam_wave_umax(kh);
        if (mh <= kBeamOrdNegInf) break;       // (uniform) nothing above -inf is left: the remaining pairs stay (-inf, -1)
        const int bi = (int)~beam_wave_umax(kh == mh ? kl : 0u);
        if (lane == j) { myv = beam_unord(mh) - lse; myc = bi; }
        // the winner's entry is struck, and its lane's next best found by the whole wave: lane i looks at the entries own + 64 i
        // (+ 4096, ..) of that lane's column -- one conflicted LDS read instead of a walk over the column by one lane
        const int own = bi & 63;
        if (lane == own) xr[bi] = -INFINITY;
        float cv = -INFINITY;
        int ci = 0x7fffffff;
        for (int v = own + 64 * lane; v < V; v += 4096) {
            const float x = xr[v];
            if (v != bi && x > cv) { cv = x; ci = v; }
        }
        const unsigned ch = beam_ord(cv), cl = ~(unsigned)ci;
        const unsigned nh = beam_wave_umax(ch);
        const unsigned nl = beam_wave_umax(ch == nh ? cl : 0u);
        if (lane == own) { kh = nh; kl = nl; }
    }
    float *val = p.val + f * RS;
    int *cls = p.cls + f * RS;
    if (lane < C) { val[1 + lane] = myv; cls[1 + lane] = myc; }
    if (lane == 63) { val[0] = xb - lse; cls[0] = p.blank; }
}

__global__ __launch_bounds__(64) void crf_beam_search_kernel(BeamParams p) {
    __shared__ int tr_lds[64 * kBeamMaxW];     // 64 frames of the trace for the back-trace
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = p.T, W = p.W, C = p.C, RS = C + 1;
    const int lx = max(0, min(p.lx[b], T));
    const double kNegInf = -__builtin_huge_val();
    const float *val = p.val + (int64_t)b * T * RS;
    const int *cls = p.cls + (int64_t)b * T * RS;
    int *tr = p.trace + (int64_t)b * T * W;
    const int jl = C > 0 ? 1 + min(lane, C - 1) : 0;   // this lane's word of a row (lanes >= C: clamped, not used)

    // the beam: the empty prefix in slot 0
    int alive = lane == 0;
    double pb = lane == 0 ? 0.0 : kNegInf, pnb = kNegInf;
    beam_u64 id = 0x243F6A8885A308D3ull, pid = 0;
    int e = -2, len = 0;                        // (no last label: -2 matches neither a class nor a filler pair)

    float nv = 0.f, nxb = 0.f;
    int nc = -1;
    if (lx > 0) { nv = val[jl]; nc = cls[jl]; nxb = val[0]; }
    for (int t = 0; t < lx; ++t) {
        const float vj = lane < C ? nv : -INFINITY, xb = nxb;
        const int cj = lane < C ? nc : -1;
        {
            const int64_t o = (int64_t)min(t + 1, lx - 1) * RS;
            nv = val[o + jl]; nc = cls[o + jl]; nxb = val[o];
        }
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
        if (lane < W) tr[(int64_t)t * W + lane] = src >= 0 ? src + 64 * (n_c + 1) : -1;
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
    }

    // results of the ranks, back-trace
    const bool out = lane < p.nbest;
    const int olen = alive ? len : 0;
    const int64_t h0 = (int64_t)b * p.nbest;
    if (out) {
        p.score[h0 + lane] = alive ? (float)beam_lse2(pb, pnb) : -INFINITY;
        p.hyp_len[h0 + lane] = olen;
    }
    int *hyp = p.hyps + (h0 + (out ? lane : 0)) * T;
    int slot = lane, at = olen;
    for (int t1 = lx; t1 > 0; t1 -= 64) {
        const int t0 = max(0, t1 - 64), nw = (t1 - t0) * W;
        __syncthreads();                        // (the trace rows are this wave's own stores; the chunk before has been read)
        for (int i = lane; i < nw; i += 64) tr_lds[i] = tr[(int64_t)t0 * W + i];
        __syncthreads();
        if (out && alive) {
            for (int t = t1 - 1; t >= t0; --t) {
                const int wd = tr_lds[(t - t0) * W + slot];
                const int c = (wd >> 6) - 1;
                slot = min(wd & 63, W - 1);     // (a live slot's word is never -1; the clamp keeps any word inside the row)
                if (c >= 0 && at > 0) hyp[--at] = c;
            }
        }
    }
    for (int r = 0; r < p.nbest; ++r) {
        const int L = beam_bcast(olen, r);
        int *row = p.hyps + (h0 + r) * T;
        for (int j = L + lane; j < T; j += 64) row[j] = p.blank;
    }
    if (p.fill_trace)
        for (int64_t i = (int64_t)lx * W + lane; i < (int64_t)T * W; i += 64) tr[i] = -1;
}

template __global__ void crf_beam_row_kernel<float>(BeamParams);
template __global__ void crf_beam_row_kernel<AlnBf16>(BeamParams);
template __global__ void crf_beam_row_kernel<AlnF16>(BeamParams);

}  // namespace crf
