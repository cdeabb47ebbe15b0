// cat_amd/csrc/k_ctct.hip -- the CTC-Transducer (CTC-T) loss and its gradient (include/ctc_crf_hip.h crf_ctct_loss / crf_ctct_grad; host side:
// crf_host_ctc.hip): the second topology of cat/rnnt/train.py's forward().  A path labels EVERY frame with one class, blanks and repeats
// collapse as in CTC, the collapse is y; frame t's emission is read from row u = the number of labels emitted before frame t.  Per node
//   b(t,u) = lp[t][u][blank],   r(t,u) = lp[t][u][y_u] (u >= 1: the last label again),   e(t,u) = lp[t][u][y_{u+1}] (u < U: the next label)
// and per column two states, Ab / An = the mass after t frames with u labels emitted that ends in a blank (or in nothing) / in y_u:
//   Ab[0][0] = 0;   Ab[t+1][u] = lse(Ab, An)[t][u] + b(t,u)
//                   An[t+1][u] = lse(An[t][u] + r(t,u), X[t][u-1] + e(t,u-1)),   X[t][u] = lse(Ab, An)[t][u] where y_{u+1} may follow y_u
//                                                                                directly (u = 0 or y_{u+1} != y_u), Ab[t][u] where not
//   total = lse(Ab, An)[T][U],  cost = -total
//   Bb[T][U] = Bn[T][U] = 0;  Bb[t][u] = lse(b + Bb[t+1][u], e + Bn[t+1][u+1])
//                             Bn[t][u] = lse(b + Bb[t+1][u], r + Bn[t+1][u], e + Bn[t+1][u+1] where y_{u+1} may follow y_u directly)
//   g_b = -exp(lse(Ab, An)[t][u] + b + Bb[t+1][u] - total),  g_r = -exp(An[t][u] + r + Bn[t+1][u] - total),
//   g_e = -exp(X[t][u] + e + Bn[t+1][u+1] - total);   d cost / d lp[t][u][v] = g_b [v = blank] + g_r [v = y_u] + g_e [v = y_{u+1}]
// (y_u = y_{u+1}: the repeat and the new label share a column, their terms add).  A lattice with T < U + #{u: y_u = y_{u+1}} has no path.
//
// The joiner output x is [R][V], row r = ((n T + t) U1 + u) is node (n, t, u) (padded layout only); it is read in place in its own dtype.
// The node record is 20 bytes in two sections under the same r: row [R][4] floats (b, r, e, log s) -- what the recursion reads, ONE 16-byte
// load per node and frame, a column's neighbours 16 bytes apart -- and rmax [R], the row's maximum M, which only the gradient needs.
//   0. crf_rnnt_prep_kernel (k_rnnt.hip) as it is: tn[n] = 0 marks an invalid utterance.
//   1. crf_ctct_row_kernel<E> (raw joiner output): one wave per live node reads its V-row once (rnnt_row_lse) and writes M, log s and the three
//      emissions (x_v - M) - log s; u = 0 has no r, u = U_n no e: -inf.  A row of -inf gives -inf, not NaN.  crf_ctct_gather_kernel (normalised
//      input): the same record with M = log s = 0, a thread per node.
//   2. crf_ctct_lattice_kernel<WG>: one workgroup per (utterance, direction), thread j = column (forward: u = j; backward: u = U_n - j), T_n
//      dependent steps -- the recursion is frame-synchronous, every column advances once per frame.  Both running values are FP64 in registers
//      (acc_lse2 / acc_lse3 of k_score_grad_body.h).  What a column hands to its neighbour is ONE value per frame -- forward
//      X[t][u] + e(t,u), backward Bn[t+1][u+1] -- so that every thread reads its own node's record only: it comes by a DPP shift inside a wave
//      and, across waves (WG), through two LDS rows with ONE barrier per frame; U1 <= 64 is the single-wave instantiation without LDS or
//      barrier.  The records of the next kCtctPF frames are loaded a batch ahead from clamped addresses.  Stored per node, fp64: forward
//      (X[t][u], An[t][u]) -- lse(Ab, An) is X where the labels differ and acc_lse2(X, An), the kernel's own bits, where not -- and backward
//      (Bb[t][u], Bn[t][u]).
//   3. crf_ctct_grad_kernel<E, RAW>: one wave per row of grad, live or not.  A live node forms its three occupancies (times weight[n]); RAW
//      re-reads the row and writes g_v - softmax_v (g_b + g_r + g_e) in the input's dtype, the normalised form the zero row with its entries.
//      Every other row (padding, invalid utterance, no finite path) is written as zeros: every element of grad is stored here.
// No atomics, vector loads and stores only, no scratch.  A node's values depend on its utterance alone: the same bits in any batch.
#include "k_rnnt_common.h"   // the row helpers, rnnt_node; acc_lse2, acc_lse3, acc_shift

namespace crf {

// the labels around row u: y_u (-1 at u = 0) and y_{u+1} (-1 at u = U_n); y_{u+1} may follow y_u directly unless both exist and are equal
struct CtctLabels { int rep, next; bool skip; };
__device__ __forceinline__ CtctLabels ctct_labels(const RnntParams &p, int n, int u, int Un) {
    const int *lab = p.labels + p.lab_off[n];
    CtctLabels l;
    l.rep = u >= 1 && u <= Un ? lab[u - 1] : -1;
    l.next = u >= 0 && u < Un ? lab[u] : -1;
    l.skip = l.rep < 0 || l.next < 0 || l.rep != l.next;
    return l;
}

// ---- stage 1 ----
__global__ __launch_bounds__(256) void crf_ctct_gather_kernel(CtctParams q) {
    const RnntParams &p = q.r;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    RnntNode y;
    if (r >= p.R || !rnnt_node(p, r, y)) return;
    const float *xr = (const float *)p.x + r * p.V;
    const CtctLabels l = ctct_labels(p, y.n, y.u, y.Un);
    *(float4 *)(p.row + 4 * r) = float4{xr[p.blank], l.rep >= 0 ? xr[l.rep] : -INFINITY, l.next >= 0 ? xr[l.next] : -INFINITY, 0.f};
    q.rmax[r] = 0.f;
}

template <typename E>
__global__ __launch_bounds__(64 * kRnntWaves) void crf_ctct_row_kernel(CtctParams q) {
    const RnntParams &p = q.r;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRnntWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    RnntNode y;
    if (r >= p.R || !rnnt_node(p, r, y)) return;  // (no barrier in this kernel: waves leave on their own)
    const char *xr = (const char *)p.x + (size_t)r * p.V * sizeof(E);
    float M, ls;
    const bool fin = rnnt_row_lse<E>(xr, p.V, lane, M, ls);
    if (lane == 0) {
        const CtctLabels l = ctct_labels(p, y.n, y.u, y.Un);
        auto lp = [&](int v) { return fin && v >= 0 ? (lat_ld<E>(xr + (size_t)v * sizeof(E)) - M) - ls : -INFINITY; };
        *(float4 *)(p.row + 4 * r) = float4{lp(p.blank), lp(l.rep), lp(l.next), ls};
        q.rmax[r] = M;
    }
}

// ---- stage 2 ----
template <bool WG>
__global__ __launch_bounds__(WG ? kRnntMaxU1 : 64) void crf_ctct_lattice_kernel(CtctParams q) {
    constexpr int PF = kCtctPF;
    constexpr double kNegInf = -INFINITY;
    __shared__ double edge[2][WG ? kRnntMaxU1 / 64 : 1];   // WG: what the top lane of every wave hands on, this frame's and the one before
    const RnntParams &p = q.r;
    const int j = threadIdx.x, lane = j & 63;
    const int wave = __builtin_amdgcn_readfirstlane(j >> 6);
    const int n = blockIdx.x;
    const bool back = blockIdx.y != 0;
    const int Tn = p.tn[n], Un = p.un[n];
    if (Tn <= 0 || Un >= (int)blockDim.x) {                // (the whole workgroup, in front of any barrier)
        if (!back && j == 0) {
            p.total[n] = -INFINITY;
            p.cost[n] = INFINITY;
            if (p.invalid) p.invalid[n] = 1;
        }
        return;
    }
    const int S = p.U1;
    const int64_t base = p.node_off[n];
    const float4 *rb = (const float4 *)p.row + base;
    double2 *out = (double2 *)(back ? p.beta : p.alpha) + base;
    const int u = back ? Un - j : j;
    const bool act = j <= Un;
    const int uc = act ? u : (back ? 0 : Un);              // (a thread behind U_n reads a live node's record and keeps -inf)
    const bool skip = ctct_labels(p, n, uc, Un).skip;

    // the records of the steps k0 .. k0 + PF - 1 from clamped frames: forward frame k, backward frame T_n - 1 - k
    auto fetch = [&](float4 (&em)[PF], int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int f = 0; f < PF; ++f) {
            const int k = min(k0 + f, Tn - 1);
            em[f] = rb[(back ? Tn - 1 - k : k) * S + uc];
        }
    };
    // what the column below handed on in this frame (the column above, backward: the threads are reversed with the problem)
    auto below = [&](double mine, int k) __attribute__((always_inline)) {
        if constexpr (WG) {
            if (lane == 63) edge[k & 1][wave] = mine;
            __syncthreads();
        }
        double nb = acc_shift<true>(mine);
        if constexpr (WG)
            if (lane == 0 && wave > 0) nb = edge[k & 1][wave - 1];
        return nb;
    };
    // forward: (v0, v1) = (Ab, An)[k][u] -> [k + 1];  backward: (v0, v1) = (Bb, Bn)[t + 1][u] -> [t], t = T_n - 1 - k
    double v0 = j == 0 ? 0.0 : kNegInf, v1 = back ? v0 : kNegInf;
    auto step = [&](const float4 &em, int k) __attribute__((always_inline)) {
        const double b = (double)em.x, r = (double)em.y, e = (double)em.z;
        double n0, n1;
        if (!back) {
            const double s = acc_lse2(v0, v1), x = skip ? s : v0;
            if (act) out[k * S + u] = double2{x, v1};
            const double nb = below(x + e, k);
            n0 = s + b;
            n1 = acc_lse2(v1 + r, nb);
        } else {
            const double x = e + below(v1, k), c = b + v0;
            n0 = acc_lse2(c, x);
            n1 = acc_lse3(c, r + v1, skip ? x : kNegInf);
            if (act) out[(Tn - 1 - k) * S + u] = double2{n0, n1};
        }
        v0 = act ? n0 : kNegInf;
        v1 = act ? n1 : kNegInf;
    };
    float4 ea[PF], eb[PF];
    fetch(ea, 0);
    for (int k0 = 0; k0 < Tn; k0 += 2 * PF) {              // (Tn is the workgroup's: every thread takes the same steps and barriers)
        fetch(eb, k0 + PF);
#pragma unroll
        for (int f = 0; f < PF; ++f)
            if (k0 + f < Tn) step(ea[f], k0 + f);
        fetch(ea, k0 + 2 * PF);
#pragma unroll
        for (int f = 0; f < PF; ++f)
            if (k0 + PF + f < Tn) step(eb[f], k0 + PF + f);
    }
    if (!back && j == Un) {
        const double total = acc_lse2(v0, v1);
        const bool ok = total > -INFINITY;                  // (false for NaN as well)
        p.total[n] = ok ? total : -INFINITY;
        p.cost[n] = ok ? (float)-total : INFINITY;
        if (p.invalid) p.invalid[n] = 0;
    }
}

// ---- stage 3 ----
template <typename E, bool RAW>
__global__ __launch_bounds__(64 * kRnntWaves) void crf_ctct_grad_kernel(CtctParams q) {
    const RnntParams &p = q.r;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRnntWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (r >= p.R) return;
    char *gr = (char *)p.grad + (size_t)r * p.V * sizeof(E);
    const char *xr = (const char *)p.x + (size_t)r * p.V * sizeof(E);
    RnntNode y;
    double total = -INFINITY;
    if (rnnt_node(p, r, y)) total = p.total[y.n];
    if (!(total > -INFINITY)) {
        rnnt_row_map<E, false>(xr, gr, p.V, lane, [](int, float) { return 0.f; });
        return;
    }
    const int S = p.U1;
    const float w = p.weight[y.n];
    const float4 o = *(const float4 *)(p.row + 4 * r);                  // b, r, e, log s
    const double2 a = ((const double2 *)p.alpha)[r];                    // X, An
    const double2 *beta = (const double2 *)p.beta;
    const CtctLabels l = ctct_labels(p, y.n, y.u, y.Un);
    const bool last = y.t + 1 >= y.Tn;
    const double behind = y.u == y.Un ? 0.0 : -INFINITY;               // (Bb, Bn)[T_n][u]
    const double2 nb = last ? double2{behind, behind} : beta[r + S];
    const double s = l.skip ? a.x : acc_lse2(a.x, a.y);                 // lse(Ab, An)[t][u], the lattice kernel's bits
    const float gb = -w * expf((float)(s + (double)o.x + nb.x - total));
    float gp = 0.f, gn = 0.f;
    if (l.rep >= 0) gp = -w * expf((float)(a.y + (double)o.y + nb.y - total));
    if (l.next >= 0) gn = -w * expf((float)(a.x + (double)o.z + (last ? (y.u + 1 == y.Un ? 0.0 : -INFINITY) : beta[r + S + 1].y) - total));
    const int blank = p.blank, rep = l.rep, next = l.next;
    if constexpr (RAW) {
        const float gs = gb + gp + gn, M = q.rmax[r];
        const bool fin = M > -INFINITY;
        rnnt_row_map<E, true>(xr, gr, p.V, lane, [&](int v, float x) {
            const float sm = fin ? score_exp((x - M) - o.w) : 0.f;
            return (v == blank ? gb : 0.f) + (v == rep ? gp : 0.f) + (v == next ? gn : 0.f) - sm * gs;
        });
    } else {
        rnnt_row_map<E, false>(xr, gr, p.V, lane, [&](int v, float) { return (v == blank ? gb : 0.f) + (v == rep ? gp : 0.f) + (v == next ? gn : 0.f); });
    }
}

template __global__ void crf_ctct_row_kernel<float>(CtctParams);
template __global__ void crf_ctct_row_kernel<AlnBf16>(CtctParams);
template __global__ void crf_ctct_row_kernel<AlnF16>(CtctParams);
template __global__ void crf_ctct_lattice_kernel<false>(CtctParams);
template __global__ void crf_ctct_lattice_kernel<true>(CtctParams);
template __global__ void crf_ctct_grad_kernel<float, false>(CtctParams);
template __global__ void crf_ctct_grad_kernel<float, true>(CtctParams);
template __global__ void crf_ctct_grad_kernel<AlnBf16, true>(CtctParams);
template __global__ void crf_ctct_grad_kernel<AlnF16, true>(CtctParams);

}  // namespace crf
