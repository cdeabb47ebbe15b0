// cat_amd/csrc/k_rnnt.hip -- the RNN-T transducer loss and its gradient (include/ctc_crf_hip.h crf_rnnt_loss / crf_rnnt_grad; host side:
// crf_host_ctc.hip): cost[n] = -log p(y_n | x_n), summed over all monotone alignments of the lattice T_n x (U_n + 1) -- blank moves
// t -> t + 1, label y[u] moves u -> u + 1, the path ends with a blank at (T_n - 1, U_n).
//
//   alpha[0][0] = 0,        alpha[t][u] = lse(alpha[t-1][u] + lb[t-1][u], alpha[t][u-1] + ll[t][u-1])
//   beta[T-1][U] = lb[T-1][U],  beta[t][u] = lse(beta[t+1][u] + lb[t][u], beta[t][u+1] + ll[t][u])
//   total = alpha[T-1][U] + lb[T-1][U],   cost = -total
//   d cost / d lb[t][u] = -exp(alpha[t][u] + lb[t][u] + beta[t+1][u] - total)    (beta[T][U] = 0, beta[T][u < U] = -inf)
//   d cost / d ll[t][u] = -exp(alpha[t][u] + ll[t][u] + beta[t][u+1] - total)    (u < U)
//
// The joiner output x is [R][V]: row r is node (n, t, u), padded ((n T + t) U1 + u) or compact (the utterances back to back, each
// T_n x (U_n + 1) row-major); it is read in place in its own dtype and never copied.  Everything per node lives in the workspace under
// the same index r.
//   0. crf_rnnt_prep_kernel, one workgroup: the prefix sums that give every utterance its first row and first label, and its validity
//      (T_n in [1, T], U_n in [0, U1 - 1], the rows and labels it claims inside the tensors, every label in [0, V) and not the blank).
//      tn[n] = 0 marks an invalid utterance; nothing of it is read afterwards.  In the compact layout an utterance whose lengths are out
//      of range claims no rows.
//   1. row stage.  crf_rnnt_row_kernel<E> (raw joiner output): one wave per live node reads its V-row ONCE -- an online log-sum-exp, 16-byte
//      loads where the row starts on a 16-byte boundary, element loads otherwise (odd V, rows that start on a 2-byte boundary), the same
//      elements in the same lanes either way -- and writes the row's maximum M, log s = log sum_v exp(x_v - M), lb = (x[blank] - M) - log s
//      and ll = (x[y_u] - M) - log s in one 16-byte store.  M and log s stay apart and the maximum is taken off FIRST, as log_softmax does:
//      x - (M + log s) rounds at ulp(M), and logits with a common offset of 4 096 put the gradient off by 2e-4 of its largest entry
//      (DESIGN.md 7 (f15)); (x - M) - log s does not know the offset.  A row of -inf gives lb = ll = -inf, not NaN.
//      crf_rnnt_gather_kernel (normalised input): the same four floats, M = log s = 0, a thread per node.
//   2. crf_rnnt_lattice_kernel<WG>: one workgroup per (utterance, direction), thread j = column (alpha: u = j; beta: u = U_n - j, time
//      reversed, which makes it the same recursion), T_n + U_n dependent steps along the anti-diagonals.  The running value stays in a
//      register; the neighbour's previous value comes by a DPP shift inside a wave and, across waves (WG), through two LDS rows with ONE
//      barrier per step; U1 <= 64 is the single-wave instantiation without LDS or barrier.  The two emissions of the next kRnntPF
//      diagonals are loaded a batch ahead from clamped addresses (no branch around a load), so the chain does not wait on memory.
//      The running values are FP64 (acc_lse2 of k_score_grad_body.h: the differences, exp and log in fp32): at T + U = 200 and V = 4 097
//      they reach 1 600, where one fp32 rounding is 6e-5 and there is one per step -- the occupancies' exponent would be off by 1e-3 against
//      the project's 1e-4.  alpha and beta are stored in fp64 for the same reason.
//   3. crf_rnnt_grad_kernel<E, RAW>: one wave per row of grad, live or not.  A live node forms its two occupancies g_blank, g_label
//      (times weight[n]) from alpha, beta, lb, ll and total; RAW re-reads the row and writes g_v - softmax_v (g_blank + g_label) in the
//      input's dtype, the normalised form writes the zero row with its two entries.  Every other row (padding, invalid utterance, no finite
//      path) is written as zeros: every element of grad is stored here, nothing is zeroed in front.
// No atomics, vector loads and stores only, no scratch.  A node's values depend on its utterance alone: the same bits in any batch and
// in either layout.
#include "k_rnnt_common.h"   // the row helpers, rnnt_node; acc_lse2, acc_shift

namespace crf {

// ---- stage 0 ----
__global__ __launch_bounds__(kRnntPrepThreads) void crf_rnnt_prep_kernel(RnntParams p) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave == 0) {
        long long cn = 0, cl = 0;                // rows and labels in front of this chunk of 64 utterances
        for (int n0 = 0; n0 < p.N; n0 += 64) {
            const int n = n0 + lane;
            const bool in = n < p.N;
            const int Tn = in ? p.lx[n] : 0, Un = in ? p.ly[n] : 0;
            const bool lenok = in && Tn >= 1 && Tn <= p.T && Un >= 0 && Un <= p.U1 - 1;
            long long ext = 0, lext = 0;
            if (in) {
                ext = p.compact ? (lenok ? (long long)Tn * (Un + 1) : 0) : (long long)p.T * p.U1;
                lext = p.compact ? (lenok ? Un : 0) : p.U1 - 1;
            }
            long long se = ext, sl = lext;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long a = __shfl_up(se, o), b = __shfl_up(sl, o);
                if (lane >= o) { se += a; sl += b; }
            }
            const long long on = cn + se - ext, ol = cl + sl - lext;
            const bool ok = lenok && on + ext <= p.R && ol + lext <= p.nlab;
            if (in) {
                p.node_off[n] = (int)min(on, (long long)p.R);
                p.lab_off[n] = (int)min(ol, (long long)p.nlab);
                p.tn[n] = ok ? Tn : 0;
                p.un[n] = ok ? Un : 0;
            }
            cn += __shfl(se, 63); cl += __shfl(sl, 63);
        }
        if (lane == 0) p.node_off[p.N] = (int)min(cn, (long long)p.R);
    }
    __syncthreads();
    for (int n = wave; n < p.N; n += kRnntPrepThreads / 64) {        // the labels, a wave per utterance
        const int Tn = p.tn[n], Un = p.un[n];
        if (Tn <= 0) continue;
        const int *yl = p.labels + p.lab_off[n];
        bool bad = false;
        for (int i = lane; i < Un; i += 64) {
            const int l = yl[i];
            bad = bad || (unsigned)l >= (unsigned)p.V || l == p.blank;
        }
        if (__ballot(bad) && lane == 0) p.tn[n] = 0;
    }
}

// ---- stage 1 ----
__global__ __launch_bounds__(256) void crf_rnnt_gather_kernel(RnntParams p) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    RnntNode y;
    if (r >= p.R || !rnnt_node(p, r, y)) return;
    const float *xr = (const float *)p.x + r * p.V;
    *(float4 *)(p.row + 4 * r) = float4{0.f, 0.f, xr[p.blank], y.u < y.Un ? xr[p.labels[p.lab_off[y.n] + y.u]] : -INFINITY};
}

template <typename E>
__global__ __launch_bounds__(64 * kRnntWaves) void crf_rnnt_row_kernel(RnntParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRnntWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    RnntNode y;
    if (r >= p.R || !rnnt_node(p, r, y)) return;  // (no barrier in this kernel: waves leave on their own)
    const char *xr = (const char *)p.x + (size_t)r * p.V * sizeof(E);
    float M, ls;
    const bool fin = rnnt_row_lse<E>(xr, p.V, lane, M, ls);
    if (lane == 0) {
        const float lb = fin ? (lat_ld<E>(xr + (size_t)p.blank * sizeof(E)) - M) - ls : -INFINITY;
        const float ll = fin && y.u < y.Un ? (lat_ld<E>(xr + (size_t)p.labels[p.lab_off[y.n] + y.u] * sizeof(E)) - M) - ls : -INFINITY;
        *(float4 *)(p.row + 4 * r) = float4{M, ls, lb, ll};
    }
}

// ---- stage 2 ----
template <bool WG>
__global__ __launch_bounds__(WG ? kRnntMaxU1 : 64) void crf_rnnt_lattice_kernel(RnntParams p) {
    constexpr int PF = kRnntPF;
    __shared__ double edge[2][WG ? kRnntMaxU1 / 64 : 1];   // WG: the top lane's value of every wave, this step's and the one before
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
    const int S = p.compact ? Un + 1 : p.U1;
    const int64_t base = p.node_off[n];
    const float *rb = p.row + 4 * base;
    double *out = (back ? p.beta : p.alpha) + base;
    const int u = back ? Un - j : j;
    const int uc = min(max(u, 0), Un), ul = min(max(u - 1, 0), Un);

    // the two emissions of the steps d0 .. d0 + PF - 1 from clamped nodes: forward lb[t-1][u] and ll[t][u-1], backward lb[t][u] and ll[t][u]
    auto fetch = [&](float (&eb)[PF], float (&el)[PF], int d0) __attribute__((always_inline)) {
#pragma unroll
        for (int f = 0; f < PF; ++f) {
            const int q = d0 + f - j;
            if (!back) {
                eb[f] = rb[4 * (min(max(q - 1, 0), Tn - 1) * S + uc) + 2];
                el[f] = rb[4 * (min(max(q, 0), Tn - 1) * S + ul) + 3];
            } else {
                const float *o = rb + 4 * (min(max(Tn - 1 - q, 0), Tn - 1) * S + uc);
                eb[f] = o[2];
                el[f] = o[3];
            }
        }
    };
    double v = -INFINITY, fin = -INFINITY;
    auto step = [&](float eb, float el, int d) __attribute__((always_inline)) {
        double nb = acc_shift<true>(v);
        if constexpr (WG)
            if (lane == 0 && wave > 0 && d > 0) nb = edge[(d - 1) & 1][wave - 1];
        const int q = d - j;
        double nv = acc_lse2(v + (double)eb, nb + (double)el);
        if (d == 0 && j == 0) nv = back ? (double)eb : 0.0;
        const bool act = q >= 0 && q < Tn && j <= Un;
        v = act ? nv : -INFINITY;
        if (act) out[(back ? Tn - 1 - q : q) * S + u] = v;
        if (q == Tn - 1) fin = v;
        if constexpr (WG) {
            if (lane == 63) edge[d & 1][wave] = v;
            __syncthreads();
        }
    };
    const int nsteps = Tn + Un;
    float ab[PF], al[PF], bb[PF], bl[PF];
    fetch(ab, al, 0);
    for (int d0 = 0; d0 < nsteps; d0 += 2 * PF) {           // (whole batches: past the last diagonal no column is active)
        fetch(bb, bl, d0 + PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) step(ab[f], al[f], d0 + f);
        fetch(ab, al, d0 + 2 * PF);
#pragma unroll
        for (int f = 0; f < PF; ++f) step(bb[f], bl[f], d0 + PF + f);
    }
    if (!back && j == Un) {
        const double total = fin + (double)rb[4 * ((Tn - 1) * S + Un) + 2];
        const bool ok = total > -INFINITY;                  // (false for NaN as well)
        p.total[n] = ok ? total : -INFINITY;
        p.cost[n] = ok ? (float)-total : INFINITY;
        if (p.invalid) p.invalid[n] = 0;
    }
}

// ---- stage 3 ----
template <typename E, bool RAW>
__global__ __launch_bounds__(64 * kRnntWaves) void crf_rnnt_grad_kernel(RnntParams p) {
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
    const int S = p.compact ? y.Un + 1 : p.U1;
    const float w = p.weight[y.n];
    const float4 o = *(const float4 *)(p.row + 4 * r);                  // M, log s, lb, ll
    const double a = p.alpha[r];
    const double nb = y.t + 1 < y.Tn ? p.beta[r + S] : (y.u == y.Un ? 0.0 : -INFINITY);
    const float gb = -w * expf((float)(a + (double)o.z + nb - total));
    float gl = 0.f;
    int label = -1;
    if (y.u < y.Un) {
        label = p.labels[p.lab_off[y.n] + y.u];
        gl = -w * expf((float)(a + (double)o.w + p.beta[r + 1] - total));
    }
    const int blank = p.blank;
    if constexpr (RAW) {
        const float gs = gb + gl;
        const bool fin = o.x > -INFINITY;
        rnnt_row_map<E, true>(xr, gr, p.V, lane, [&](int v, float x) {
            const float sm = fin ? score_exp((x - o.x) - o.y) : 0.f;
            return (v == blank ? gb : 0.f) + (v == label ? gl : 0.f) - sm * gs;
        });
    } else {
        rnnt_row_map<E, false>(xr, gr, p.V, lane, [&](int v, float) { return v == blank ? gb : v == label ? gl : 0.f; });
    }
}

template __global__ void crf_rnnt_row_kernel<float>(RnntParams);
template __global__ void crf_rnnt_row_kernel<AlnBf16>(RnntParams);
template __global__ void crf_rnnt_row_kernel<AlnF16>(RnntParams);
template __global__ void crf_rnnt_lattice_kernel<false>(RnntParams);
template __global__ void crf_rnnt_lattice_kernel<true>(RnntParams);
template __global__ void crf_rnnt_grad_kernel<float, false>(RnntParams);
template __global__ void crf_rnnt_grad_kernel<float, true>(RnntParams);
template __global__ void crf_rnnt_grad_kernel<AlnBf16, true>(RnntParams);
template __global__ void crf_rnnt_grad_kernel<AlnF16, true>(RnntParams);

}  // namespace crf
