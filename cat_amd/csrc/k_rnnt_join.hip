// cat_amd/csrc/k_rnnt_join.hip -- the two stages of the RNN-T loss that touch V, for a joiner that is a plain sum (cat/rnnt/joiner.py LogAdd):
// log p(v | t, u) = f[t][v] + g[u][v] - log sum_v exp(f[t][v] + g[u][v]) from f [N][T][V] and g [N][U1][V] alone -- the joint tensor
// [N][T][U1][V] is never formed (include/ctc_crf_hip.h crf_rnnt_simple_loss / crf_rnnt_simple_grad; host side: crf_host_ctc.hip).  The prep
// kernel, the lattice kernel, the 16-byte node record and the alpha / beta / utt sections are those of k_rnnt.hip in the padded layout.
// f + g is formed in fp32 from the inputs' exact values.
//   1. crf_join_row_kernel<E> replaces crf_rnnt_row_kernel: one workgroup of 256 threads per (utterance, kJoinTT frames x kJoinTU rows).  The
//      tile's f rows and g rows are staged in LDS as fp32, kJoinVC columns at a time; thread (ty, tx) keeps the 2 x 2 nodes
//      (t0 + 2 ty + {0, 1}, u0 + 2 tx + {0, 1}) in registers with an online (maximum, sum relative to it) each and walks the chunk four
//      columns a step: four 16-byte LDS reads feed sixteen exps.  A node's row is walked from column 0 in steps of four by ONE thread, so
//      its bits depend on its own f row, g row and V alone.  The maximum is taken off FIRST -- per node, never factored into a maximum of f
//      and one of g, which underflows where f and g peak at different columns.  A row of -inf gives M = -inf, lb = ll = -inf, no NaN.
//   2. crf_join_grad_kernel<E> replaces crf_rnnt_grad_kernel: lane = class column.  One workgroup of kJoinGV threads per (utterance, kJoinGV
//      columns, split s < kJoinSplit); split s takes the frame chunks j = s, s + kJoinSplit, ... of kJoinGL frames, chunk j = frames
//      [j kJoinGL, (j + 1) kJoinGL).  Rows u are taken kJoinGU at a time: the thread holds g[u][v] and the sum over its frames of d g[u][v]
//      in registers.  Per chunk the workgroup forms the nodes' (M, log s, gb, gl) once into LDS -- gb, gl the two occupancies times the
//      utterance's weight, as crf_rnnt_grad_kernel forms them -- and every thread then reads them as broadcasts: per (t, u, v) one exp,
//      -(gb + gl) exp(((f + g) - M) - log s), added to d f[t][v] (a register over u) and to d g[u][v]; a node with gb + gl = 0 (a dead one,
//      or one whose row is all -inf) is given M = +inf, so that its term is an exact 0 without a branch, and groups of 8 rows behind U_n are skipped.
//      gb [v = blank] + gl [v = y_u] follows in a second pass over the tile's nodes, taken only by the waves (one in V / 64) whose columns
//      hold the blank or one of the tile's labels.  d f goes to the fp32 section df [N][T][V] (row tile 0 stores, later tiles add: the
//      same thread, in order), d g to dg [kJoinSplit][N][U1][V] -- both always, whichever gradient is asked for.
//   3. crf_join_fold_kernel<E>: writes EVERY element of the gradients asked for in the inputs' type: d f = df, d g = the splits' partial sums
//      in the order s = 0, 1, ..., over the live rows; zeros for t >= T_n, u > U_n, invalid utterances and lattices without a finite path
//      (whose partial sums were never written and are not read).
// Which frames meet in which partial sum depends on T_n alone (the chunks lie at multiples of kJoinGL, whatever T and N are), every sum runs
// in a fixed order, and there are no atomics: the same bits run to run, and for an utterance alone or anywhere in a batch.  Vector loads and
// stores only, no scratch.
#include "k_lattice_common.h"   // lat_ld, score_exp

namespace crf {

template <typename E> __device__ __forceinline__ void join_st(char *a, float v) {
    if constexpr (sizeof(E) == 4) *(float *)a = v;
    else if constexpr (std::is_same<E, AlnBf16>::value) {
        const unsigned b = __float_as_uint(v);       // round to nearest even (a gradient is finite: no NaN handling)
        *(unsigned short *)a = (unsigned short)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
    } else *(_Float16 *)a = (_Float16)v;
}

// four more columns of one node's online log-sum-exp: x = a + b in fp32, the running maximum m and s = sum exp(x - m).  While every
// column so far is -inf the sum stays an exact 0 (the shift is taken from 0 then: exp(-inf) = 0, never exp(-inf + inf)).
__device__ __forceinline__ void join_acc(float &m, float &s, const float4 &a, const float4 &b) {
    const float x0 = a.x + b.x, x1 = a.y + b.y, x2 = a.z + b.z, x3 = a.w + b.w;
    const float mn = fmaxf(m, fmaxf(fmaxf(x0, x1), fmaxf(x2, x3)));
    const float mr = mn > -INFINITY ? mn : 0.f;
    s = s * score_exp(m - mr) + (((score_exp(x0 - mr) + score_exp(x1 - mr)) + score_exp(x2 - mr)) + score_exp(x3 - mr));
    m = mn;
}

// ---- stage 1 ----
template <typename E>
__global__ __launch_bounds__(kJoinRowThreads) void crf_join_row_kernel(JoinParams q) {
    constexpr int TT = kJoinTT, TU = kJoinTU, VC = kJoinVC, LD = kJoinVC + 4;     // (rows 16-byte aligned, 4 banks apart)
    static_assert(TT == 32 && TU == 32 && kJoinRowThreads == 256, "a 16 x 16 grid of threads, 2 x 2 nodes each");
    __shared__ __attribute__((aligned(16))) float fs[TT][LD];
    __shared__ __attribute__((aligned(16))) float gs[TU][LD];
    const RnntParams &p = q.r;
    const int ntt = (p.T + TT - 1) / TT;
    const int n = blockIdx.x / ntt, t0 = (blockIdx.x - n * ntt) * TT, u0 = blockIdx.y * TU;
    const int Tn = p.tn[n], Un = p.un[n];
    if (Tn <= 0 || t0 >= Tn || u0 > Un) return;                                  // (the whole workgroup, in front of any barrier)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int V = p.V;
    const char *fb = (const char *)q.f + (size_t)n * p.T * V * sizeof(E);
    const char *gb = (const char *)q.g + (size_t)n * p.U1 * V * sizeof(E);
    const bool work = t0 + 2 * ty < Tn && u0 + 2 * tx <= Un;
    float m[2][2], s[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { m[a][b] = -INFINITY; s[a][b] = 0.f; }
    for (int v0 = 0; v0 < V; v0 += VC) {
        __syncthreads();                                                          // (the chunk before has been read)
        for (int i = tid; i < (TT + TU) * VC; i += kJoinRowThreads) {             // rows behind the tensor's last are its last row again
            const int row = i / VC, col = i - row * VC, v = v0 + col;
            float x = -INFINITY;                                                  // columns behind V
            if (v < V)
                x = row < TT ? lat_ld<E>(fb + ((size_t)min(t0 + row, p.T - 1) * V + v) * sizeof(E))
                             : lat_ld<E>(gb + ((size_t)min(u0 + row - TT, p.U1 - 1) * V + v) * sizeof(E));
            if (row < TT) fs[row][col] = x; else gs[row - TT][col] = x;
        }
        __syncthreads();
        if (work) {
            const int steps = (min(V - v0, VC) + 3) >> 2;
            for (int i = 0; i < steps; ++i) {
                const float4 f0 = *(const float4 *)&fs[2 * ty][4 * i], f1 = *(const float4 *)&fs[2 * ty + 1][4 * i];
                const float4 g0 = *(const float4 *)&gs[2 * tx][4 * i], g1 = *(const float4 *)&gs[2 * tx + 1][4 * i];
                join_acc(m[0][0], s[0][0], f0, g0);
                join_acc(m[0][1], s[0][1], f0, g1);
                join_acc(m[1][0], s[1][0], f1, g0);
                join_acc(m[1][1], s[1][1], f1, g1);
            }
        }
    }
    if (!work) return;
    const int *lab = p.labels + p.lab_off[n];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int t = t0 + 2 * ty + a, u = u0 + 2 * tx + b;
            if (t >= Tn || u > Un) continue;
            const char *fr = fb + (size_t)t * V * sizeof(E), *gr = gb + (size_t)u * V * sizeof(E);
            const float M = m[a][b];
            const bool fin = M > -INFINITY;
            const float ls = fin ? logf(s[a][b]) : 0.f;
            float lb = -INFINITY, ll = -INFINITY;
            if (fin) {
                lb = ((lat_ld<E>(fr + (size_t)p.blank * sizeof(E)) + lat_ld<E>(gr + (size_t)p.blank * sizeof(E))) - M) - ls;
                if (u < Un) {
                    const size_t y = (size_t)lab[u] * sizeof(E);
                    ll = ((lat_ld<E>(fr + y) + lat_ld<E>(gr + y)) - M) - ls;
                }
            }
            *(float4 *)(p.row + 4 * (((int64_t)n * p.T + t) * p.U1 + u)) = float4{M, ls, lb, ll};
        }
}

// ---- stage 3 ----
template <typename E>
__global__ __launch_bounds__(kJoinGV) void crf_join_grad_kernel(JoinParams q) {
    constexpr int GU = kJoinGU, GL = kJoinGL, GV = kJoinGV;
    static_assert(GU == 32 && (GL * GU) % GV == 0, "the tile's labels are one 32-bit mask; whole passes of the workgroup over the chunk's nodes");
    __shared__ float4 sc[GL][GU];                                                 // (M, log s, gb, gl) of the chunk's nodes
    const RnntParams &p = q.r;
    const int V = p.V, U1 = p.U1;
    const int nvt = (V + GV - 1) / GV;
    const int n = blockIdx.x / nvt, vt = blockIdx.x - n * nvt, sp = blockIdx.y;
    const int Tn = p.tn[n], Un = p.un[n];
    if (Tn <= 0 || sp * GL >= Tn) return;                                        // (the whole workgroup, in front of any barrier)
    const double total = p.total[n];
    if (!(total > -INFINITY)) return;
    const int tid = threadIdx.x, v = vt * GV + tid;
    const int wv0 = __builtin_amdgcn_readfirstlane(vt * GV + (tid & ~63));       // the wave's first column
    const bool on = v < V;                                                        // (a thread behind V works on column 0 and stores nothing)
    const bool wblank = (unsigned)(p.blank - wv0) < 64u;                          // (wave-uniform)
    const float isblank = v == p.blank ? 1.f : 0.f;
    const float w = p.weight[n];
    const int *lab = p.labels + p.lab_off[n];
    const int64_t base = (int64_t)n * p.T * U1;
    const char *fb = (const char *)q.f + ((size_t)n * p.T * V + (on ? v : 0)) * sizeof(E);
    const char *gb = (const char *)q.g + ((size_t)n * U1 * V + (on ? v : 0)) * sizeof(E);
    float *dfb = q.df_part + (size_t)n * p.T * V + v;
    float *dgb = q.dg_part + ((size_t)sp * p.N + n) * U1 * V + v;
    const size_t rowb = (size_t)V * sizeof(E);
    const unsigned rlast = (unsigned)Un * (unsigned)V;                            // (an utterance's g has < 2^23 elements)

    for (int u0 = 0; u0 <= Un; u0 += GU) {
        const int nu = min(GU, Un + 1 - u0);
        const int myl = u0 + (tid & 31) < Un ? lab[u0 + (tid & 31)] : -1;          // lane k (and k + 32) of every wave: y[u0 + k], -1 where there is none
        const bool onehot = wblank || __ballot((unsigned)(myl - wv0) < 64u) != 0; // the blank or a label of the tile lies in the wave's columns
        unsigned mine = 0u;                                                       // bit k: y[u0 + k] is column v
#pragma unroll
        for (int k = 0; k < GU; ++k) mine |= __builtin_amdgcn_readlane(myl, k) == v ? 1u << k : 0u;
        float g[GU], dg[GU];
        // The row's offset walks in a register the compiler may not fold: folded, the 32 multiples of V become 64 scalar registers that
        // live across the whole kernel.  A row behind U_n reads row U_n again: its nodes have no occupancy.
        unsigned ro = (unsigned)u0 * (unsigned)V;
#pragma unroll
        for (int k = 0; k < GU; ++k) {
            g[k] = lat_ld<E>(gb + (size_t)min(ro, rlast) * sizeof(E));
            ro += (unsigned)V;
            asm volatile("" : "+v"(ro));
            dg[k] = 0.f;
        }
        for (int j = sp; j * GL < Tn; j += kJoinSplit) {
            const int t0 = j * GL, nt = min(GL, Tn - t0);
            __syncthreads();                                                      // (the chunk before has been read)
#pragma unroll 1
            for (int h = 0; h < GL * GU / GV; ++h) {
                const int i = h * GV + tid, tl = i / GU, k = i - tl * GU, t = t0 + tl, u = u0 + k;
                float4 o = float4{INFINITY, 0.f, 0.f, 0.f};
                if (tl < nt && k < nu) {
                    const int64_t r = base + (int64_t)t * U1 + u;
                    const float4 rec = *(const float4 *)(p.row + 4 * r);         // M, log s, lb, ll
                    const double a = p.alpha[r];
                    const double nb = t + 1 < Tn ? p.beta[r + U1] : (u == Un ? 0.0 : -INFINITY);
                    o.z = -w * expf((float)(a + (double)rec.z + nb - total));
                    if (u < Un) o.w = -w * expf((float)(a + (double)rec.w + p.beta[r + 1] - total));
                    if (o.z + o.w != 0.f) { o.x = rec.x; o.y = rec.y; }           // (gb and gl have one sign: else both are 0, and M may be -inf)
                }
                sc[tl][k] = o;                                                    // a node without occupancy: M = +inf, its exp is an exact 0
            }
            __syncthreads();
            float fnext = lat_ld<E>(fb + (size_t)t0 * rowb);
            for (int tl = 0; tl < nt; ++tl) {
                const float fv = fnext;
                fnext = lat_ld<E>(fb + (size_t)min(t0 + tl + 1, Tn - 1) * rowb);
                float acc = 0.f;
#pragma unroll
                for (int k0 = 0; k0 < GU; k0 += 8) {                              // the softmax terms, eight rows' broadcasts in flight at a time
                    if (k0 < nu) {
#pragma unroll
                        for (int k = k0; k < k0 + 8; ++k) {
                            const float4 o = sc[tl][k];
                            const float term = -(o.z + o.w) * score_exp(((fv + g[k]) - o.x) - o.y);
                            acc += term;
                            dg[k] += term;
                        }
                    }
                }
                if (onehot) {                                                     // gb at the blank's column, gl at the label's: one wave in V / 64
                    unsigned bits = mine;                                         // (taken apart here, frame by frame: 32 registers or 64 scalar
                    asm volatile("" : "+v"(bits));                                //  ones would hold the parts across the loop otherwise)
#pragma unroll
                    for (int k = 0; k < GU; ++k) {
                        const float4 o = sc[tl][k];
                        const float e = fmaf((float)((bits >> k) & 1u), o.w, isblank * o.z);
                        acc += e;
                        dg[k] += e;
                    }
                }
                float *d = dfb + (size_t)(t0 + tl) * V;
                if (on) {
                    if (u0) acc += *d;
                    *d = acc;
                }
            }
        }
        if (on) {
            ro = (unsigned)u0 * (unsigned)V;
#pragma unroll
            for (int k = 0; k < GU; ++k) {
                if (k < nu) dgb[ro] = dg[k];
                ro += (unsigned)V;
                asm volatile("" : "+v"(ro));
            }
        }
    }
}

// ---- stage 4 ----
template <typename E>
__global__ __launch_bounds__(256) void crf_join_fold_kernel(JoinParams q) {
    const RnntParams &p = q.r;
    const bool isg = blockIdx.y != 0;
    char *out = (char *)(isg ? q.grad_g : q.grad_f);
    const int per = isg ? p.U1 : p.T;
    const int64_t row = blockIdx.x;
    if (!out || row >= (int64_t)p.N * per) return;
    const int n = (int)(row / per), i = (int)(row - (int64_t)n * per);
    const int Tn = p.tn[n], Un = p.un[n], V = p.V;
    const bool live = Tn > 0 && (isg ? i <= Un : i < Tn) && p.total[n] > -INFINITY;
    const int ns = !live ? 0 : isg ? min(kJoinSplit, (Tn + kJoinGL - 1) / kJoinGL) : 1;
    const float *src = isg ? q.dg_part + ((size_t)n * p.U1 + i) * V : q.df_part + (size_t)row * V;
    const size_t step = isg ? (size_t)p.N * p.U1 * V : 0;
    out += (size_t)row * V * sizeof(E);
    for (int v = threadIdx.x; v < V; v += 256) {
        float a = 0.f;
        for (int s = 0; s < ns; ++s) a = s ? a + src[s * step + v] : src[v];
        join_st<E>(out + (size_t)v * sizeof(E), a);
    }
}

template __global__ void crf_join_row_kernel<float>(JoinParams);
template __global__ void crf_join_row_kernel<AlnBf16>(JoinParams);
template __global__ void crf_join_row_kernel<AlnF16>(JoinParams);
template __global__ void crf_join_grad_kernel<float>(JoinParams);
template __global__ void crf_join_grad_kernel<AlnBf16>(JoinParams);
template __global__ void crf_join_grad_kernel<AlnF16>(JoinParams);
template __global__ void crf_join_fold_kernel<float>(JoinParams);
template __global__ void crf_join_fold_kernel<AlnBf16>(JoinParams);
template __global__ void crf_join_fold_kernel<AlnF16>(JoinParams);

}  // namespace crf
