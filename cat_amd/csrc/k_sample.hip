// cat_amd/csrc/k_sample.hip -- label sequences drawn on the GPU: per frame K classes from softmax(x) (or the arg-max), then the CTC map B
// (repeats merged, blanks dropped) on each of the B K frame paths.  Host side: crf_ctc_sample (crf_host_ctc.hip).
//
// Row stage (crf_sample_row_kernel<G, E, GREEDY>): G lanes per row (n, t), G = 16 for V <= kSampleSmallV (16 rows per workgroup of 256
// threads), else a wave per row (one wave per workgroup); rows t >= lx[n] idle.  The row is read ONCE, whatever K is:
//   1. lane `sub` loads the entries v = sub, sub + G, ... (coalesced), keeps their maximum and puts the upcast values into LDS;
//      m = max_v x^_v by a butterfly over the G lanes;
//   2. lane l owns the SEGMENT of seg = ceil(V / G) | 1 consecutive classes [l seg, (l + 1) seg) (an odd stride: no bank conflicts) and
//      replaces them, in order, by the running sum inside the segment:  w_v = exp2((x^_v - m) log2 e) (v_exp_f32; exp(-inf) = 0),
//      S_v = S_{v-1} + w_v, S = 0 in front of the segment; tot_l = its last value;
//   3. the segments' totals meet in a Hillis-Steele scan over the lanes (step 1, 2, 4, ..): incl_l.  The partial sums of a parallel scan are
//      not ordered among themselves, so the segment-level CDF is their running maximum over the segments of positive total,
//      I_l = max(incl_j : j <= l, tot_j > 0) -- exact in any order, monotone, and I_l > I_{l-1} only where tot_l > 0.
// The kernel's fp32 inclusive running sum is  C_v = I_{l-1} + S_v  for v in segment l (I_{-1} = 0), and C_{V-1} = I_{G-1}.  Draw k takes
//   u = (Philox4x32-10(counter (t, n, k >> 2, offset), key seed)[k & 3] >> 8) 2^-24,    thr = u C_{V-1},
// the first segment l with I_l > thr (binary search over the G values in LDS), in it the smallest v with I_{l-1} + S_v > thr (binary search
// in LDS; S is monotone inside a segment and rises only where w_v > 0, and so does the rounded sum); where the rounding of the two levels
// disagrees (no such v in the segment) the segment's last class of positive weight; thr rounded up to C_{V-1}: the last segment of
// positive total.  Hence: a class of weight 0 is never drawn, a class of positive weight always is.  Four draws per Philox call, the calls
// spread over the lanes.  A row of -inf only (m = -inf): the blank.
// GREEDY: (value, lowest index) per lane in one pass, the butterfly compares value, then index: the smallest v with x^_v = m
// (torch.argmax's rule: class 0 for a row of -inf only); no LDS.
// Neither NaN nor +inf leads out of bounds: both searches end inside their ranges, and whatever is not a class of the segment falls back
// to the segment's last class of positive weight, that to the blank.
// The classes go to cls[(n K + k)][t] (the workspace), so that the collapse reads a path along t.
//
// Collapse stage (crf_sample_collapse_kernel): one wave per path h = n K + k, 64 frames per step; the previous class comes by a one-lane
// DPP shift with the carry of the step before in lane 0, the keep flags are balloted, a kept class lands at base + (kept lanes below),
// base advances by the popcount; then the tail [len, T) takes the blank.  paths[h][t] (optional) = the class, -1 for t >= lx[n].  No LDS,
// no atomics; every entry of hyps, hyp_len and paths is written by exactly one plain vector store.
#include "k_lattice_common.h"

namespace crf {

// Philox4x32-10 (Salmon et al., SC'11; Random123's constants)
__device__ __forceinline__ void sample_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

template <int G, typename E, bool GREEDY>
__global__ __launch_bounds__(kSampleRowThreads(G)) void crf_sample_row_kernel(SampleParams p) {
    extern __shared__ float sample_lds[];      // per row of this workgroup: [V] the row / its sums, [G] I, [G] the segments' last positive class
    const int sub = threadIdx.x & (G - 1), r = threadIdx.x / G;
    const int64_t f = (int64_t)blockIdx.x * (kSampleRowThreads(G) / G) + r;
    const bool inside = f < (int64_t)p.B * p.T;
    const int n = inside ? (int)(f / p.T) : 0, t = inside ? (int)(f % p.T) : 0;
    const bool live = inside && t < p.lx[n];   // (the same in all G lanes of a row; idle rows run along on -inf and store nothing)
    const E *row = (const E *)p.x + ((int64_t)n * p.xs_b + (int64_t)t * p.xs_t);
    const int V = p.V;

    if constexpr (GREEDY) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        if (live) {
#pragma unroll 8
            for (int v = sub; v < V; v += G) {
                const float x = lat_ld<E>((const char *)(row + v));
                if (x > bv) { bv = x; bi = v; }                              // (ascending v: the lowest index of the lane's maximum)
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, G);
            const int oi = __shfl_xor(bi, o, G);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        // nothing exceeds -inf: a row of -inf only takes class 0, as torch.argmax does; a row of NaN only the blank
        if (live && sub == 0) p.cls[(int64_t)n * p.T + t] = bi < V ? bi : bv == -INFINITY ? 0 : p.blank;
    } else {
        float *cdf = sample_lds + (size_t)r * (V + 2 * G);
        float *segI = cdf + V;
        int *segP = (int *)(segI + G);
        float m = -INFINITY;
        if (live) {
#pragma unroll 8
            for (int v = sub; v < V; v += G) {
                const float x = lat_ld<E>((const char *)(row + v));
                cdf[v] = x;
                m = fmaxf(m, x);
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, G));
        __syncthreads();                       // (every thread of the workgroup comes to the barriers: nothing leaves early)
        const int seg = ((V + G - 1) / G) | 1;
        const int a = sub * seg, b = min(V, a + seg);
        float s = 0.f;
        int lastpos = -1;                      // the segment's last class of positive weight
        if (live) {
            for (int v = a; v < b; ++v) {
                const float w = __builtin_amdgcn_exp2f((cdf[v] - m) * 1.4426950408889634f);   // (m = -inf: NaN, the row emits the blank)
                s += w;
                cdf[v] = s;
                lastpos = w > 0.f ? v : lastpos;
            }
        }
        float incl = s;
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
            const float y = __shfl_up(incl, o, G);
            incl = sub >= o ? incl + y : incl;
        }
        float I = s > 0.f ? incl : 0.f;
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
            const float y = __shfl_up(I, o, G);
            I = sub >= o ? fmaxf(I, y) : I;
        }
        const float top = __shfl(I, G - 1, G);
        segI[sub] = I;
        segP[sub] = lastpos;
        __syncthreads();
        if (!live) return;
        const bool none = !(m > -INFINITY);    // a row of -inf only (or with a NaN maximum): the blank
        const int nq = (p.K + 3) >> 2;
        int *out = p.cls + ((int64_t)n * p.K) * p.T + t;
        for (int q = sub; q < nq; q += G) {
            unsigned rnd[4];
            sample_philox((unsigned)t, (unsigned)n, (unsigned)q, p.offset, p.seed_lo, p.seed_hi, rnd);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * q + j;
                if (k >= p.K) break;
                const float thr = (float)(rnd[j] >> 8) * 5.9604644775390625e-8f * top;
                int lo = 0, hi = G;            // the first segment l in [0, G] with I_l > thr
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (segI[mid] > thr) hi = mid; else lo = mid + 1;
                }
                if (lo == G) {                 // thr was rounded up to the total: the first segment that reaches it -- the last of positive total
                    lo = 0; hi = G - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (segI[mid] >= top) hi = mid; else lo = mid + 1;
                    }
                }
                const int l = lo;              // in [0, G)
                const float base = l > 0 ? segI[l - 1] : 0.f;
                const int v1 = min(V, (l + 1) * seg);
                lo = min(V, l * seg); hi = v1; // the smallest v of the segment with base + S_v > thr
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (base + cdf[mid] > thr) hi = mid; else lo = mid + 1;
                }
                const int lp = segP[l];
                out[(int64_t)k * p.T] = none ? p.blank : lo < v1 ? lo : lp >= 0 ? lp : p.blank;
            }
        }
    }
}

// lane l takes lane l - 1's value, lane 0 keeps `carry` (wave_shr:1; a lane without a source keeps `old`)
__device__ __forceinline__ int sample_shift_up(int v, int carry) {
    return __builtin_amdgcn_update_dpp(carry, v, 0x138, 0xf, 0xf, false);
}

__global__ __launch_bounds__(kSampleWaves * 64) void crf_sample_collapse_kernel(SampleParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t h = (int64_t)blockIdx.x * kSampleWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (h >= (int64_t)p.B * p.K) return;       // (no barrier in this kernel: waves leave on their own)
    const int n = (int)(h / p.K);
    const int T = p.T, lx = max(0, min(p.lx[n], T));
    const int *cls = p.cls + h * T;
    int *hyp = p.hyps + h * T;
    int *path = p.paths ? p.paths + h * T : nullptr;
    int base = 0, carry = -1;                  // kept so far; the class of the frame before this step (none: -1 is no class)
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const int c = t < lx ? cls[t] : -1;
        const int prev = sample_shift_up(c, carry);
        carry = __shfl(c, 63);
        const bool keep = t < lx && c != p.blank && c != prev;
        const unsigned long long mask = __ballot(keep);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (keep) hyp[base + rank] = c;
        if (path && t < T) path[t] = c;
        base += __popcll(mask);
    }
    for (int j = base + lane; j < T; j += 64) hyp[j] = p.blank;
    if (lane == 0) p.hyp_len[h] = base;
}

#define CRF_SAMPLE_INST(E)                                                              \
    template __global__ void crf_sample_row_kernel<16, E, false>(SampleParams);         \
    template __global__ void crf_sample_row_kernel<64, E, false>(SampleParams);         \
    template __global__ void crf_sample_row_kernel<16, E, true>(SampleParams);          \
    template __global__ void crf_sample_row_kernel<64, E, true>(SampleParams);
CRF_SAMPLE_INST(float)
CRF_SAMPLE_INST(AlnBf16)
CRF_SAMPLE_INST(AlnF16)
#undef CRF_SAMPLE_INST

}  // namespace crf
