// cat_amd/csrc/k_rnnt_common.h -- what the kernels over a transducer's joiner output [R][V] share (k_rnnt.hip: the RNN-T loss, k_ctct.hip: the
// CTC-Transducer loss): a row of V elements taken 16 bytes at a time, its log-sum-exp, a map over it, and the node a row belongs to.
#pragma once
#include "k_score_grad_body.h"   // acc_lse2, acc_shift

namespace crf {

// ---- a row of V elements of E, 16 bytes at a time ----
template <typename E> __device__ __forceinline__ void rnnt_unpack(const uint4 &q, float (&x)[16 / sizeof(E)]);
template <> __device__ __forceinline__ void rnnt_unpack<float>(const uint4 &q, float (&x)[4]) {
    x[0] = __uint_as_float(q.x); x[1] = __uint_as_float(q.y); x[2] = __uint_as_float(q.z); x[3] = __uint_as_float(q.w);
}
template <> __device__ __forceinline__ void rnnt_unpack<AlnBf16>(const uint4 &q, float (&x)[8]) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = __uint_as_float(w[i] << 16); x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
template <> __device__ __forceinline__ void rnnt_unpack<AlnF16>(const uint4 &q, float (&x)[8]) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] & 0xffffu));
        x[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] >> 16));
    }
}
// fp32 -> E, round to nearest even (a gradient is finite: no NaN handling)
template <typename E> __device__ __forceinline__ unsigned rnnt_bits(float v);
template <> __device__ __forceinline__ unsigned rnnt_bits<float>(float v) { return __float_as_uint(v); }
template <> __device__ __forceinline__ unsigned rnnt_bits<AlnBf16>(float v) {
    const unsigned b = __float_as_uint(v);
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}
template <> __device__ __forceinline__ unsigned rnnt_bits<AlnF16>(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
template <typename E> __device__ __forceinline__ uint4 rnnt_pack(const float (&x)[16 / sizeof(E)]) {
    if constexpr (sizeof(E) == 4) return uint4{rnnt_bits<E>(x[0]), rnnt_bits<E>(x[1]), rnnt_bits<E>(x[2]), rnnt_bits<E>(x[3])};
    else return uint4{rnnt_bits<E>(x[0]) | (rnnt_bits<E>(x[1]) << 16), rnnt_bits<E>(x[2]) | (rnnt_bits<E>(x[3]) << 16),
                      rnnt_bits<E>(x[4]) | (rnnt_bits<E>(x[5]) << 16), rnnt_bits<E>(x[6]) | (rnnt_bits<E>(x[7]) << 16)};
}
template <typename E> __device__ __forceinline__ void rnnt_st(char *a, float v) {
    if constexpr (sizeof(E) == 4) *(float *)a = v;
    else *(unsigned short *)a = (unsigned short)rnnt_bits<E>(v);
}
// A row is taken in chunks of 16 bytes COUNTED FROM ITS START, chunk i by lane i % 64: one 16-byte load (store) where the row starts on a
// 16-byte boundary and the chunk is whole, element loads (stores) otherwise -- odd V, rows that start on a 2-byte boundary, as the other
// kernels on raw output read them.  Which lane takes which element, and in which order, does not depend on the address: a row gives the
// same bits wherever it lies.  Elements past V read as -inf.
template <typename E> __device__ __forceinline__ void rnnt_chunk_ld(const char *xr, bool aligned, int v0, int V, float (&x)[16 / sizeof(E)]) {
    constexpr int ES = sizeof(E), EPV = 16 / ES;
    if (aligned && v0 + EPV <= V) { rnnt_unpack<E>(*(const uint4 *)(xr + (size_t)v0 * ES), x); return; }
#pragma unroll
    for (int k = 0; k < EPV; ++k) x[k] = v0 + k < V ? lat_ld<E>(xr + (size_t)(v0 + k) * ES) : -INFINITY;
}
template <typename E> __device__ __forceinline__ void rnnt_chunk_st(char *gr, bool aligned, int v0, int V, const float (&x)[16 / sizeof(E)]) {
    constexpr int ES = sizeof(E), EPV = 16 / ES;
    if (aligned && v0 + EPV <= V) { *(uint4 *)(gr + (size_t)v0 * ES) = rnnt_pack<E>(x); return; }
#pragma unroll
    for (int k = 0; k < EPV; ++k)
        if (v0 + k < V) rnnt_st<E>(gr + (size_t)(v0 + k) * ES, x[k]);
}

// log sum_v exp(x_v) of one row, the wave's 64 lanes over it, read once: per lane a running (maximum, sum relative to it), per chunk one
// rescale; the lanes' pairs meet in a butterfly (the maximum first, so every lane holds the same bits).  -> the maximum M and
// log sum_v exp(x_v - M), apart (their sum would round at ulp(M)); false for a row of -inf, M = -inf and 0 then.
template <typename E> __device__ __forceinline__ bool rnnt_row_lse(const char *xr, int V, int lane, float &M, float &ls) {
    constexpr int EPV = 16 / sizeof(E);
    const bool aligned = ((unsigned)(uintptr_t)xr & 15u) == 0u;
    const int nchunk = (V + EPV - 1) / EPV;
    float m = -INFINITY, s = 0.f;
    for (int i = lane; i < nchunk; i += 64) {
        float x[EPV];
        rnnt_chunk_ld<E>(xr, aligned, i * EPV, V, x);
        float vm = x[0];
#pragma unroll
        for (int k = 1; k < EPV; ++k) vm = fmaxf(vm, x[k]);
        const float mn = fmaxf(m, vm);
        if (mn > -INFINITY) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < EPV; ++k) a += score_exp(x[k] - mn);
            s = s * score_exp(m - mn) + a;       // (m = -inf: s = 0, exp(-inf) = 0)
            m = mn;
        }
    }
    M = m; ls = 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
    if (!(M > -INFINITY)) return false;
    s *= score_exp(m - M);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    ls = logf(s);
    return true;
}

// out_v = f(v, x_v) over one row, the wave's 64 lanes over it; READ = false: x is not read (f takes 0)
template <typename E, bool READ, typename F>
__device__ __forceinline__ void rnnt_row_map(const char *xr, char *gr, int V, int lane, F &&f) {
    constexpr int EPV = 16 / sizeof(E);
    const bool xal = ((unsigned)(uintptr_t)xr & 15u) == 0u, gal = ((unsigned)(uintptr_t)gr & 15u) == 0u;
    const int nchunk = (V + EPV - 1) / EPV;
    for (int i = lane; i < nchunk; i += 64) {
        const int v0 = i * EPV;
        float x[EPV];
        if constexpr (READ) rnnt_chunk_ld<E>(xr, xal, v0, V, x);
#pragma unroll
        for (int k = 0; k < EPV; ++k) x[k] = f(v0 + k, READ ? x[k] : 0.f);
        rnnt_chunk_st<E>(gr, gal, v0, V, x);
    }
}

// Row r -> its node.  false: r is padding, lies behind the last utterance or belongs to an invalid one.
struct RnntNode { int n, t, u, Tn, Un; };
__device__ __forceinline__ bool rnnt_node(const RnntParams &p, int64_t r, RnntNode &y) {
    if (!p.compact) {
        const int64_t per = (int64_t)p.T * p.U1;
        y.n = (int)(r / per);
        const int rem = (int)(r - (int64_t)y.n * per);
        y.t = rem / p.U1; y.u = rem - y.t * p.U1;
        y.Tn = p.tn[y.n]; y.Un = p.un[y.n];
        return y.Tn > 0 && y.t < y.Tn && y.u <= y.Un;
    }
    if (r >= (int64_t)p.node_off[p.N]) return false;
    int lo = 0, hi = p.N;                        // the last utterance whose first row is at or in front of r (one without rows never is)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)p.node_off[mid] <= r) lo = mid; else hi = mid;
    }
    y.n = lo; y.Tn = p.tn[lo]; y.Un = p.un[lo];
    if (y.Tn <= 0) return false;
    const int local = (int)(r - (int64_t)p.node_off[lo]);
    y.t = local / (y.Un + 1); y.u = local - y.t * (y.Un + 1);
    return y.t < y.Tn;
}

}  // namespace crf
