// cat_amd/csrc/k_beam_common.h -- the wave helpers the two beam searches share (k_beam.hip: LM-free; k_beam_lm.hip: with the n-gram LM):
// the wave maximum of an unsigned word and of a double without the LDS crossbar, the order-preserving integer images of floats, the
// uniform-lane broadcasts, the sum of two log masses and the prefix id.  One copy for both translation units (and for crf_unity.hip).
#pragma once
#include "k_lattice_common.h"

namespace crf {

typedef unsigned long long beam_u64;

// the wave's maximum of an unsigned word in every lane, without the LDS crossbar: rotate-and-max inside each row of 16 lanes (DPP
// row_ror 8 / 4 / 2 / 1), the four rows through readlane + scalar max (crf_device.h wave_max's scheme)
__device__ __forceinline__ unsigned beam_wave_umax(unsigned v) {
#define CRF_DPP_UMAX(ctrl) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, false))
    CRF_DPP_UMAX(0x128);
    CRF_DPP_UMAX(0x124);
    CRF_DPP_UMAX(0x122);
    CRF_DPP_UMAX(0x121);
#undef CRF_DPP_UMAX
    const int iv = (int)v;
    return max(max((unsigned)__builtin_amdgcn_readlane(iv, 0), (unsigned)__builtin_amdgcn_readlane(iv, 16)),
               max((unsigned)__builtin_amdgcn_readlane(iv, 32), (unsigned)__builtin_amdgcn_readlane(iv, 48)));
}
// a float as the unsigned word that orders as the floats do (sign bit flipped for x >= 0, all bits for x < 0); NaN: 0, below everything
constexpr unsigned kBeamOrdNegInf = 0x007fffffu;               // beam_ord(-inf): nothing at or below it is a class of E_t
__device__ __forceinline__ unsigned beam_ord(float x) {
    const unsigned u = __float_as_uint(x);
    return x != x ? 0u : x == 0.f ? 0x80000000u : (u >> 31) ? ~u : (u | 0x80000000u);   // (-0 and +0 are one value)
}
__device__ __forceinline__ float beam_unord(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// ---- the beam stage's wave helpers ----
// the wave's maximum of any doubles (-inf included), exact: through the integer image that orders as the doubles do (sign bit flipped for
// v >= 0, all bits for v < 0), high word first, then the low words of the lanes that hold the high maximum
__device__ __forceinline__ double beam_wave_max(double v) {
    beam_u64 u = (beam_u64)__double_as_longlong(v);
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    const unsigned hi = (unsigned)(u >> 32), lo = (unsigned)u;
    const unsigned mh = beam_wave_umax(hi);
    const unsigned ml = beam_wave_umax(hi == mh ? lo : 0u);
    beam_u64 k = ((beam_u64)mh << 32) | ml;
    k = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)k);
}
// lane `src`'s value in every lane; src is uniform
__device__ __forceinline__ int beam_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float beam_bcast(float v, int src) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src)); }
__device__ __forceinline__ beam_u64 beam_bcast(beam_u64 v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((beam_u64)hi << 32) | lo;
}
__device__ __forceinline__ double beam_bcast(double v, int src) { return __longlong_as_double((long long)beam_bcast((beam_u64)__double_as_longlong(v), src)); }
// log(exp(a) + exp(b)) in fp64 with fp32 exp / log of the differences (k_score_grad.hip's acc_lse2); both -inf: -inf
__device__ __forceinline__ double beam_lse2(double a, double b) {
    const double m = fmax(fmax(a, b), -1.7976931348623157e308);
    return m + (double)score_log(score_exp((float)(a - m)) + score_exp((float)(b - m)));
}
// the id of the prefix l + c from the id of l: a multiply-add and a 64-bit finaliser
__device__ __forceinline__ beam_u64 beam_mix(beam_u64 id, int c) {
    beam_u64 x = id * 0x9E3779B97F4A7C15ull + (beam_u64)(unsigned)(c + 1);
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x;
}

}  // namespace crf
