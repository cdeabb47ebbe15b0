// cat_amd/csrc/k_lattice_common.h -- device helpers the kernels on the CTC lattice of 2L+1 states share (k_align.hip: best path; k_score.hip:
// sum-product scores; k_score_grad.hip: their gradient; k_sample.hip takes the element load only, k_beam.hip the element load and the
// fp32 exp / log of the sums): the upcast element load, the label
// set-up and validity rule of a transcript, the clamped emission prefetch, the fp64 sum of the frames' normalisers, and the fp32
// log-sum-exp of the scores with its one operand order.
// The max-plus / sum-product frame bodies, the back-pointers and the DPP wave recursions stay with their kernels.
//
// Validity (lat_valid) is part of the contract of both surfaces: a transcript of L labels is scored on lx frames iff it fits the
// instantiation, lx > 0, every label lies in [0, V), and L + repeats <= lx (gpu_ctc.h:161-174: L + repeats <= T_b).
// Order of the fp64 sum of lse[t], t < lx (part of the bit-for-bit contract; no atomics; frames at or past lx are never read): a thread's
// (workgroup form) or lane's (wave form) frames t = id, id + stride, ... in order, the wave's butterfly (xor 32, 16, ..., 1), and in the
// workgroup form the eight wave sums in order.
#pragma once
#include "crf_device.h"
#include "crf_kernels_decl.h"

namespace crf {

// one element, upcast: a row of 16-bit elements starts on a 2-byte boundary only (odd V), so these are 2-byte loads
template <typename E> __device__ __forceinline__ float lat_ld(const char *a);
template <> __device__ __forceinline__ float lat_ld<float>(const char *a) { return *(const float *)a; }
template <> __device__ __forceinline__ float lat_ld<AlnBf16>(const char *a) { return __uint_as_float((unsigned)*(const unsigned short *)a << 16); }
template <> __device__ __forceinline__ float lat_ld<AlnF16>(const char *a) { return (float)*(const _Float16 *)a; }

// cnt = repeats | out-of-range labels << 12, summed over the transcript (each count <= 2047 in a workgroup, <= 255 in a wave)
__device__ __forceinline__ bool lat_valid(bool fits, int lx, int L, int cnt) {
    return fits && lx > 0 && (cnt >> 12) == 0 && L + (cnt & 0xfff) <= lx;
}

// Workgroup geometry (kCtcThreads x NR, state s = tid + i * kCtcThreads), first half of the set-up: the label sequence with blanks into
// lab[], repeats and labels outside [0, V) counted in one reduction through red[kCtcWaves], the two -inf entries in front of state 0 of
// both vectors.  Holds one __syncthreads(); returns the count of the whole transcript in every thread.  (tid, lane and wave are the
// kernel's own values: recomputed here they would cost the alignment kernel scalar registers it keeps for its back-trace.)
template <int S>
__device__ __forceinline__ int lat_wg_labels(const int *ul, int L, bool fits, int blank, int V, int (&lab)[S], int *red, float (&A)[2][S + 2],
                                             int tid, int lane, int wave) {
    const int Sx = fits ? 2 * L + 1 : 1;
    int cnt = 0;
    for (int s = tid; s < S; s += kCtcThreads) lab[s] = (s < Sx && (s & 1)) ? ul[s >> 1] : blank;
    for (int i = tid; i < (fits ? L : 0); i += kCtcThreads) {
        const int l = ul[i];
        if ((unsigned)l >= (unsigned)V) cnt += 1 << 12;
        else if (i > 0 && l == ul[i - 1]) cnt += 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) red[wave] = cnt;
    if (tid < 2) { A[0][tid] = -INFINITY; A[1][tid] = -INFINITY; }
    __syncthreads();
    cnt = 0;
#pragma unroll
    for (int i = 0; i < kCtcWaves; ++i) cnt += red[i];
    return cnt;
}
// ... second half, for a valid transcript, state s of a thread (the kernel's own unrolled loop over its NR states calls this, so that what
// else it sets up per state -- the alignment's back-pointer word -- stays in that loop): the state's column as a byte offset into a row
// of E, whether it may skip, and its entry of the virtual vector v_{-1} = (0, -inf, -inf, ...) in A[0].  A label outside [0, V) has
// ended the transcript before; the states past Sx hold the blank.  The caller's barrier follows.
template <typename E, int S>
__device__ __forceinline__ void lat_wg_state(const int (&lab)[S], int Sx, int s, unsigned &labo, bool &skip, float (&A)[2][S + 2]) {
    const int l = lab[s];
    labo = (unsigned)l * (unsigned)sizeof(E);
    skip = s < Sx && (s & 1) && s >= 2 && l != lab[s - 2];
    A[0][2 + s] = s == 0 ? 0.f : -INFINITY;
}

// Emissions of the frames t .. t + PF - 1: unconditional loads (the frame is clamped to lx - 1, the column is always a valid one), so that
// nothing but the loop itself branches around them and the compiler can count what is in flight instead of waiting for everything.
template <int PF, int NR, typename E>
__device__ __forceinline__ void lat_fetch(float (&e)[PF][NR], const E *xb, int64_t xs_t, int lx, const unsigned (&labo)[NR], int t) {
#pragma unroll
    for (int f = 0; f < PF; ++f) {
        const char *row = (const char *)(xb + (int64_t)min(t + f, lx - 1) * xs_t);
#pragma unroll
        for (int i = 0; i < NR; ++i) e[f][i] = lat_ld<E>(row + labo[i]);
    }
}
// (The batch loop around it -- fetch(ea, 0); for (t0 ...) { fetch(eb, t0 + PF); PF frames on ea; fetch(ea, t0 + 2 PF); PF frames on eb } --
// is written out in each of the three frame kernels: as a function that takes the fetch and the frame it gave the same arithmetic but
// another schedule and register allocation in most instantiations, with longer frame loops; profiles/refactor_lattice_isa.txt.)

// ---- the sum-product arithmetic of the hypothesis scores and of their gradient (k_score.hip, k_score_grad.hip: one operand order) ----
// exp and log on the hardware's base-2 instructions without the library's denormal handling: the sums below lie in [1, 3] (or are 0:
// log -> -inf), and a term below 2^-126 of the largest adds nothing either way.  exp(-inf) = 0.
__device__ __forceinline__ float score_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.4426950408889634f); }
__device__ __forceinline__ float score_log(float s) { return __builtin_amdgcn_logf(s) * 0.6931471805599453f; }
// log(exp(a0) + exp(a1) + exp(a2)): the sum is (e0 + e1) + e2.  A term of -inf adds an exact 0, so the two-term form below gives the
// bits of the three-term form with a2 = -inf.  An all -inf triple: the maximum is raised to -FLT_MAX, every difference stays -inf.
__device__ __forceinline__ float score_lse3(float a0, float a1, float a2) {
    const float m = fmaxf(fmaxf(fmaxf(a0, a1), a2), -3.402823466e+38f);
    return m + score_log((score_exp(a0 - m) + score_exp(a1 - m)) + score_exp(a2 - m));
}
__device__ __forceinline__ float score_lse2(float a0, float a1) {
    const float m = fmaxf(fmaxf(a0, a1), -3.402823466e+38f);
    return m + score_log(score_exp(a0 - m) + score_exp(a1 - m));
}

// lane l takes lane l - 1's value, lane 0 takes -inf (wave_shr:1; a lane without a source keeps `old`)
__device__ __forceinline__ float score_shift_up(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000u, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

// sum_{t < lx} lse[t] in fp64, in the order stated at the top.  Wave form (STRIDE 64, id = lane): the sum in every lane.
template <int STRIDE = 64>
__device__ __forceinline__ double lat_lse_sum_wave(const float *lr, int lx, int id) {
    double part = 0.0;
    for (int t = id; t < lx; t += STRIDE) part += (double)lr[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    return part;
}
// Workgroup form: the waves' sums through lred[kCtcWaves], one __syncthreads(); the sum in thread 0 only.
__device__ __forceinline__ double lat_lse_sum_wg(const float *lr, int lx, double *lred, int tid, int lane, int wave) {
    const double part = lat_lse_sum_wave<kCtcThreads>(lr, lx, tid);
    if (lane == 0) lred[wave] = part;
    __syncthreads();
    double sum = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < kCtcWaves; ++i) sum += lred[i];
    }
    return sum;
}

}  // namespace crf
