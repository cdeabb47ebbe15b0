// cat_amd/csrc/k_edit.hip -- token edit distance (Levenshtein) of H hypotheses to the transcripts of their utterances, with the
// substitutions, deletions and insertions of one optimal alignment.  Host side: crf_ctc_edit_distance (crf_host_ctc.hip).
//
//   D[0][j] = j, D[i][0] = i;   D[i][j] = the smallest of  diag D[i-1][j-1] + (r_i != y_j),  del D[i-1][j] + 1,  ins D[i][j-1] + 1,
//   among equal costs the first in that order (strict compares in a fixed order); the cell inherits its predecessor's counts.
//
// Integers only: the result depends on the two token sequences alone and is the same bits wherever a hypothesis stands.
//
// A cell is two words: c = the cost and sd = nsub | ndel << 16 (both <= kMaxCtcLabelLen + 1); nins = c - nsub - ndel is never carried.
// diag adds (r_i != y_j) to both words, del adds 1 and 1 << 16, ins adds 1 to c and leaves sd: a candidate is two adds, a choice one compare
// and two selects.
//
// Geometry: one wave per hypothesis, reference row i = lane NR + k + 1 in register k (NR in 1, 2, 4, 8 from the call's longest
// reference), the table walked skewed -- at step j lane l is on hypothesis column j - l + 1 -- so that the cell above a lane's first row
// is the last row of the lane below it one step earlier, and the diagonal one what arrived the step before: one DPP wave_shr:1 per word
// and step, as the recursions of k_score.hip pass their states.  The hypothesis token travels down the lanes by the same shift; the
// wave loads 64 tokens at a time, one block ahead, and lane 0 takes its token out of that register (v_readlane, the step is
// wave-uniform).  Lane 0's upper neighbour is the border (j, (0, 0, j)).  No LDS, no barrier; the loop runs Y + (last lane in use) steps.
// Strips (STRIP, references of more than kEditStripRows rows; NR = 8, one wave per workgroup): the rows are walked kEditStripRows at a
// time.  Lane 63 stores the cells of a strip's last row, one per column, into LDS; the next strip reads them, 64 columns per load, where
// the first strip has the border.  One wave writes column j - 63 while it reads from column j on: in place, in order, no barrier.
#include "crf_device.h"
#include "crf_kernels_decl.h"

namespace crf {

// lane l takes lane l - 1's value, lane 0 takes `first` (wave_shr:1; a lane without a source keeps `old`)
__device__ __forceinline__ int edit_shift_up(int v, int first) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);
}

template <int NR, bool STRIP>
__global__ __launch_bounds__(STRIP ? 64 : kEditWaves * 64) void crf_ctc_edit_kernel(EditParams p) {
    static_assert(!STRIP || NR * 64 == kEditStripRows, "a strip is one wave's rows");
    constexpr int S = NR * 64;                // reference rows one pass holds
    extern __shared__ int2 edit_row[];        // STRIP: [stride] the cell (c, sd) of the strip's last row at column j + 1
    const int lane = threadIdx.x & 63;
    const int64_t hw = STRIP ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kEditWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (hw >= p.H) return;                    // (no barrier in this kernel: waves leave on their own)
    const int h = (int)hw;
    const int u = __builtin_amdgcn_readfirstlane(p.hyp_utt[h]), Y = __builtin_amdgcn_readfirstlane(p.hyp_len[h]);
    bool ok = (unsigned)u < (unsigned)p.B && Y >= 0 && Y <= p.stride;
    int R = 0;
    if (ok) {
        R = __builtin_amdgcn_readfirstlane(p.ref_len[u]);
        ok = R >= 0 && R <= p.max_ref && R <= (STRIP ? kMaxCtcLabelLen : S);
    }
    if (!ok) {                                // nothing of it is read
        if (lane == 0) {
            p.dist[h] = -1;
            if (p.ops) { p.ops[3 * (int64_t)h] = -1; p.ops[3 * (int64_t)h + 1] = -1; p.ops[3 * (int64_t)h + 2] = -1; }
        }
        return;
    }
    const int *y = p.hyps + (int64_t)h * p.stride;
    const int *r = p.refs + __builtin_amdgcn_readfirstlane(p.ref_off[u]);
    const int nstrip = STRIP ? max(1, (R + S - 1) / S) : 1;

    int c[NR], sd[NR];
    for (int s = 0; s < nstrip; ++s) {
        const int row0 = s * S + lane * NR;   // the lane holds rows row0 + 1 .. row0 + NR; row i compares r[i - 1]
        int rt[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            rt[k] = row0 + k < R ? r[row0 + k] : 0;
            c[k] = row0 + k + 1;              // column 0: (0, i, 0)
            sd[k] = (row0 + k + 1) << 16;
        }
        int dgc = row0, dgs = row0 << 16;     // the cell above the lane's first row, one column back
        int tk = 0;
        const int rows = min(R - s * S, S);
        const int last_lane = rows > 0 ? (rows - 1) / NR : 0;
        const int steps = rows > 0 && Y > 0 ? Y + last_lane : 0;
        const bool keep = STRIP && s + 1 < nstrip;   // a strip follows: its upper neighbours are this one's last row
        int toknxt = lane < Y ? y[lane] : 0;
        for (int base = 0; base < steps; base += 64) {
            const int tokcur = toknxt;
            toknxt = base + 64 + lane < Y ? y[base + 64 + lane] : 0;
            int topc = base + lane + 1, tops = 0;   // the border row: (j, (0, 0, j))
            if constexpr (STRIP) {
                if (s > 0 && base + lane < Y) { const int2 t = edit_row[base + lane]; topc = t.x; tops = t.y; }
            }
            const int n = min(64, steps - base);
            for (int jj = 0; jj < n; ++jj) {
                const int j = base + jj;
                tk = edit_shift_up(tk, __builtin_amdgcn_readlane(tokcur, jj));
                int upc, ups;
                if constexpr (STRIP) {
                    upc = edit_shift_up(c[NR - 1], __builtin_amdgcn_readlane(topc, jj));
                    ups = edit_shift_up(sd[NR - 1], __builtin_amdgcn_readlane(tops, jj));
                } else {
                    upc = edit_shift_up(c[NR - 1], j + 1);
                    ups = edit_shift_up(sd[NR - 1], 0);
                }
                const bool act = (unsigned)(j - lane) < (unsigned)Y;   // column j - lane + 1 in 1 .. Y
                int dc = dgc, ds = dgs, ac = upc, as = ups;            // diagonal and upper neighbour of row k
#pragma unroll
                for (int k = 0; k < NR; ++k) {
                    const int ne = rt[k] != tk ? 1 : 0;
                    int bc = dc + ne, bs = ds + ne;                    // diag
                    const int delc = ac + 1, insc = c[k] + 1;
                    if (delc < bc) { bc = delc; bs = as + 0x10000; }   // del
                    if (insc < bc) { bc = insc; bs = sd[k]; }          // ins
                    dc = c[k]; ds = sd[k];
                    ac = bc; as = bs;
                    c[k] = act ? bc : c[k];
                    sd[k] = act ? bs : sd[k];
                }
                dgc = upc; dgs = ups;
                if constexpr (STRIP) {
                    if (keep && lane == 63 && act) edit_row[j - 63] = make_int2(c[NR - 1], sd[NR - 1]);
                }
            }
        }
    }

    // row R at column Y: one register of one lane of the last strip (R = 0: the border)
    int rc = Y, rs = 0;
    if (R > 0) {
        const int rr = R - 1 - (nstrip - 1) * S;
        int mc = 0, ms = 0;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            mc = k == rr % NR ? c[k] : mc;
            ms = k == rr % NR ? sd[k] : ms;
        }
        rc = __builtin_amdgcn_readlane(mc, rr / NR);
        rs = __builtin_amdgcn_readlane(ms, rr / NR);
    }
    if (lane == 0) {
        p.dist[h] = rc;
        if (p.ops) {
            const int nsub = rs & 0xffff, ndel = (int)((unsigned)rs >> 16);
            p.ops[3 * (int64_t)h] = nsub; p.ops[3 * (int64_t)h + 1] = ndel; p.ops[3 * (int64_t)h + 2] = rc - nsub - ndel;
        }
    }
}

template __global__ void crf_ctc_edit_kernel<1, false>(EditParams);
template __global__ void crf_ctc_edit_kernel<2, false>(EditParams);
template __global__ void crf_ctc_edit_kernel<4, false>(EditParams);
template __global__ void crf_ctc_edit_kernel<8, false>(EditParams);
template __global__ void crf_ctc_edit_kernel<8, true>(EditParams);

}  // namespace crf
