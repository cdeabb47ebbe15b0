"""The yardstick of ctc_edit_distance (include/ctc_crf_hip.h crf_ctc_edit_distance): the contract's double loop in plain Python -- cost and
the (nsub, ndel, nins) counts with the tie rule -- and an anti-diagonal NumPy form of the same recursion for long sequences and whole
batches.  tests/test_ctc_edit_api.py holds the NumPy form to the loop and the loop to hand-worked values.

    D[0][j] = (j; 0, 0, j)   D[i][0] = (i; 0, i, 0)
    D[i][j] = the cheapest of  diag D[i-1][j-1] + (r_i != y_j),  del D[i-1][j] + 1,  ins D[i][j-1] + 1
              -- among equal costs the first in ORDER -- with that cell's counts, one added to the matching count (none for a match)."""
import numpy as np

ORDER = ("diag", "del", "ins")            # the contract's tie rule: strict compares in this order


def loop(r, y, order=ORDER):
    """(dist, nsub, ndel, nins) of hypothesis y against reference r, sequences of ints.  `order`: another tie order (for the tests of the
    yardstick: which results depend on the rule at all)."""
    r, y = [int(v) for v in r], [int(v) for v in y]
    R, Y = len(r), len(y)
    D = [[None] * (Y + 1) for _ in range(R + 1)]
    for j in range(Y + 1):
        D[0][j] = (j, 0, 0, j)
    for i in range(R + 1):
        D[i][0] = (i, 0, i, 0)
    for i in range(1, R + 1):
        for j in range(1, Y + 1):
            ne = int(r[i - 1] != y[j - 1])
            a, b, c = D[i - 1][j - 1], D[i - 1][j], D[i][j - 1]
            cand = {"diag": (a[0] + ne, a[1] + ne, a[2], a[3]), "del": (b[0] + 1, b[1], b[2] + 1, b[3]), "ins": (c[0] + 1, c[1], c[2], c[3] + 1)}
            best = cand[order[0]]
            for k in order[1:]:
                if cand[k][0] < best[0]:
                    best = cand[k]
            D[i][j] = best
    return D[R][Y]


def antidiag_batch(refs, hyps):
    """The same recursion for P pairs at once, one anti-diagonal i + j = d per step.  refs, hyps: lists of int sequences.
    -> int64 array [P][4] = (dist, nsub, ndel, nins).  The pairs are padded to the longest reference and hypothesis; a cell depends on
    cells of smaller i and j only, so the padding never reaches D[R_p][Y_p]."""
    P = len(refs)
    assert P == len(hyps)
    out = np.zeros((P, 4), dtype=np.int64)
    if P == 0:
        return out
    Rs, Ys = np.array([len(r) for r in refs]), np.array([len(y) for y in hyps])
    Rm, Ym = int(Rs.max()), int(Ys.max())
    r = np.full((P, max(Rm, 1)), -1, dtype=np.int64)           # r_i of pair p at column i - 1
    yr = np.full((P, max(Ym, 1)), -2, dtype=np.int64)          # y_j of pair p at column Ym - j: ascending in i along an anti-diagonal
    for p in range(P):
        r[p, :Rs[p]] = np.asarray(refs[p], dtype=np.int64)
        if Ys[p]:
            yr[p, Ym - Ys[p]:Ym] = np.asarray(hyps[p], dtype=np.int64)[::-1]
    p1 = p2 = None
    for d in range(Rm + Ym + 1):
        cur = np.zeros((4, P, Rm + 1), dtype=np.int64)         # (cost, nsub, ndel, nins) of the cells (i, d - i)
        if d <= Ym:
            cur[0, :, 0] = d; cur[3, :, 0] = d                 # i = 0: (j; 0, 0, j)
        if d <= Rm:
            cur[0, :, d] = d; cur[2, :, d] = d                 # j = 0: (i; 0, i, 0)
        lo, hi = max(1, d - Ym), min(Rm, d - 1)                # the inner cells i = lo .. hi, j = d - i
        if lo <= hi:
            ne = (r[:, lo - 1:hi] != yr[:, Ym - d + lo:Ym - d + hi + 1]).astype(np.int64)
            dg = p2[:, :, lo - 1:hi].copy(); dg[0] += ne; dg[1] += ne
            de = p1[:, :, lo - 1:hi].copy(); de[0] += 1; de[2] += 1
            im = p1[:, :, lo:hi + 1].copy(); im[0] += 1; im[3] += 1
            best = dg
            best = np.where((de[0] < best[0])[None], de, best)
            best = np.where((im[0] < best[0])[None], im, best)
            cur[:, :, lo:hi + 1] = best
        for p in np.nonzero(Rs + Ys == d)[0]:
            out[p] = cur[:, p, Rs[p]]
        p2, p1 = p1, cur
    return out


def antidiag(r, y):
    """(dist, nsub, ndel, nins) of one pair by the anti-diagonal form."""
    return tuple(int(v) for v in antidiag_batch([r], [y])[0])


def wer(dist, ref_lengths):
    """cal_wer's figure (cat/ctc/train.py:200-210): summed errors over summed reference lengths."""
    return float(np.sum(dist)) / float(np.sum(ref_lengths))
