"""fp64 NumPy yardsticks of the forced alignment (crf_ctc_align): the Viterbi recursion over the 2L+1 CTC states with the library's tie
rule, a brute force over all frame labellings for tiny cases, and the checks a returned path must pass.  No GPU, no library."""
import itertools

import numpy as np

NEG = -np.inf


def expand(labels, blank):
    """The 2L+1 states' classes: blank, l_0, blank, l_1, ..., blank."""
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    return ext


def fits(labels, lx):
    """The CTC validity rule: L + repeats <= lx and lx > 0."""
    labels = np.asarray(labels)
    return lx > 0 and len(labels) + int((labels[1:] == labels[:-1]).sum()) <= lx


def viterbi(x, labels, blank):
    """x [lx, V] log-probs (any float type; the recursion runs in fp64), labels [L] -> (score, pos [lx]); (-inf, None) when no alignment
    of non-zero probability exists.  pos[t] = the transcript index emitted at frame t, -1 for a blank frame.
    Tie rule: among equal candidates the smallest move wins -- stay, then advance by one, then skip; at the end state 2L before 2L-1."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    lx, L = x.shape[0], len(labels)
    if not fits(labels, lx):
        return NEG, None
    ext = expand(labels, blank)
    S = len(ext)
    can_skip = np.zeros(S, dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    v = np.full(S, NEG)
    v[0] = x[0, blank]
    if S > 1:
        v[1] = x[0, ext[1]]
    bp = np.zeros((lx, S), dtype=np.int8)
    for t in range(1, lx):
        c0 = v
        vp = np.concatenate([[NEG, NEG], v])
        c1 = vp[1:-1]
        c2 = np.where(can_skip, vp[:-2], NEG)
        best, mv = c0.copy(), np.zeros(S, dtype=np.int8)
        m = c1 > best
        best[m], mv[m] = c1[m], 1
        m = c2 > best
        best[m], mv[m] = c2[m], 2
        v = x[t, ext] + best
        bp[t] = mv
    s = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        s = S - 2
    score = v[s]
    if not score > NEG:
        return NEG, None
    pos = np.empty(lx, dtype=np.int64)
    for t in range(lx - 1, -1, -1):
        pos[t] = (s >> 1) if (s & 1) else -1
        s -= int(bp[t, s])
    assert s in (0, 1)
    return float(score), pos


def collapse(frame_labels, blank):
    """The CTC rule: merge runs, drop blanks."""
    out, prev = [], None
    for c in frame_labels:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def brute_force(x, labels, blank):
    """The best of all V^T frame labellings that collapse to `labels`: (score, frame classes [T]) in fp64; (-inf, None) if there is none."""
    x = np.asarray(x, dtype=np.float64)
    T, V = x.shape
    want = [int(c) for c in labels]
    best, arg = NEG, None
    for seq in itertools.product(range(V), repeat=T):
        if collapse(seq, blank) != want:
            continue
        sc = float(sum(x[t, c] for t, c in enumerate(seq)))
        if sc > best:
            best, arg = sc, seq
    return best, (None if arg is None else np.array(arg))


def pos_to_classes(pos, labels, blank):
    """Frame classes of a pos row (entries >= -1)."""
    pos = np.asarray(pos)
    labels = np.asarray(labels, dtype=np.int64)
    return np.where(pos < 0, blank, labels[np.maximum(pos, 0)] if len(labels) else blank)


def check_path(pos_row, labels, lx, blank):
    """What every returned row must satisfy: -2 exactly past lx; over [0, lx) the emitted transcript indices are non-decreasing with steps
    of 0 or 1, start at 0, end at L-1, a repeated label is separated by a blank frame, and the frame classes collapse to the transcript."""
    pos_row = np.asarray(pos_row)
    labels = np.asarray(labels, dtype=np.int64)
    L = len(labels)
    assert np.all(pos_row[lx:] == -2), "frames past lx"
    p = pos_row[:lx]
    assert np.all(p >= -1) and np.all(p < max(L, 1)) and (L > 0 or np.all(p == -1)), "range"
    em = p[p >= 0]
    if L:
        assert len(em) and em[0] == 0 and em[-1] == L - 1, "first / last emitted index"
        d = np.diff(em)
        assert np.all((d == 0) | (d == 1)), "steps of the emitted index"
    # state sequence s_t = 2k+1 for an emission, and for a blank frame the blank state between its neighbours
    k_prev = -1          # last emitted index so far
    s_prev = None
    for t in range(lx):
        s = 2 * p[t] + 1 if p[t] >= 0 else 2 * (k_prev + 1)
        if p[t] >= 0:
            k_prev = int(p[t])
        if s_prev is not None:
            mv = s - s_prev
            assert mv in (0, 1, 2), (t, s_prev, s)
            if mv == 2:
                assert (s & 1) and labels[s >> 1] != labels[(s >> 1) - 1], ("skip between equal labels", t)
        else:
            assert s in (0, 1)
        s_prev = s
    assert collapse(pos_to_classes(p, labels, blank), blank) == [int(c) for c in labels], "collapse"


def path_score(x, pos_row, labels, lx, blank):
    """fp64 sum of the path's entries."""
    cls = pos_to_classes(np.asarray(pos_row)[:lx], labels, blank)
    return float(np.asarray(x, dtype=np.float64)[np.arange(lx), cls].sum())
