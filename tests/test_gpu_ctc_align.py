"""GPU tests of the forced alignment (ctc_crf.ctc_align / crf_ctc_align, cat_amd/csrc/k_align.hip) against the fp64 NumPy Viterbi of
tests/align_ref.py (itself held to a brute force in tests/test_ctc_align_api.py).

Every call here writes into `pos` / `scores` tensors prefilled with a sentinel, on a workspace filled with 0xFF bytes, and runs
batch-major AND time-major; the two must agree bit for bit.  Shapes are the smallest that reach each code path: the four register
geometries (2L+1 <= 512, 1024, 2048, 4096 states), back-pointer words of 16 frames, back-trace tiles of 64 frames x 128 states."""
import numpy as np
import pytest
import torch

from tests import align_ref

pytestmark = pytest.mark.gpu
SENT_POS, SENT_SCORE = -77, 12345.0


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def bound(T, s_ref):
    """T fp32 additions of partial sums no larger than |S|, doubled because a near-tie may pick a neighbouring path."""
    return 4.0 * T * 2.0 ** -24 * max(1.0, abs(s_ref))


def tokens_of(pos, labels, ly, blank):
    """The tokens tensor that belongs to `pos`."""
    off = np.concatenate([[0], np.cumsum(ly)])
    out = np.full(pos.shape, -1, dtype=np.int64)
    for b in range(pos.shape[0]):
        lab = np.asarray(labels[off[b]:off[b + 1]], dtype=np.int64)
        out[b] = np.where(pos[b] == -2, -1, align_ref.pos_to_classes(np.maximum(pos[b], -1), lab, blank))
    return out


def run(crf, x, labels, lx, ly, blank, layouts=(False, True)):
    """x: [B,T,V] float32 CUDA tensor, batch-major.  -> (pos [B,T], tokens [B,T], scores [B], invalid [B]) as numpy, after checking that the
    layouts agree bit for bit, that no sentinel is left and that tokens belong to pos."""
    B, T, V = x.shape
    lab_t, lx_t, ly_t = (torch.tensor(np.asarray(a), dtype=torch.int32) for a in (labels, lx, ly))
    out = {}
    for tm in layouts:
        xx = x.transpose(0, 1).contiguous() if tm else x
        pos0 = torch.full((B, T), SENT_POS, dtype=torch.int32, device=x.device)
        sc0 = torch.full((B,), SENT_SCORE, dtype=torch.float32, device=x.device)
        pos, tok, sc, inv = crf._C.ctc_align(xx, lab_t, lx_t, ly_t, blank, tm, pos_out=pos0, scores_out=sc0)
        assert pos.data_ptr() == pos0.data_ptr() and sc.data_ptr() == sc0.data_ptr()
        assert pos.dtype == torch.int32 and tok.dtype == torch.int32 and tok.shape == (B, T) and tok.device == x.device
        out[tm] = tuple(a.cpu().numpy() for a in (pos, tok, sc, inv))
        del xx
    first = out[layouts[0]]
    for tm in layouts[1:]:
        for a, c in zip(first, out[tm]):
            assert np.array_equal(a.view(np.int32), c.view(np.int32)), ("layouts differ", tm)
    pos, tok, sc, inv = first
    assert not np.any(pos == SENT_POS) and not np.any(sc == SENT_SCORE)
    assert np.all((inv == 0) | (inv == 1))
    assert np.array_equal(tok, tokens_of(pos, labels, ly, blank)), "tokens do not belong to pos"
    return pos, tok, sc, inv


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. planted alignments: exact
# ---------------------------------------------------------------------------------------------------------------------------------
def random_alignment(rng, labels, lx, blank):
    """A uniformly drawn split of the lx frames over the 2L+1 states (labels at least one frame, a blank between equal labels at least
    one): (frame classes [lx], pos [lx])."""
    L = len(labels)
    ext = align_ref.expand(labels, blank)
    dmin = np.zeros(2 * L + 1, dtype=np.int64)
    dmin[1::2] = 1
    if L > 1:
        dmin[2:-1:2] = np.asarray(labels[1:]) == np.asarray(labels[:-1])
    extra = lx - int(dmin.sum())
    assert extra >= 0
    d = dmin + np.bincount(rng.integers(0, 2 * L + 1, size=extra), minlength=2 * L + 1)
    states = np.repeat(np.arange(2 * L + 1), d)
    return ext[states], np.where(states & 1, states >> 1, -1)


def planted_batch(rng, L, tmode, V, blank):
    """Five utterances with the longest transcript L: no repeats / one repeated label / random (repeats happen: small V) / L // 2 /
    max(L - 1, 0), each over lx = L + repeats (the only alignment), that + 1, or about 1.5 L + 20 frames: ragged lx."""
    pool = np.array([v for v in range(V) if v != blank])

    def norep(n):
        a = rng.integers(0, len(pool), size=n)
        for i in range(1, n):
            if a[i] == a[i - 1]:
                a[i] = (a[i] + 1 + rng.integers(0, len(pool) - 1)) % len(pool)
        return pool[a]
    labs = [norep(L), np.full(L, pool[rng.integers(0, len(pool))]), pool[rng.integers(0, len(pool), size=L)],
            pool[rng.integers(0, len(pool), size=L // 2)], norep(max(L - 1, 0))]
    need = [max(1, len(a) + int((a[1:] == a[:-1]).sum())) for a in labs]
    lx = [n if tmode == 0 else n + 1 if tmode == 1 else max(n, int(1.5 * len(a)) + 20) for n, a in zip(need, labs)]
    T = max(lx) + (2 if tmode == 2 else 0)                       # (frames past every lx as well)
    x = np.full((5, T, V), np.log(0.1 / (V - 1)), dtype=np.float32)
    want = np.full((5, T), -2, dtype=np.int64)
    for b, a in enumerate(labs):
        cls, pos = random_alignment(rng, a, lx[b], blank)
        x[b, np.arange(lx[b]), cls] = np.float32(np.log(0.9))
        want[b, :lx[b]] = pos
    return x, np.concatenate(labs), np.array(lx), np.array([len(a) for a in labs]), want


@pytest.mark.parametrize("L", [0, 1, 7, 8, 15, 16, 31, 32, 255, 256, 511, 512, 1023, 1024, 2047])
def test_planted_alignments_exact(crf, L):
    """The planted class has log 0.9 in every frame, the rest share 0.1: the planted path is the only maximum, and pos must be it exactly.
    L crosses every register geometry and the 16- / 32- / 64-state boundaries of the back-trace's words; T = L + repeats leaves one
    alignment, + 1 two positions for one spare frame, 1.5 L + 20 the general case; blank at 0, V - 1 and inside."""
    rng = np.random.default_rng(4000 + L)
    V = 8 if L >= 255 else (5, 8, 23)[L % 3]
    for tmode in (0, 1, 2):
        for blank in (0, V - 1, V // 2):
            x, labels, lx, ly, want = planted_batch(rng, L, tmode, V, blank)
            pos, tok, sc, inv = run(crf, torch.tensor(x, device="cuda:0"), labels, lx, ly, blank)
            assert np.all(inv == 0), (L, tmode, blank, inv)
            for b in range(5):
                bad = np.nonzero(pos[b] != want[b])[0]
                assert bad.size == 0, (L, tmode, blank, b, int(lx[b]), int(ly[b]), bad[:5], pos[b][bad[:5]], want[b][bad[:5]])
                ref = align_ref.path_score(x[b], want[b], labels[ly[:b].sum():ly[:b + 1].sum()], int(lx[b]), blank)
                assert abs(sc[b] - ref) <= bound(int(lx[b]), ref), (L, tmode, blank, b, sc[b], ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. random dense log-probs: a valid path with the best score
# ---------------------------------------------------------------------------------------------------------------------------------
def dense_batch(seed, B, T, V, blank, sigma=1.0):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    x = torch.randn((B, T, V), generator=g, device="cuda:0").mul_(sigma).log_softmax(-1)
    rng = np.random.default_rng(seed)
    lx = np.array([T, T, max(1, T - 1), max(1, T // 2), max(1, T // 3), T][:B])
    pool = np.array([v for v in range(V) if v != blank])
    labs = []
    for b in range(B):
        n = int(rng.integers(0, lx[b] // 2 + 2)) if b else int(lx[b] + 1) // 2   # the first: as long as always fits without repeats
        a = pool[rng.integers(0, min(len(pool), 6 if b % 2 else len(pool)), size=n)]    # (odd utterances: six classes, repeats)
        while not align_ref.fits(a, int(lx[b])):
            a = a[:-1]
        labs.append(a)
    return x, np.concatenate(labs).astype(np.int64), lx, np.array([len(a) for a in labs]), labs


def check_against_oracle(x_np, labs, lx, blank, pos, sc, exact_path=False):
    for b, a in enumerate(labs):
        n = int(lx[b])
        ref, rpos = align_ref.viterbi(x_np[b, :n], a, blank)
        assert rpos is not None
        align_ref.check_path(pos[b], a, n, blank)
        mine = align_ref.path_score(x_np[b], pos[b], a, n, blank)
        tol = bound(n, ref)
        assert abs(mine - sc[b]) <= tol, (b, mine, sc[b], tol)          # the score is that of the returned path
        assert abs(mine - ref) <= tol and abs(sc[b] - ref) <= tol, (b, mine, sc[b], ref, tol)   # ... and the best there is
        if exact_path:
            assert np.array_equal(pos[b, :n], rpos), (b, np.nonzero(pos[b, :n] != rpos)[0][:5])


@pytest.mark.parametrize("V", [37, 72, 8192])
@pytest.mark.parametrize("T", [1, 2, 50, 333])
def test_random_dense_scores(crf, T, V):
    blank = (0, V - 1, V // 3)[(T + V) % 3]
    x, labels, lx, ly, labs = dense_batch(100 * T + V, 6, T, V, blank)
    pos, tok, sc, inv = run(crf, x, labels, lx, ly, blank)
    assert np.all(inv == 0)
    check_against_oracle(x.cpu().numpy(), labs, lx, blank, pos, sc)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ties
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 5, 31, 32, 40, 300])
def test_ties_follow_the_rule(crf, L):
    """Uniform log-probs: every alignment has the same score in fp32 as in fp64 (each state's value at frame t is the same chain of t
    additions), so the path is decided by the tie rule alone -- stay, then advance, then skip; state 2L before 2L - 1 -- and must equal
    the oracle's; two calls agree bit for bit."""
    V, blank = 6, 2
    rng = np.random.default_rng(L)
    pool = np.array([v for v in range(V) if v != blank])
    labs = [pool[rng.integers(0, len(pool), size=L)], np.full(L, pool[0]), pool[rng.integers(0, 2, size=max(L - 1, 0))]]
    lx = np.array([int(1.5 * L) + 20, 2 * L + 3, 2 * L + 17])
    T = int(lx.max()) + 1
    x = torch.full((3, T, V), float(np.log(1.0 / V)), device="cuda:0")
    labels, ly = np.concatenate(labs), np.array([len(a) for a in labs])
    first = run(crf, x, labels, lx, ly, blank)
    again = run(crf, x, labels, lx, ly, blank)
    for a, c in zip(first, again):
        assert np.array_equal(a.view(np.int32), c.view(np.int32))
    assert np.all(first[3] == 0)
    check_against_oracle(x.cpu().numpy(), labs, lx, blank, first[0], first[2], exact_path=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. edge cases
# ---------------------------------------------------------------------------------------------------------------------------------
def test_invalid_and_dead_utterances(crf):
    """L + repeats > lx and lx = 0: score -inf, row -2, invalid 1.  -inf columns that leave exactly one alignment: that path.  -inf columns
    that leave none: score -inf, row -2, invalid 0.  ly = 0: all blank, score = the blank column's sum."""
    V, blank, T = 5, 0, 40
    rng = np.random.default_rng(5)
    xn = np.log(rng.dirichlet(np.ones(V), size=(6, T))).astype(np.float32)
    labs = [np.array([1, 1, 2]), np.array([3, 4]), np.array([1, 2, 2, 3]), np.array([1, 2, 2, 3]), np.array([], dtype=np.int64), np.array([2, 3, 4])]
    lx = np.array([3, 0, 30, 30, 17, 40])            # 0: needs 4 frames; 1: no frames; 2: one alignment left; 3: none; 4: empty; 5: ordinary
    cls, want2 = random_alignment(rng, labs[2], 30, blank)
    keep = xn[2, np.arange(30), cls].copy()
    xn[2, :30] = -np.inf
    xn[2, np.arange(30), cls] = keep
    xn[3, :30] = xn[2, :30]
    xn[3, 11, :] = -np.inf                            # a frame nothing can pass
    labels, ly = np.concatenate(labs), np.array([len(a) for a in labs])
    pos, tok, sc, inv = run(crf, torch.tensor(xn, device="cuda:0"), labels, lx, ly, blank)
    assert inv.tolist() == [1, 1, 0, 0, 0, 0]
    for b in (0, 1, 3):
        assert sc[b] == -np.inf and np.all(pos[b] == -2) and np.all(tok[b] == -1), b
    assert np.array_equal(pos[2, :30], want2) and np.all(pos[2, 30:] == -2)
    ref = align_ref.path_score(xn[2], pos[2], labs[2], 30, blank)
    assert abs(sc[2] - ref) <= bound(30, ref)
    assert np.all(pos[4, :17] == -1) and np.all(pos[4, 17:] == -2) and np.all(tok[4, :17] == blank)
    ref = float(xn[4, :17, blank].astype(np.float64).sum())
    assert abs(sc[4] - ref) <= bound(17, ref)
    check_against_oracle(xn[5:], [labs[5]], lx[5:], blank, pos[5:], sc[5:])


def test_public_surface_and_metadata_checks(crf):
    """ctc_crf.ctc_align: three device tensors, no autograd; the metadata checks of the loss apply (label = blank, label >= V, lx > T)."""
    V, blank = 9, 4
    x, labels, lx, ly, labs = dense_batch(9, 4, 30, V, blank)
    x.requires_grad_(True)
    args = [torch.tensor(a, dtype=torch.int32) for a in (labels, lx, ly)]
    pos, tok, sc = crf.ctc_align(x, *args, blank=blank)
    assert pos.is_cuda and tok.is_cuda and sc.is_cuda and not sc.requires_grad and sc.dtype == torch.float32
    pos_t, tok_t, sc_t = crf.ctc_align(x.detach().transpose(0, 1).contiguous(), *args, blank=blank, time_major=True)
    assert torch.equal(pos, pos_t) and torch.equal(tok, tok_t) and torch.equal(sc, sc_t)
    check_against_oracle(x.detach().cpu().numpy(), labs, lx, blank, pos.cpu().numpy(), sc.cpu().numpy())
    bad = args[0].clone(); bad[0] = blank
    with pytest.raises(RuntimeError, match="blank"):
        crf.ctc_align(x.detach(), bad, args[1], args[2], blank=blank)
    bad[0] = V
    with pytest.raises(RuntimeError, match="labels must lie"):
        crf.ctc_align(x.detach(), bad, args[1], args[2], blank=blank)
    with pytest.raises(RuntimeError, match="frame lengths"):
        crf.ctc_align(x.detach(), args[0], args[1] + 100, args[2], blank=blank)
    with pytest.raises(RuntimeError, match="blank must lie"):
        crf.ctc_align(x.detach(), *args, blank=V)


def test_activations_beyond_2_31_elements(crf):
    """Rows past 2^31 elements (64-bit row addresses), both layouts: planted paths in the first and the last utterance of a batch of
    B x T x V > 2^31 uniform activations; the others have empty transcripts."""
    B, T, V, blank = 100, 2800, 8000, 3
    assert B * T * V > 2 ** 31
    if torch.cuda.mem_get_info()[0] < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory")
    rng = np.random.default_rng(31)
    pool = np.array([v for v in range(V) if v != blank])
    labs = [pool[rng.integers(0, len(pool), size=300)] if b in (0, B - 1) else pool[:0] for b in range(B)]
    lx = np.array([T - (b % 7) for b in range(B)])
    plant = {b: random_alignment(rng, labs[b], int(lx[b]), blank) for b in (0, B - 1)}
    labels, ly = np.concatenate(labs), np.array([len(a) for a in labs])
    res = {}
    for tm in (False, True):
        x = torch.full((T, B, V) if tm else (B, T, V), float(np.log(0.1 / (V - 1))), device="cuda:0")
        for b, (cls, _) in plant.items():
            n = int(lx[b])
            row = x[:n, b] if tm else x[b, :n]
            row[torch.arange(n, device="cuda:0"), torch.tensor(cls, device="cuda:0")] = float(np.log(0.9))
        pos0 = torch.full((B, T), SENT_POS, dtype=torch.int32, device="cuda:0")
        sc0 = torch.full((B,), SENT_SCORE, dtype=torch.float32, device="cuda:0")
        pos, tok, sc, inv = crf._C.ctc_align(x, *[torch.tensor(a, dtype=torch.int32) for a in (labels, lx, ly)], blank, tm, pos_out=pos0, scores_out=sc0)
        res[tm] = tuple(a.cpu().numpy() for a in (pos, tok, sc, inv))
        del x, pos, tok, sc, inv
        torch.cuda.empty_cache()
    for a, c in zip(res[False], res[True]):
        assert np.array_equal(a.view(np.int32), c.view(np.int32))
    pos, tok, sc, inv = res[False]
    assert np.all(inv == 0) and not np.any(pos == SENT_POS)
    for b in range(B):
        n = int(lx[b])
        want = plant[b][1] if b in plant else np.full(n, -1)
        assert np.array_equal(pos[b, :n], want) and np.all(pos[b, n:] == -2), b
    assert np.array_equal(tok, tokens_of(pos, labels, ly, blank))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. against the loss
# ---------------------------------------------------------------------------------------------------------------------------------
def test_best_path_below_the_sum_over_paths(crf):
    """scores[b] <= log p_ctc[b] of crf_ctc_fwd_bwd on the same inputs (the best path is one term of the sum), with equality where
    lx = L + repeats leaves one alignment; both layouts."""
    V, blank, T = 37, 36, 60
    x, labels, lx, ly, labs = dense_batch(55, 6, T, V, blank)
    labs[1] = np.array([1, 1, 2, 3, 3, 3, 4, 5, 6, 7])
    lx[1] = 13                                                                # L + repeats: the only alignment
    labs[2] = np.full(7, 5)
    lx[2] = 13                                                                # one repeated label, no spare frame
    labels, ly = np.concatenate(labs), np.array([len(a) for a in labs])
    pos, tok, sc, inv = run(crf, x, labels, lx, ly, blank)
    targs = [torch.tensor(a, dtype=torch.int32) for a in (labels, lx, ly)]
    for tm in (False, True):
        xx = x.transpose(0, 1).contiguous() if tm else x
        _, _, ex = crf._C.loss_fwd_bwd(xx, *targs, 0.0, -1.0, None, True, time_major=tm, blank=blank)
        costs = ex["costs_ctc"].cpu().numpy().astype(np.float64)
        assert np.all(ex["invalid"].cpu().numpy() == 0)
        for b in range(6):
            tol = bound(int(lx[b]), costs[b])
            assert sc[b] <= costs[b] + tol, (tm, b, sc[b], costs[b])
            if b in (1, 2):
                assert abs(sc[b] - costs[b]) <= tol, (tm, b, sc[b], costs[b], tol)
