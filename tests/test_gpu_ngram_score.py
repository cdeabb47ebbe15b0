"""GPU tests of ctc_crf.ngram_score / crf_ngram_score (cat_amd/csrc/k_ngram.hip): bit equality of the per-position values with the host
walk NgramLM.token_scores, the scores against the fp64 sum of those values and against the textbook of tests/ngram_score_ref.py (which
never sees the compiled tables), the search's lm_scores, the edges of the row search, order 8, the same bits in any batch, invalid rows,
more than 65 535 rows, no host synchronisation, and the N-best chain ctc_beam_search -> ctc_score + ngram_score -> ctc_edit_distance.

Tolerances.  A score is the fp64 sum of fp32 values rounded to fp32 once: the kernel's fp64 sum is exact to far below half an fp32 ulp,
so it may differ from the host's fp64 sum rounded only at a tie -- held to one ulp, 2^-23 |score|.  Against the textbook: 1e-6 of the sum
of the magnitudes of all terms (tests/test_ngram_lm.py's bound per look-up, summed)."""
import numpy as np
import pytest
import torch

from tests import ngram_ref
from tests.ngram_score_ref import ScoreRef

pytestmark = pytest.mark.gpu
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ULP = 2.0 ** -23
DEV = "cuda:0"


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


def suffix_closed(ng, seed):
    """The dict with every suffix (and every prefix of those) of its n-grams added: no pruned context."""
    rng = np.random.default_rng(seed)
    out = dict(ng)
    todo = [k for k in ng if ngram_ref.EOS not in k]
    while todo:
        k = todo.pop()
        for sub in (k[1:], k[:-1]):
            if sub and sub not in out:
                out[sub] = (round(float(-0.1 - 2.9 * rng.random()), 4), round(float(-1.0 + 1.2 * rng.random()), 4))
                todo.append(sub)
    return out


_MODELS = {}


def model(seed, V, order, bos=True, unk=False, closed=False):
    """(NgramLM, ScoreRef, the n-gram dict) of one random model with </s> entries, built once."""
    import ctc_crf
    key = (seed, V, order, bos, unk, closed)
    if key not in _MODELS:
        ng = ngram_ref.random_model(seed, V, order, bos=bos, unk=unk, eos=True)
        if closed:
            ng = suffix_closed(ng, seed)
        _MODELS[key] = (ctc_crf.NgramLM.from_ngrams(ng, V), ScoreRef(ng, V), ng)
    return _MODELS[key]


def draw_row(rng, grams, V, n):
    """n tokens: n-grams of the model (so that long matches occur) between single random tokens."""
    row = []
    while len(row) < n:
        if grams and rng.random() < 0.6:
            row += list(grams[int(rng.integers(len(grams)))])
        else:
            row.append(int(rng.integers(V)))
    return row[:n]


def class_grams(ng):
    top = max(len(k) for k in ng)
    return [k for k in ng if len(k) >= max(2, top - 1) and all(isinstance(w, int) for w in k)]


def pack(rows, W, lens=None, fill=I32_MIN):
    """-> (hyps [H, W] int32 with `fill` behind every length, hyp_lengths [H] int32) on the device."""
    h = np.full((len(rows), W), fill, dtype=np.int64)
    for i, r in enumerate(rows):
        h[i, :len(r)] = r
    lens = [len(r) for r in rows] if lens is None else lens
    return torch.tensor(h, dtype=torch.int32).to(DEV), torch.tensor(lens, dtype=torch.int32).to(DEV)


def score(crf, lm, rows, W, bos=True, eos=False, tokens=True, lens=None):
    """-> numpy (scores, invalid, token_logp, token_order) of one call."""
    hyps, hl = pack(rows, W, lens)
    out = crf.ngram_score(hyps, hl, lm, bos=bos, eos=eos, return_token_scores=tokens)
    assert out[0].shape == (len(rows),) and out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and not out[0].requires_grad
    if tokens:
        assert out[2].shape == out[3].shape == (len(rows), W) and out[2].dtype == torch.float32 and out[3].dtype == torch.int32
    return tuple(t.cpu().numpy() for t in out) + ((None, None) if not tokens else ())


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_against_host_walk(crf, lm, rows, W, bos, eos):
    sc, inv, tl, to = score(crf, lm, rows, W, bos, eos)
    assert not inv.any()
    for h, r in enumerate(rows):
        L = len(r)
        lps, orders = lm.token_scores(r, bos=bos)
        assert np.array_equal(bits(tl[h, :L]), bits(np.asarray(lps, dtype=np.float32))), (h, L, "token_logp")
        assert np.array_equal(to[h, :L], np.asarray(orders, dtype=np.int32)), (h, L, to[h, :L], orders)
        assert not tl[h, L:].any() and not to[h, L:].any() and not np.signbit(tl[h, L:]).any(), (h, "behind the length")
        s = (lm.start if bos else 0)
        for c in r:
            s = lm.lookup(s, c)[1]
        want = float(np.sum(np.asarray(lps, dtype=np.float64))) + (float(lm.eos_logp[s]) if eos else 0.0)
        assert abs(float(sc[h]) - want) <= ULP * abs(want), (h, L, sc[h], want)
    return sc, tl, to


LENGTHS = lambda order: sorted({n for n in (0, 1, order - 2, order - 1, order, 63, 64, 65, 127, 128, 129, 300) if n >= 0})
CONFIGS = [(order, V, closed, bos, unk) for order in (1, 2, 3, 5, 8) for V, closed, bos, unk in
           ((3, False, True, False), (9, True, False, False), (300, False, True, True), (9, False, False, True), (300, True, True, False))]


@pytest.mark.parametrize("order,V,closed,bos,unk", CONFIGS)
def test_bit_equal_with_the_host_walk(crf, order, V, closed, bos, unk):
    lm, _, ng = model(21, V, order, bos, unk, closed)
    assert lm.order == order and lm.eos_logp is not None
    rng = np.random.default_rng([order, V])
    grams = class_grams(ng) if order > 1 else []
    rows = [draw_row(rng, grams, V, n) for n in LENGTHS(order)]            # ONE list with all the lengths
    deep = 0
    for with_bos in (True, False):
        for eos in (False, True):
            _, _, to = check_against_host_walk(crf, lm, rows, 320, with_bos, eos)
            deep = max(deep, int(to.max()))
    assert deep == order, (deep, order)                                     # the longest n-grams are reached
    assert crf._C.last_ngram_score_kernel() == "crf_ngram_score_kernel<tokens>"


@pytest.mark.parametrize("order,bos,unk", [(3, True, False), (5, True, True), (5, False, False), (3, False, True)])
def test_against_the_textbook(crf, order, bos, unk):
    """Pruned contexts (random_model as it is): where a state resolved from the last order - 1 tokens alone could differ from the state
    of the sequential walk, if the argument in k_ngram.hip were wrong."""
    V = 9
    lm, ref, ng = model(22, V, order, bos, unk)
    rng = np.random.default_rng(order)
    grams = class_grams(ng)
    rows = [draw_row(rng, grams, V, n) for n in (0, 1, 2, 5, 17, 64, 65, 150)] + [draw_row(rng, [], V, 40)]
    for with_bos in (True, False):
        for eos in (False, True):
            sc, inv, tl, to = score(crf, lm, rows, 160, with_bos, eos)
            for h, r in enumerate(rows):
                want, mass = ref.score(r, with_bos, eos), ref.mass_score(r, with_bos, eos)
                assert abs(float(sc[h]) - want) <= 1e-6 * mass + 1e-30, (h, with_bos, eos, sc[h], want)
                assert to[h, :len(r)].tolist() == ref.orders(r, with_bos), (h, with_bos)
    assert crf._C.last_ngram_score_kernel() == "crf_ngram_score_kernel<tokens>"


def test_against_the_search(crf):
    N, T, V, W = 3, 40, 9, 8
    lm, _, _ = model(23, V, 3)
    rng = np.random.default_rng(5)
    x = torch.log_softmax(torch.tensor(rng.standard_normal((N, T, V)).astype(np.float32)), -1).to(DEV)
    lx = torch.tensor([40, 0, 27], dtype=torch.int32)
    for alpha, beta in ((0.5, 1.0), (1.25, -0.5), (0.3, 0.0)):
        hyps, hl, hu, sc, ls = crf.ctc_beam_search(x, lx, W, W, 8, 0, lm=lm, alpha=alpha, beta=beta, return_lm_scores=True)
        lm_s, inv, tl, _ = crf.ngram_score(hyps, hl, lm, return_token_scores=True)
        assert not inv.any().item()
        lens, got, want = hl.cpu().numpy(), lm_s.cpu().double().numpy(), ls.cpu().double().numpy()
        tl, missing = tl.cpu().double().numpy(), 0
        for h in range(N * W):
            total = alpha * got[h] + beta * lens[h]
            slack = ULP * (np.abs(alpha * tl[h, :lens[h]]).sum() + abs(beta) * lens[h] + abs(total))
            assert abs(total - want[h]) <= slack, (alpha, beta, h, total, want[h], slack)
            if lens[h] == 0 and not np.isfinite(sc[h].item()):
                missing += 1
                assert got[h] == 0.0 and want[h] == 0.0
        assert missing == W - 1                                             # (utterance 1 has no frames: the empty prefix alone)


def test_row_search_edges(crf):
    """V = 8192, order 2: contexts whose rows hold 0, 1, 2, 8 191 and 8 192 arcs; the first and the last label of a row and labels just
    outside it."""
    V = 8192
    ng = {(c,): (-1.0 - (c % 7) * 0.25, -0.125 * (1 + c % 5)) for c in range(V)}
    rows_of = {11: [5], 12: [100, 8000], 13: [c for c in range(V) if c != 4000], 14: list(range(V))}          # (10: no arcs)
    for ctx, labs in rows_of.items():
        for c in labs:
            ng[(ctx, c)] = (-0.5 - (c % 11) * 0.125, 0.0)
    ng[(ngram_ref.EOS,)] = (-2.0, 0.0)
    lm = crf.NgramLM.from_ngrams(ng, V)
    assert lm.order == 2 and lm.num_states == V + 1
    probes = {10: [0, 5, 8191], 11: [5, 4, 6, 0, 8191], 12: [100, 8000, 99, 101, 7999, 8001, 0, 8191], 13: [0, 8191, 4000, 3999, 4001],
              14: [0, 8191, 4000]}
    rows = [[ctx, c] for ctx, cs in probes.items() for c in cs]
    _, _, to = check_against_host_walk(crf, lm, rows, 2, False, True)
    for h, (ctx, c) in enumerate(rows):
        assert to[h, 1] == (2 if c in rows_of.get(ctx, ()) else 1), (ctx, c)


def test_order_eight(crf):
    """Seven sparse rows walked from the deepest state, and a row whose every position backs off to the root."""
    V = 3
    ng = {(c,): (-0.5 - 0.125 * c, -0.25) for c in range(V)}
    for n in range(2, 9):
        ng[(0, 1) * (n // 2) + (0,) * (n % 2)] = (-0.125 * n, -0.5 if n < 8 else 0.0)
    ng[(ngram_ref.EOS,)] = (-1.5, 0.0)
    lm = crf.NgramLM.from_ngrams(ng, V)
    assert lm.order == 8 and max(len(h) for h in lm.state_history) == 7
    rows = [[0, 1] * 40, [0, 1, 0, 1, 0, 1, 0, 2] * 9, [2] * 70, [0, 1, 0, 1, 0, 1, 0, 1, 2, 0, 1]]
    for bos in (True, False):
        _, _, to = check_against_host_walk(crf, lm, rows, 96, bos, True)
        # (0 1)*: "1" completes the 8-gram; behind it the longest state is the 6-gram (0 1 0 1 0 1), and "0" completes the 7-gram
        assert set(to[0, 7:80:2].tolist()) == {8} and set(to[0, 8:80:2].tolist()) == {7} and to[2, :70].tolist() == [1] * 70
        assert to[1, 7] == 1 and to[1, 6] == 7                             # "2" behind the seven-token state: seven back-offs to the root


def test_same_bits_in_any_batch(crf):
    V, W = 9, 200
    lm, _, ng = model(24, V, 5)
    rng = np.random.default_rng(9)
    grams = class_grams(ng)
    rows = [draw_row(rng, grams, V, int(n)) for n in rng.integers(0, W + 1, size=301)]
    rows[7] = draw_row(rng, grams, V, 129)
    base = score(crf, lm, rows, W, True, True)
    again = score(crf, lm, rows, W, True, True)
    perm = rng.permutation(len(rows))
    moved = score(crf, lm, [rows[i] for i in perm], W, True, True)
    alone = score(crf, lm, [rows[7]], W, True, True)
    plain = score(crf, lm, rows, W, True, True, tokens=False)
    assert crf._C.last_ngram_score_kernel() == "crf_ngram_score_kernel<scores>"
    for k in range(4):
        assert np.array_equal(bits(base[k]), bits(again[k]))
        assert np.array_equal(bits(base[k][perm]), bits(moved[k]))
        assert np.array_equal(bits(base[k][7:8]), bits(alone[k]))
    assert np.array_equal(bits(base[0]), bits(plain[0])) and np.array_equal(base[1], plain[1])
    # rows a stride apart against the contiguous copy
    hyps, hl = pack(rows, W)
    wide = torch.full((len(rows), W + 37), I32_MAX, dtype=torch.int32, device=DEV)
    wide[:, :W] = hyps
    view = wide[:, :W]
    assert not view.is_contiguous()
    out = crf.ngram_score(view, hl, lm, eos=True, return_token_scores=True)
    for k in range(4):
        assert out[k].shape == base[k].shape and np.array_equal(bits(out[k].cpu().numpy()), bits(base[k]))


def test_invalid_rows(crf):
    V, W, L = 9, 140, 130
    lm, _, ng = model(25, V, 3)
    rng = np.random.default_rng(3)
    good = [draw_row(rng, class_grams(ng), V, n) for n in (L, 64, 1, L)]
    want = score(crf, lm, good, W, True, True)
    rows, lens, bad = [], [], []
    for n in (-1, W + 1, I32_MIN):                                          # lengths out of range: nothing of the row is read
        rows.append(good[0]); lens.append(n); bad.append(True)
    for tok in (V, -1, I32_MAX):
        for at in (0, 63, 64, L - 1):
            r = list(good[0]); r[at] = tok
            rows.append(r); lens.append(L); bad.append(True)
    r = list(good[1]) + [V, -1, I32_MAX]                                     # bad tokens BEHIND the length do not invalidate
    rows.append(r); lens.append(64); bad.append(False)
    keep = len(rows) - 1
    mixed, mixed_len, where = [], [], []
    for i, (r, n) in enumerate(zip(rows, lens)):                            # a good neighbour between any two of them
        mixed += [r, good[i % 4]]; mixed_len += [n, len(good[i % 4])]; where.append(i % 4)
    for tokens in (True, False):
        sc, inv, tl, to = score(crf, lm, mixed, W, True, True, tokens=tokens, lens=mixed_len)
        for i, b in enumerate(bad):
            assert inv[2 * i] == int(b), (i, lens[i])
            if b:
                assert sc[2 * i] == -np.inf and (not tokens or (not tl[2 * i].any() and not to[2 * i].any())), i
            g = where[i]
            assert bits(sc[2 * i + 1:2 * i + 2]) == bits(want[0][g:g + 1]) and inv[2 * i + 1] == 0
            if tokens:
                assert np.array_equal(bits(tl[2 * i + 1]), bits(want[2][g])) and np.array_equal(to[2 * i + 1], want[3][g])
        assert bits(sc[2 * keep:2 * keep + 1]) == bits(want[0][1:2])
        if tokens:
            assert np.array_equal(bits(tl[2 * keep]), bits(want[2][1])) and np.array_equal(to[2 * keep], want[3][1])
    # a row masked with length -1 stays out of a sum the caller forms over the valid rows
    assert np.isfinite(sc[inv == 0]).all() and (sc[inv == 1] == -np.inf).all()


def test_more_rows_than_a_grid_dimension(crf):
    """H = 70 000 > 65 535 rows of W = 4: every row the bits of its content scored alone."""
    H, W, V = 70000, 4, 3
    lm, _, _ = model(26, V, 3)
    rng = np.random.default_rng(1)
    hyps = rng.integers(0, V, size=(H, W)).astype(np.int32)
    lens = rng.integers(0, W + 1, size=H).astype(np.int32)
    sc, inv, tl, to = crf.ngram_score(torch.tensor(hyps).to(DEV), torch.tensor(lens).to(DEV), lm, eos=True, return_token_scores=True)
    sc, inv, tl, to = sc.cpu().numpy(), inv.cpu().numpy(), tl.cpu().numpy(), to.cpu().numpy()
    masked = np.where(np.arange(W)[None, :] < lens[:, None], hyps, -1)
    contents, index = np.unique(masked, axis=0, return_inverse=True)
    index = index.reshape(-1)
    assert len(contents) == sum(V ** k for k in range(W + 1))
    rows = [[int(c) for c in r if c >= 0] for r in contents]
    one = score(crf, lm, rows, W, True, True)
    assert not inv.any()
    assert np.array_equal(bits(sc), bits(one[0][index])) and np.array_equal(bits(tl), bits(one[2][index])) and np.array_equal(to, one[3][index])


def test_no_host_synchronisation(crf):
    lm, _, ng = model(27, 9, 3)
    rng = np.random.default_rng(2)
    hyps, hl = pack([draw_row(rng, class_grams(ng), 9, n) for n in (0, 5, 70)], 80)
    crf.ngram_score(hyps, hl, lm, eos=True)                                 # (uploads the tables and eos_logp)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = crf.ngram_score(hyps, hl, lm, eos=True, return_token_scores=True)
        crf.ngram_score(hyps[:, :40].detach(), hl, lm, bos=False)         # (rows a stride apart: a device copy, no read)
        with pytest.raises(RuntimeError):
            out[0][0].item()                                                # the positive control
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.isfinite(out[0].cpu().numpy()).all()


def test_the_nbest_chain(crf):
    """ctc_beam_search (LM-free, nbest = 8) -> ctc_score + ngram_score -> the re-ranked 1-best -> ctc_edit_distance, all on the device,
    against the same chain through .cpu() and NgramLM.score; the LM changes the 1-best of at least one utterance."""
    N, T, V, K = 8, 30, 6, 8
    alpha, beta = 1.5, 0.5
    lm, _, _ = model(28, V, 3)
    rng = np.random.default_rng(28)
    x = torch.log_softmax(torch.tensor(rng.standard_normal((N, T, V)).astype(np.float32)), -1).to(DEV)
    lx = torch.tensor(rng.integers(T - 8, T + 1, size=N), dtype=torch.int32)
    labels = [[int(c) for c in rng.integers(1, V, size=int(n))] for n in rng.integers(5, 15, size=N)]
    lab, ly = torch.tensor([c for r in labels for c in r], dtype=torch.int32), torch.tensor([len(r) for r in labels], dtype=torch.int32)
    hyps, hl, hu, sc = crf.ctc_beam_search(x, lx, 16, K, V - 1)
    ac = crf.ctc_score(x, hyps, hl, lx, hu)
    lm_s, inv = crf.ngram_score(hyps, hl, lm, eos=True)
    total = ac.double() + alpha * lm_s.double() + beta * hl.double()
    total = torch.where(torch.isfinite(sc), total, torch.full_like(total, -float("inf")))   # (a rank the beam does not hold)
    best = total.view(N, K).argmax(1)
    rows = (torch.arange(N, device=DEV) * K + best)
    dist = crf.ctc_edit_distance(hyps[rows].contiguous(), hl[rows].contiguous(), lab, ly)
    # the host chain
    hyps_c, hl_c, ac_c, sc_c = hyps.cpu().numpy(), hl.cpu().numpy(), ac.cpu().double().numpy(), sc.cpu().numpy()
    lm_c = np.array([np.float32(lm.score(hyps_c[h, :hl_c[h]].tolist(), eos=True)) for h in range(N * K)], dtype=np.float64)
    total_c = np.where(np.isfinite(sc_c), ac_c + alpha * lm_c + beta * hl_c, -np.inf)
    best_c = total_c.reshape(N, K).argmax(1)
    assert not inv.any().item() and (np.abs(lm_s.cpu().double().numpy() - lm_c) <= ULP * np.abs(lm_c)).all()
    assert best.cpu().tolist() == best_c.tolist()
    first_c = np.where(np.isfinite(sc_c), ac_c, -np.inf).reshape(N, K).argmax(1)      # the 1-best without the LM
    assert (best_c != first_c).any(), "the LM changes no 1-best: the chain would show nothing"
    want = []
    for n in range(N):
        h = n * K + int(best_c[n])
        want.append(edit(labels[n], hyps_c[h, :hl_c[h]].tolist()))
    assert dist.cpu().tolist() == want


def edit(a, b):
    """Levenshtein distance, the plain row-by-row recursion."""
    d = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        p, d[0] = d[0], i
        for j, y in enumerate(b, 1):
            p, d[j] = d[j], min(p + (x != y), d[j] + 1, d[j - 1] + 1)
    return d[len(b)]
