"""GPU tests of the beam search with n-gram LM fusion (ctc_crf.ctc_beam_search(lm=...) / crf_ctc_beam_lm; cat_amd/csrc/k_beam_lm.hip)
against the fp64 yardsticks tests/beam_lm_ref.py and tests/ngram_ref.py (the textbook back-off lookup; it never sees the compiled tables).

Tolerances.  RTOL = 1e-4 is tests/test_gpu_ctc_beam.py's bound on an acoustic score; the fused score adds fp64 sums of fp32 terms to it,
so a fused score is held to RTOL (|acoustic| + |lm|) -- each part to its own magnitude, and a fused score near 0 does not hide an error.
lm_scores alone is held to 1e-5 * sum_i(|alpha lp_i| + |beta|): the table values, alpha * lp and + beta are rounded to fp32 (2^-24
relative each, three roundings of a term), the sum is fp64.  Every call runs batch-major AND time-major with a poisoned workspace; the two
layouts must agree bit for bit."""
import numpy as np
import pytest
import torch

from tests import beam_lm_ref, beam_ref, ngram_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4
LM_RTOL = 1e-5
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def _i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int64).reshape(-1), dtype=torch.int32)


_MODELS = {}


def model(seed, V, order, bos=True, unk=False):
    """(NgramLM, ngram_ref.Ref) of one random model, built once."""
    import ctc_crf
    key = (seed, V, order, bos, unk)
    if key not in _MODELS:
        ng = ngram_ref.random_model(seed, V, order, bos=bos, unk=unk)
        _MODELS[key] = (ctc_crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V))
    return _MODELS[key]


def run(crf, x, lx, W, nbest, C, blank, lm, alpha, beta, fused=False):
    """x: [N,T,V] CUDA tensor, batch-major.  -> (hyps [N,nbest,T], lens, scores, trace [N,T,W], lm_scores [N,nbest]) as numpy, after
    checking that the two layouts agree bit for bit."""
    N, T, V = x.shape
    out = []
    for tm in (False, True):
        xin = x.transpose(0, 1).contiguous() if tm else x
        hyps, hl, hu, sc, tr, ls = crf.ctc_beam_search(xin, _i32(lx), W, nbest, C, blank, tm, fused, return_trace=True, lm=lm, alpha=alpha,
                                                       beta=beta, return_lm_scores=True)
        assert hyps.shape == (N * nbest, T) and sc.shape == (N * nbest,) and tr.shape == (N, T, W) and ls.shape == (N * nbest,)
        assert sc.dtype == torch.float32 and ls.dtype == torch.float32 and tr.dtype == torch.int32
        assert torch.equal(hu.cpu(), torch.arange(N * nbest, dtype=torch.int32) // nbest)
        out.append((hyps.cpu().numpy().reshape(N, nbest, T), hl.cpu().numpy().reshape(N, nbest), sc.cpu().numpy().reshape(N, nbest),
                    tr.cpu().numpy(), ls.cpu().numpy().reshape(N, nbest)))
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the layouts differ"
    return out[0]


def close_fused(got, ac, lm):
    if not np.isfinite(ac):
        return got == ac
    return np.isfinite(got) and abs(got - (ac + lm)) <= RTOL * (abs(ac) + abs(lm))


def lm_slack(ref, alpha, beta, pre):
    hist = ref.start
    s = 0.0
    for c in pre:
        s += abs(alpha * ref.cond(hist, c)) + abs(beta)
        hist = hist + (c,)
    return LM_RTOL * s


def check_bookkeeping(ref, alpha, beta, blank, hyps, lens, scores, lms, what=""):
    """The LM part of every returned rank, from the hypothesis alone: independent of how the search went."""
    for r in range(len(lens)):
        pre = tuple(int(c) for c in hyps[r, :lens[r]])
        assert (hyps[r, lens[r]:] == blank).all(), (what, r)
        if scores[r] == -np.inf:
            assert lens[r] == 0 and lms[r] == 0.0, (what, r)
            continue
        want = alpha * ref.score(pre) + beta * len(pre)
        assert abs(lms[r] - want) <= lm_slack(ref, alpha, beta, pre) + 1e-30, (what, r, pre, lms[r], want)


def check_against_replay(x64, lx, W, C, blank, ref, alpha, beta, hyps, lens, scores, trace, lms, normalize=False, what=""):
    T = x64.shape[0]
    lxc = max(0, min(int(lx), T))
    assert (trace[lxc:] == -1).all(), (what, "trace rows past lx")
    rp = beam_lm_ref.replay(x64, lx, trace, W, C, blank, ref, alpha, beta, normalize)
    print(f"{what} lx={lx}: replay excess {rp['excess']:.3e} {rp['why'] or ''}")
    assert rp["why"] is None and rp["excess"] <= RTOL, (what, lx, rp["excess"], rp["why"])
    assert not np.any(np.isnan(scores))
    for r in range(len(lens)):
        pre, want, l = rp["prefixes"][r], rp["scores"][r], rp["lms"][r]
        if pre is None:
            assert lens[r] == 0 and scores[r] == -np.inf
            pre = ()
        else:
            assert close_fused(scores[r], want - l, l), (what, lx, r, scores[r], want)
        assert lens[r] == len(pre) and tuple(hyps[r, :lens[r]]) == pre, (what, lx, r, hyps[r], pre)
    assert all(scores[r] >= scores[r + 1] for r in range(len(lens) - 1)), (what, lx, scores)
    check_bookkeeping(ref, alpha, beta, blank, hyps, lens, scores, lms, what)
    return rp


ZERO_CASES = [("tie",) + c for c in beam_ref.TIE_CASES] + [("replay",) + c for c in beam_ref.REPLAY_CASES if c[1:5] in ((3, 2, 8, 30), (5, 16, 8, 64), (65, 64, 64, 64))]


@pytest.mark.parametrize("case", ZERO_CASES, ids=lambda c: "%s-seed%d-V%d-W%d-C%d-T%d" % c[:6])
def test_zero_weights_equal_the_lm_free_call(crf, case):
    """alpha = beta = 0 with a random order-3 model: hyps, lengths, scores and trace equal ctc_beam_search without lm BIT FOR BIT -- on
    every exact-tie case (the total order) and three replay cases (merges, re-entry, W = C = 64), in all three dtypes; lm_scores are 0."""
    if case[0] == "tie":
        _, seed, V, W, C, T, blank, groups = case
        x = np.stack([beam_ref.grouped_inputs(seed, T, V, blank, groups)] * 3)
        lxs = (T, T - 1, 1)
    else:
        _, seed, V, W, C, T, lxs, blank = case
        x = beam_ref.make_inputs(seed, len(lxs), T, V)
    lm, _ = model(3, V, 3)
    for dtype in sorted(DTYPES):
        xg = torch.tensor(x).to(DTYPES[dtype]).to("cuda:0")
        for tm in (False, True):
            xin = xg.transpose(0, 1).contiguous() if tm else xg
            want = crf.ctc_beam_search(xin, _i32(lxs), W, W, C, blank, tm, False, return_trace=True)
            got = crf.ctc_beam_search(xin, _i32(lxs), W, W, C, blank, tm, False, return_trace=True, lm=lm, alpha=0.0, beta=0.0,
                                      return_lm_scores=True)
            for k, (a, b) in enumerate(zip(got[:5], want)):
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (dtype, tm, k)
            assert (got[5] == 0).all()


@pytest.mark.parametrize("V", [3, 4])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_exhaustive(crf, V, dtype):
    """V = 3 (lx = 3, 4, 5) and V = 4 (lx = 2, 3, 4: 61 prefixes at four frames, 105 at five), W = 64 >= the number of prefixes,
    C = V - 1: nothing is pruned, so the returned set is every label sequence of finite mass, each with the fused score
    brute force + alpha * textbook LM + beta * len, in the order of those scores (replay); every blank, both normalize values."""
    from tests.test_gpu_ctc_beam import count_prefixes
    lx = [3, 4, 5] if V == 3 else [2, 3, 4]
    T = max(lx)
    assert all(count_prefixes(V, n) <= 64 for n in lx)
    rng = np.random.default_rng(60 + V)
    raw = torch.tensor((2.0 * rng.standard_normal((3, T, V))).astype(np.float32))
    for normalize, order, alpha, beta in ((False, 2, 0.3, 2.0), (True, 3, 1.5, -1.0)):
        lm, ref = model(11, V, order)
        xc = (raw if normalize else torch.log_softmax(raw, -1)).to(DTYPES[dtype])
        x64 = xc.double().numpy()
        xg = xc.to("cuda:0")
        for blank in range(V):
            hyps, lens, scores, trace, lms = run(crf, xg, lx, 64, 64, V - 1, blank, lm, alpha, beta, fused=normalize)
            for b in range(3):
                what = f"V={V} {dtype} normalize={normalize} blank={blank} lx={lx[b]}"
                want = {k: v for k, v in beam_ref.brute(x64[b], lx[b], blank, normalize).items() if v > -np.inf}
                n = int((scores[b] > -np.inf).sum())
                got = {tuple(int(c) for c in hyps[b, r, :lens[b, r]]): scores[b, r] for r in range(n)}
                assert len(got) == n and set(got) == set(want), (what, len(got), len(want))
                for k, v in got.items():
                    assert close_fused(v, want[k], alpha * ref.score(k) + beta * len(k)), (what, k, v, want[k])
                assert (scores[b, n:] == -np.inf).all() and (lens[b, n:] == 0).all()
                check_against_replay(x64[b], lx[b], 64, V - 1, blank, ref, alpha, beta, hyps[b], lens[b], scores[b], trace[b], lms[b], normalize, what)


REPLAY_SHAPES = [(5, 16, 4, 64), (72, 16, 40, 150), (130, 64, 64, 40)]
WEIGHTS = [(a, b) for a in (0.3, 1.5) for b in (-1.0, 0.0, 2.0)]


def replay_setting(si, di, wi):
    """The settings of one replay test: the six (alpha, beta) pairs are crossed with the shapes and dtypes; the order (1, 2, 4), the
    fuse_log_softmax setting and the blank (0, V - 1) rotate with the three indices so that, per shape and dtype, every order meets both
    alphas, and both fuse settings and both blanks meet every order and every beta."""
    alpha, beta = WEIGHTS[wi]
    return alpha, beta, (1, 2, 4)[(wi + di) % 3], bool((wi // 3 + wi + si) & 1), bool((wi + di + si) & 1)


@pytest.mark.parametrize("wi", range(6), ids=lambda i: "a%g-b%g" % WEIGHTS[i])
@pytest.mark.parametrize("di", range(3), ids=lambda i: sorted(DTYPES)[i])
@pytest.mark.parametrize("si", range(3), ids=lambda i: "V%d-W%d-C%d-T%d" % REPLAY_SHAPES[i])
def test_replay(crf, si, di, wi):
    """Two utterances (lx = T and a ragged one): replay of the GPU's own trace in fp64 shows no unchosen candidate beating a chosen one by
    more than RTOL (|acoustic| + |lm|), no structural complaint; the fused scores, prefixes and lm_scores are those of the replayed beam,
    ranks are non-increasing, and the LM bookkeeping holds on the returned hypotheses."""
    V, W, C, T = REPLAY_SHAPES[si]
    dtype = sorted(DTYPES)[di]
    alpha, beta, order, fused, blank_last = replay_setting(si, di, wi)
    blank = V - 1 if blank_last else 0
    lm, ref = model(5, V, order, bos=bool(wi & 1), unk=bool(wi & 2))
    rng = np.random.default_rng([si, di, wi])
    raw = torch.tensor((2.0 * rng.standard_normal((2, T, V))).astype(np.float32))
    xc = (raw if fused else torch.log_softmax(raw, -1)).to(DTYPES[dtype])
    lxs = [T, T // 2 + 1]
    out = run(crf, xc.to("cuda:0"), lxs, W, W, C, blank, lm, alpha, beta, fused=fused)
    x64 = xc.double().numpy()
    for b, lx in enumerate(lxs):
        what = f"{REPLAY_SHAPES[si]} {dtype} alpha={alpha} beta={beta} order={order} fused={fused} blank={blank}"
        rp = check_against_replay(x64[b], lx, W, C, blank, ref, alpha, beta, out[0][b], out[1][b], out[2][b], out[3][b], out[4][b], fused, what)
        assert [p for p in beam_ref.spell(out[3][b], lx, W)] == rp["prefixes"]


@pytest.mark.parametrize("si,wi", [(0, 1), (1, 3), (2, 5)])
def test_acoustic_part_is_a_lower_bound_of_ctc_score(crf, si, wi):
    """scores - lm_scores is the prefix's acoustic mass within the search: at most ctc_score of the hypothesis, up to RTOL |ctc_score| and
    the slack of the LM part (fp32 inputs with log-probs, so that ctc_score takes the same rows)."""
    V, W, C, T = REPLAY_SHAPES[si]
    alpha, beta = WEIGHTS[wi]
    lm, ref = model(5, V, 2)
    x = beam_ref.make_inputs(si + 1, 2, T, V)
    lxs = [T, T // 2 + 1]
    xg = torch.tensor(x, device="cuda:0")
    hyps, lens, scores, trace, lms = run(crf, xg, lxs, W, W, C, 0, lm, alpha, beta)
    hu = torch.arange(2 * W, dtype=torch.int32) // W
    full = crf.ctc_score(xg, torch.tensor(hyps.reshape(2 * W, T)), torch.tensor(lens.reshape(-1)), _i32(lxs), hu, blank=0).cpu().numpy().reshape(2, W)
    seen = 0
    for b in range(2):
        check_bookkeeping(ref, alpha, beta, 0, hyps[b], lens[b], scores[b], lms[b])
        for r in range(W):
            if np.isfinite(scores[b, r]):
                pre = tuple(int(c) for c in hyps[b, r, :lens[b, r]])
                slack = RTOL * abs(full[b, r]) + lm_slack(ref, alpha, beta, pre) + 1e-6 * (abs(scores[b, r]) + abs(lms[b, r]))   # (+ the fp32 roundings of the two outputs)
                assert np.isfinite(full[b, r]) and float(scores[b, r]) - float(lms[b, r]) <= full[b, r] + slack, (b, r, scores[b, r], lms[b, r], full[b, r])
                seen += 1
    assert seen >= W


def test_the_lm_decides(crf):
    """Six frames over (blank, a, b, c): a, then blanks, then b slightly ahead of c -- the acoustic best is (a, b).  A bigram that favours
    c after a (log10 -0.05 against -2 for b) makes (a, c) rank 0 at alpha = 2; without lm, and at alpha = 0, (a, b) stays on top."""
    p = np.array([[0.05, 0.85, 0.05, 0.05], [0.9, 0.04, 0.03, 0.03], [0.9, 0.04, 0.03, 0.03],
                  [0.1, 0.02, 0.48, 0.40], [0.9, 0.04, 0.03, 0.03], [0.9, 0.04, 0.03, 0.03]])
    x = torch.tensor(np.log(p)[None].astype(np.float32), device="cuda:0")
    ng = {(0,): (-1.0, 0.0), (1,): (-0.5, -0.3), (2,): (-0.5, -0.3), (3,): (-0.5, -0.3), (1, 2): (-2.0, 0.0), (1, 3): (-0.05, 0.0)}
    lm = crf.NgramLM.from_ngrams(ng, 4)
    plain = crf.ctc_beam_search(x, _i32([6]), 8, 2, 3)
    assert plain[0][0, :2].tolist() == [1, 2] and plain[1][0] == 2
    zero = crf.ctc_beam_search(x, _i32([6]), 8, 2, 3, lm=lm, alpha=0.0, beta=0.0)
    assert zero[0][0, :2].tolist() == [1, 2]
    fusedr = crf.ctc_beam_search(x, _i32([6]), 8, 2, 3, lm=lm, alpha=2.0, beta=0.0, return_lm_scores=True)
    assert fusedr[0][0, :2].tolist() == [1, 3] and fusedr[1][0] == 2
    ref = ngram_ref.Ref(ng, 4)
    assert abs(float(fusedr[4][0]) - 2.0 * ref.score((1, 3))) < 1e-5 * 2.0 * abs(ref.score((1, 3)))


def check_equals_search(crf, x, lxs, W, C, blank, lm, ref, alpha, beta, what, dtype="fp32", wants=None):
    """Inputs whose reference candidates are apart by >= 1e-5 relative (100 x the fp32 roundings of lmw and of the sums): the GPU's trace,
    hypotheses and lengths must EQUAL beam_lm_ref.search's, the scores within tolerance.  wants: the reference searches of a caller that
    holds them to conditions of its own in place of that gap (the exact-tie cases); dtype: of the activations, which must hold x exactly."""
    xg = torch.tensor(x).to(DTYPES[dtype])
    assert torch.equal(xg.float(), torch.tensor(x))
    hyps, lens, scores, trace, lms = run(crf, xg.to("cuda:0"), lxs, W, W, C, blank, lm, alpha, beta)
    for b, lx in enumerate(lxs):
        if wants is None:
            want = beam_lm_ref.search(x[b], lx, W, W, C, blank, ref, alpha, beta)
            assert want["gap"] >= 1e-5, (what, b, want["gap"])
        else:
            want = wants[b]
        assert (trace[b, lx:] == -1).all(), (what, b, "trace rows past lx")
        assert np.array_equal(trace[b], want["trace"]), (what, b, trace[b][:lx].tolist(), want["trace"][:lx].tolist())
        for r in range(W):
            pre, sc, l = want["nbest"][r] if r < len(want["nbest"]) else ((), -np.inf, 0.0)
            assert lens[b, r] == len(pre) and tuple(hyps[b, r, :lens[b, r]]) == pre, (what, b, r)
            assert close_fused(scores[b, r], sc - l, l), (what, b, r, scores[b, r], sc)
        check_bookkeeping(ref, alpha, beta, blank, hyps[b], lens[b], scores[b], lms[b], what)
    return trace


@pytest.mark.parametrize("closed,order", [(False, 5), (True, 5), (False, 8), (True, 8)], ids=["pruned", "suffix-closed", "pruned-order8", "suffix-closed-order8"])
def test_back_off_depth(crf, closed, order):
    """beam_lm_ref.back_off_case: an order-5 model of unigrams and ONE 5-gram chain -- from the state of (0 1 2 3) every class but 4 backs
    off four times down to the root (suffix-closed: through four sparse rows of the tables; pruned: the tables skip the contexts the model
    does not hold) -- and the same at order 8, the largest the tables and the kernel's walk take (kNgramMaxOrder): from the state of
    (0 .. 6) seven sparse rows, then the root's.  Equality with the reference search."""
    ng, x, (V, W, C, T, blank, alpha, beta) = beam_lm_ref.back_off_case(closed, order)
    lm, ref = crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
    assert lm.order == order
    tr = check_equals_search(crf, x, [T], W, C, blank, lm, ref, alpha, beta, f"order {order}")
    assert tuple(range(order)) in beam_ref.spell(tr[0], T, W)


@pytest.mark.parametrize("case", beam_lm_ref.LM_TIE_CASES, ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5] + ("-live" if c[10] is None else "-zero%d" % c[10]))
def test_exact_ties_under_a_live_lm(crf, case):
    """beam_lm_ref.LM_TIE_CASES: grouped inputs (through bf16: one set of values in all three dtypes) under a model whose values depend
    on the groups only, so candidates tie EXACTLY in the fused score, in fp64 and in the kernel's arithmetic alike, while alpha and beta
    are not 0 and the heads of the rows jump (tests/test_ctc_beam_lm_api.py holds the cases to their conditions; the two that guard
    equality are asserted here again per lx: no two candidates among the ranks 0 .. W that do not tie come nearer than 1e-3 relative, and
    no tie is decided by unequal keys).  replay counts a tie as no excess whichever way it went; here the GPU's trace, label sequences and
    lengths must EQUAL the reference's at lx = T, T - 1 and 1, in fp32, bf16 and fp16: a stay that loses a tie to an extension, the higher
    slot or the higher place first, a head or a next head taken from the wrong end of its ties changes a trace word."""
    seed, V, W, C, T, blank, G, order, alpha, beta, zero_group = case
    x, ng = beam_lm_ref.lm_tie_inputs(case)
    lm, ref = crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
    lxs = (T, T - 1, 1)
    wants = []
    for lx in lxs:
        a = beam_lm_ref.audit_ties(x, lx, W, C, blank, ref, alpha, beta)
        assert a["gap"] >= 1e-3 and a["key_level"] == 0, (case, lx, a)
        wants.append(beam_lm_ref.search(x, lx, W, W, C, blank, ref, alpha, beta))
    assert not np.array_equal(wants[0]["trace"], beam_ref.search(x, T, W, W, C, blank)["trace"])
    for dtype in sorted(DTYPES):
        check_equals_search(crf, np.stack([x] * 3), lxs, W, C, blank, lm, ref, alpha, beta, f"{case} {dtype}", dtype, wants)


def test_row_search_edges(crf):
    """beam_lm_ref.row_edges_case: V = 8192, rows of 0, 1, 2, 3, 63, 64, 65 and 8191 arcs, E_t planted with their first, last and absent
    labels.  Equality with the reference search."""
    ng, rows, x, (V, W, C, T, blank, alpha, beta) = beam_lm_ref.row_edges_case()
    lm, ref = crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
    tr = check_equals_search(crf, x, [T], W, C, blank, lm, ref, alpha, beta, "V=8192 rows")
    found = [p for p in beam_ref.spell(tr[0], T, W) if p and len(p) == 2 and p[1] in rows.get(p[0], ())]
    assert len({p[0] for p in found}) >= 4, found


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_same_bits_across_calls_batches_and_poison(crf, dtype):
    """An utterance's outputs are the same bits in a second call, alone and inside a batch of five (permuted), with fewer ranks asked
    for, and whatever the workspace held on entry (0xFF poison on and off); both layouts inside `run`."""
    N, T, V, W, C, blank = 5, 70, 41, 16, 40, 3
    lm, ref = model(7, V, 4)
    rng = np.random.default_rng(17)
    xg = torch.tensor((2.0 * rng.standard_normal((N, T, V))).astype(np.float32)).to(DTYPES[dtype]).to("cuda:0")
    lx = [70, 1, 33, 0, 69]
    first = run(crf, xg, lx, W, W, C, blank, lm, 0.7, 1.0, fused=True)
    again = run(crf, xg, lx, W, W, C, blank, lm, 0.7, 1.0, fused=True)
    crf._C.set_debug_poison(False)
    try:
        plain = run(crf, xg, lx, W, W, C, blank, lm, 0.7, 1.0, fused=True)
    finally:
        crf._C.set_debug_poison(True)
    perm = [3, 0, 4, 2, 1]
    moved = run(crf, xg[perm].contiguous(), [lx[i] for i in perm], W, W, C, blank, lm, 0.7, 1.0, fused=True)
    alone = run(crf, xg[2:3].contiguous(), lx[2:3], W, W, C, blank, lm, 0.7, 1.0, fused=True)
    three = run(crf, xg, lx, W, 3, C, blank, lm, 0.7, 1.0, fused=True)
    for k in range(5):
        assert np.array_equal(first[k].view(np.int32), again[k].view(np.int32))
        assert np.array_equal(first[k].view(np.int32), plain[k].view(np.int32))
        assert np.array_equal(first[k][perm].view(np.int32), moved[k].view(np.int32))
        assert np.array_equal(first[k][2:3].view(np.int32), alone[k].view(np.int32))
        if k != 3:
            assert np.array_equal(first[k][:, :3].view(np.int32), three[k].view(np.int32))
    assert np.array_equal(first[3], three[3])
    x64 = xg.cpu().double().numpy()
    for b in (0, 2):
        check_against_replay(x64[b], lx[b], W, C, blank, ref, 0.7, 1.0, first[0][b], first[1][b], first[2][b], first[3][b], first[4][b], True, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_long_traces_at_the_widest_beam(crf, dtype):
    """V = 9, C = 8, W = nbest = 64, T = 130 under an order-3 model: the back-trace takes the trace through lm_n's LDS in chunks of 64
    frames x W words -- at W = 64 all of it -- three chunks at lx = 130 and 129, two that end on the boundary at 128, one frame past a
    chunk at 65, one chunk at 64 and a single frame.  Replay per utterance, and the label sequences of ALL 64 ranks are those the trace
    spells."""
    V, W, C, T, blank = 9, 64, 8, 130, 4
    lxs = [130, 129, 128, 65, 64, 1]
    alpha, beta = 0.7, 2.0                                          # (an insertion bonus: the beam's label sequences pass 64 labels)
    lm, ref = model(5, V, 3)
    rng = np.random.default_rng(130)
    xc = torch.log_softmax(torch.tensor((2.0 * rng.standard_normal((len(lxs), T, V))).astype(np.float32)), -1).to(DTYPES[dtype])
    hyps, lens, scores, trace, lms = run(crf, xc.to("cuda:0"), lxs, W, W, C, blank, lm, alpha, beta)
    x64 = xc.double().numpy()
    for b, lx in enumerate(lxs):
        check_against_replay(x64[b], lx, W, C, blank, ref, alpha, beta, hyps[b], lens[b], scores[b], trace[b], lms[b], False, f"long {dtype}")
        pre = beam_ref.spell(trace[b], lx, W)
        assert lx == 1 or all(p is not None for p in pre), (dtype, lx)
        for r in range(W):
            want = pre[r] or ()
            assert lens[b, r] == len(want) and tuple(hyps[b, r, :lens[b, r]]) == want and (hyps[b, r, lens[b, r]:] == blank).all(), (dtype, lx, r)
    assert max(lens[0]) > 64                                        # (a label sequence longer than one chunk of frames)


def test_a_batch_larger_than_the_device(crf):
    """N = 300 utterances -- more workgroups than the device has compute units -- made of 5 distinct inputs in turn, T = 6, W = 8, ragged
    lx with 0, an order-3 model at alpha = 0.7, beta = 1: every utterance's outputs are the bits of a call on the 5 alone."""
    N, T, V, W, C, blank = 300, 6, 11, 8, 8, 2
    assert N > torch.cuda.get_device_properties(0).multi_processor_count
    lm, ref = model(7, V, 3)
    rng = np.random.default_rng(300)
    x5 = torch.tensor((2.0 * rng.standard_normal((5, T, V))).astype(np.float32))
    lx5 = [6, 0, 3, 5, 1]
    idx = np.arange(N) % 5
    base = run(crf, x5.to("cuda:0"), lx5, W, W, C, blank, lm, 0.7, 1.0, fused=True)
    big = run(crf, x5[idx].contiguous().to("cuda:0"), [lx5[i] for i in idx], W, W, C, blank, lm, 0.7, 1.0, fused=True)
    for k in range(5):
        assert np.array_equal(big[k].view(np.int32), base[k][idx].view(np.int32)), k
    x64 = x5.double().numpy()
    for b in range(5):
        check_against_replay(x64[b], lx5[b], W, C, blank, ref, 0.7, 1.0, base[0][b], base[1][b], base[2][b], base[3][b], base[4][b], True, f"batch b={b}")


def test_edges(crf):
    """lx = 0 (rank 0 is the empty prefix at fused score 0, lm 0); classes at -inf and a frame entirely at -inf (the beam dies: every
    rank missing, lm_scores 0, later trace rows -1); V = 2 (one label: every lookup is the same class); nbest = W throughout."""
    from tests.test_gpu_ctc_beam import minus_inf_inputs
    for V, W in ((6, 4), (130, 16)):
        lm, ref = model(9, V, 3)
        xc, blank = minus_inf_inputs(V, "fp32", False)
        lx = [5, 5, 4, 5]
        hyps, lens, scores, trace, lms = run(crf, xc.to("cuda:0"), lx, W, W, 40, blank, lm, 1.5, 2.0)
        x64 = xc.double().numpy()
        for b in range(4):
            check_against_replay(x64[b], lx[b], W, 40, blank, ref, 1.5, 2.0, hyps[b], lens[b], scores[b], trace[b], lms[b], False, f"-inf V={V} b={b}")
        assert (trace[3, 2:] == -1).all() and (lens[3] == 0).all() and (scores[3] == -np.inf).all() and (lms[3] == 0).all()
    lm, ref = model(9, 2, 3)
    x = beam_ref.make_inputs(3, 3, 12, 2)
    lx = [12, 0, 5]
    for blank in (0, 1):
        hyps, lens, scores, trace, lms = run(crf, torch.tensor(x, device="cuda:0"), lx, 8, 8, 8, blank, lm, 0.3, -1.0)
        for b in range(3):
            check_against_replay(x[b].astype(np.float64), lx[b], 8, 8, blank, ref, 0.3, -1.0, hyps[b], lens[b], scores[b], trace[b], lms[b], False, f"V=2 b={b}")
        assert lens[1, 0] == 0 and scores[1, 0] == 0.0 and lms[1, 0] == 0.0 and (scores[1, 1:] == -np.inf).all() and (trace[1] == -1).all()
