"""GPU tests of the weighted multi-hypothesis CTC gradient (ctc_crf._C.ctc_score_grad / crf_ctc_score_grad, ctc_crf.ctc_logp;
cat_amd/csrc/k_score_grad.hip) against the fp64 oracle on the activations repeated per hypothesis on the host (tests/score_grad_ref.py:
reference, driver, tolerances).  Inputs are log_softmax(normal * 2); every call writes into a grad prefilled with NaN and scores prefilled
with a sentinel and runs batch-major AND time-major, which must agree."""
import numpy as np
import pytest
import torch

from tests.score_grad_ref import TOL, check_grad, flat, fold, i32, logp_normal, ref_gamma, run_grad
from tests.util import rel_err

pytestmark = pytest.mark.gpu
KERNEL_OF_L = {31: 1, 32: 2, 63: 2, 64: 4, 127: 4, 128: 8, 255: 8}     # NR of the instantiation, from the call's longest hypothesis


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def dev(a):
    return torch.tensor(a).to("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. parity, small: the shape of small_batch in tests/test_gpu_ctc_score.py
# ---------------------------------------------------------------------------------------------------------------------------------
N1, T1, V1 = 3, 48, 6
LX1 = np.array([48, 31, 9], dtype=np.int32)
_SMALL = {}


def small_batch(blank):
    """N = 3, ragged lx, (7, 0, 4) hypotheses per utterance in shuffled order: lengths 0, 1, 2, 5, 12, one with repeated labels, one with
    L <= lx < L + repeats and one longer than lx = 9 (both invalid).  Computed once per blank, shared and left unchanged."""
    if blank not in _SMALL:
        rng = np.random.default_rng(5100 + blank)
        pool = np.array([v for v in range(V1) if v != blank])
        draw = lambda n: pool[rng.integers(0, len(pool), size=n)].astype(np.int32)
        a, b, c, d = pool[:4]
        u0 = [draw(0), draw(1), draw(2), draw(5), draw(12), np.array([a, a, b, b, a], dtype=np.int32), draw(12)]
        u2 = [draw(2), draw(1), np.array([a, a, b, b, c, c, d, d], dtype=np.int32), draw(12)]
        hyps, utt = u0 + u2, [0] * 7 + [2] * 4
        order = rng.permutation(len(hyps))
        hyps, utt = [hyps[i] for i in order], np.array([utt[i] for i in order])
        logp = logp_normal(rng, N1, T1, V1)
        gamma, cost, valid = ref_gamma(logp, hyps, utt, LX1, blank)
        assert valid.sum() == len(hyps) - 2 and np.all(np.isfinite(cost[valid == 1]))
        w_pos = rng.uniform(0.25, 2.0, size=len(hyps))
        w_mix = rng.normal(size=len(hyps))
        for v in (logp, gamma, cost, valid, utt, w_pos, w_mix):
            v.setflags(write=False)
        _SMALL[blank] = dict(logp=logp, hyps=hyps, utt=utt, gamma=gamma, cost=cost, valid=valid, w_pos=w_pos, w_mix=w_mix)
    return _SMALL[blank]


def check_small(c, g, sc, inv, w, positive, what):
    ref = fold(c["gamma"], c["cost"], c["valid"], c["utt"], w, N1)
    check_grad(g, ref, LX1, positive, what)
    assert not np.any(g[1]), "an utterance without a hypothesis has a zero gradient"
    assert np.array_equal(inv, 1 - c["valid"]) and np.all(np.isinf(sc[c["valid"] == 0]))
    ok = c["valid"] == 1
    assert np.all(np.abs(sc[ok] - c["cost"][ok]) <= TOL * np.abs(c["cost"][ok]))
    return ref


@pytest.mark.parametrize("blank", [0, V1 - 1, 2])
def test_parity_small(crf, blank):
    c = small_batch(blank)
    x = dev(c["logp"])
    g, sc, inv = run_grad(crf._C, x, c["hyps"], c["utt"], LX1, blank, None)
    check_small(c, g, sc, inv, None, True, f"small blank {blank} w=1")
    assert crf._C.last_score_grad_kernel() == "crf_ctc_score_grad_alpha_kernel<1>"
    g, sc, inv = run_grad(crf._C, x, c["hyps"], c["utt"], LX1, blank, c["w_pos"])
    check_small(c, g, sc, inv, c["w_pos"], True, f"small blank {blank} w>0")
    ref_abs = fold(c["gamma"], c["cost"], c["valid"], c["utt"], np.abs(c["w_mix"]), N1)
    g, sc, inv = run_grad(crf._C, x, c["hyps"], c["utt"], LX1, blank, c["w_mix"])
    ref = check_small(c, g, sc, inv, c["w_mix"], False, f"small blank {blank} mixed")
    assert np.linalg.norm(ref) >= 0.1 * np.linalg.norm(ref_abs), "the mixed-sign reference is cancellation noise"


def test_single_hypothesis_rows_sum_to_one(crf):
    c = small_batch(0)
    h = int(np.argmax([len(a) if c["valid"][k] else -1 for k, a in enumerate(c["hyps"])]))
    u = int(c["utt"][h])
    g, sc, inv = run_grad(crf._C, dev(c["logp"]), [c["hyps"][h]], [u], LX1, 0, np.ones(1))
    rows = g[u, :LX1[u]].sum(-1)
    assert np.all(np.abs(rows - 1.0) <= TOL), rows
    assert not np.any(g[[k for k in range(N1) if k != u]])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. scores bit for bit: the first and last length of every instantiation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", sorted(KERNEL_OF_L))
def test_scores_are_ctc_scores_bits(crf, L):
    V, blank = 8, 0
    rng = np.random.default_rng(700 + L)
    pool = np.arange(1, V)
    rep = np.repeat(pool[rng.integers(0, len(pool), size=(L + 2) // 3)], 3)[:L].astype(np.int32)    # runs of three: many repeats
    hyps = [pool[rng.integers(0, len(pool), size=L)].astype(np.int32), rep, pool[rng.integers(0, len(pool), size=L // 2)].astype(np.int32)]
    reps = [int(np.sum(h[1:] == h[:-1])) for h in hyps]
    T = max(len(h) + r for h, r in zip(hyps, reps)) + 5
    utt, lx = [0, 1, 1], [T, T - 2]
    logp = logp_normal(rng, 2, T, V)
    gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
    assert np.all(valid == 1)
    w = rng.uniform(0.25, 2.0, size=3)
    x = dev(logp)
    g, sc, inv = run_grad(crf._C, x, hyps, utt, lx, blank, w)
    assert crf._C.last_score_grad_kernel() == f"crf_ctc_score_grad_alpha_kernel<{KERNEL_OF_L[L]}>"
    for tm in (False, True):
        xx = x.transpose(0, 1).contiguous() if tm else x
        s2, i2 = crf._C.ctc_score(xx, i32(flat(hyps)), i32([len(h) for h in hyps]), i32(lx), i32(utt), blank, tm)
        assert crf._C.last_score_kernel() == f"crf_ctc_score_wave_kernel<{KERNEL_OF_L[L]}>"
        assert np.array_equal(sc.view(np.int32), s2.cpu().numpy().view(np.int32)), (L, tm, sc, s2)
        assert np.array_equal(inv, i2.cpu().numpy())
    check_grad(g, fold(gamma, cost, valid, utt, w, 2), lx, True, f"L = {L}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. frame-loop edges: the prefetch batches of 8 / 8 / 4 / 2 frames and the clamp to lx - 1; L = 0, 1 and L = lx exactly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_lx,nr", [(17, 1), (33, 2)])
def test_frame_loop_edges(crf, max_lx, nr):
    T, V, blank = 40, 6, 1
    lx = [n for n in (1, 2, 15, 16, 17, 32, 33) if n <= max_lx]
    rng = np.random.default_rng(31 + max_lx)
    pool = np.array([v for v in range(V) if v != blank])
    hyps, utt = [], []
    for u, n in enumerate(lx):
        full = pool[(np.arange(n) + u) % len(pool)].astype(np.int32)        # L = lx, no repeats: ONE alignment
        for h in (full[:0], full[:1], full):
            hyps.append(h)
            utt.append(u)
    logp = logp_normal(rng, len(lx), T, V)
    gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
    assert np.all(valid == 1)
    w = rng.uniform(0.25, 2.0, size=len(hyps))
    g, sc, inv = run_grad(crf._C, dev(logp), hyps, utt, lx, blank, w)
    assert crf._C.last_score_grad_kernel() == f"crf_ctc_score_grad_alpha_kernel<{nr}>" and not np.any(inv)
    check_grad(g, fold(gamma, cost, valid, utt, w, len(lx)), lx, True, f"frame loop, lx up to {max_lx}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. reduce-stage edges
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_class(crf):
    """V = 1: only the empty hypothesis exists; its occupancy is 1 in the blank's column for every frame t < lx."""
    lx = [9, 4]
    x = torch.zeros(2, 9, 1, device="cuda:0")
    g, sc, inv = run_grad(crf._C, x, [np.zeros(0, np.int32)] * 3, [0, 1, 1], lx, 0, np.array([1.0, 0.5, 0.25]))
    want = np.zeros((2, 9, 1))
    want[0, :9], want[1, :4] = 1.0, 0.75
    assert np.all(np.abs(g - want) <= TOL) and not np.any(g[1, 4:]) and np.all(sc == 0.0) and not np.any(inv)


@pytest.mark.parametrize("V", [7, 1031])
def test_reduce_stage_edges(crf, V):
    """V = 7 and V = 1031 (more classes than threads, odd); one utterance with 33 hypotheses and one with none; a permutation of the
    list gives the same gradient."""
    N, T, blank = 3, 20, V // 2
    lx = [20, 20, 13]
    rng = np.random.default_rng(V)
    pool = np.array([v for v in range(V) if v != blank])
    hyps = [pool[rng.integers(0, len(pool), size=int(rng.integers(0, 7)))].astype(np.int32) for _ in range(36)]
    utt = np.array([0] * 33 + [2] * 3)
    order = rng.permutation(36)
    hyps, utt = [hyps[i] for i in order], utt[order]
    logp = logp_normal(rng, N, T, V)
    gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
    w = rng.uniform(0.25, 2.0, size=36)
    x = dev(logp)
    g, sc, inv = run_grad(crf._C, x, hyps, utt, lx, blank, w)
    ref = fold(gamma, cost, valid, utt, w, N)
    check_grad(g, ref, lx, True, f"V = {V}")
    assert not np.any(g[1])
    perm = rng.permutation(36)
    g2, sc2, inv2 = run_grad(crf._C, x, [hyps[i] for i in perm], utt[perm], lx, blank, w[perm], layouts=(False,))
    assert np.array_equal(sc2.view(np.int32), sc[perm].view(np.int32)) and np.array_equal(inv2, inv[perm])
    assert rel_err(g2, g) <= TOL
    w_mix = rng.normal(size=36)
    g, _, _ = run_grad(crf._C, x, hyps, utt, lx, blank, w_mix, layouts=(False,))
    check_grad(g, fold(gamma, cost, valid, utt, w_mix, N), lx, False, f"V = {V} mixed")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. -inf
# ---------------------------------------------------------------------------------------------------------------------------------
def test_minus_inf_column(crf):
    """A class column of -inf: the hypotheses that need it score -inf with invalid 0 and add nothing (zero_infinity=True), the others
    match the reference; no NaN anywhere."""
    N, T, V, blank, dead = 2, 24, 6, 0, 3
    lx = [24, 17]
    rng = np.random.default_rng(55)
    logp = logp_normal(rng, N, T, V)
    logp[:, :, dead] = -np.inf
    hyps = [np.array(a, dtype=np.int32) for a in ([1, 2, 4], [1, 3, 2], [], [3], [5, 5, 1], [2, 3, 3, 4])]
    utt = [0, 0, 1, 1, 1, 0]
    gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
    needs = np.array([dead in a for a in hyps])
    assert np.all(valid == 1) and np.all(np.isinf(cost[needs])) and np.all(np.isfinite(cost[~needs]))
    w = rng.uniform(0.25, 2.0, size=len(hyps))
    g, sc, inv = run_grad(crf._C, dev(logp), hyps, utt, lx, blank, w)
    assert not np.any(inv) and np.all(sc[needs] == -np.inf) and np.all(np.isfinite(sc[~needs]))
    check_grad(g, fold(gamma, cost, valid, utt, w, N), lx, True, "-inf column")
    assert not np.any(g[:, :, dead])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def test_autograd_through_log_softmax(crf):
    c = small_batch(2)
    blank, hyps, utt = 2, c["hyps"], c["utt"]
    rng = np.random.default_rng(6)
    raw = (2.0 * rng.standard_normal((N1, T1, V1))).astype(np.float32)
    w = rng.normal(size=len(hyps))
    hl = i32([len(h) for h in hyps])
    # torch, CPU, fp64: log_softmax -> repeat -> ctc_loss(reduction='none', zero_infinity=True) -> the same weighted sum
    lg = torch.tensor(raw, dtype=torch.float64, requires_grad=True)
    rep = torch.log_softmax(lg, -1)[torch.tensor(utt, dtype=torch.long)]
    tgt = torch.zeros(len(hyps), 12, dtype=torch.long)
    for k, a in enumerate(hyps):
        tgt[k, :len(a)] = torch.tensor(a, dtype=torch.long)
    nll = torch.nn.functional.ctc_loss(rep.transpose(0, 1), tgt, torch.tensor(LX1[utt], dtype=torch.long), hl.long(), blank=blank,
                                       reduction="none", zero_infinity=True)
    (torch.tensor(w) * nll).sum().backward()
    want = lg.grad.numpy()
    for tm in (False, True):
        logits = dev(raw).requires_grad_(True)
        x = torch.log_softmax(logits, -1)
        x = x.transpose(0, 1).contiguous() if tm else x
        scores, inv = crf.ctc_logp(x, i32(flat(hyps)), hl, i32(LX1), i32(utt), blank, tm)
        assert scores.requires_grad and not inv.requires_grad
        with torch.no_grad():
            s2, i2 = crf._C.ctc_score(x.detach(), i32(flat(hyps)), hl, i32(LX1), i32(utt), blank, tm)
        assert torch.equal(scores.detach().view(torch.int32), s2.view(torch.int32)) and torch.equal(inv, i2)
        fin = torch.isfinite(scores.detach())
        assert fin.cpu().numpy().tolist() == (c["valid"] == 1).tolist()
        loss = -(dev(w.astype(np.float32))[fin] * scores[fin]).sum()
        loss.backward()
        got = logits.grad.cpu().numpy()
        e = rel_err(got, want)
        print(f"[score_grad] autograd time_major={tm}: rel_err {e:.3e}")
        assert not np.any(np.isnan(got)) and e <= TOL, e


def test_sample_then_logp_round_trip(crf):
    """The docstring's recipe: ctc_sample -> ctc_logp -> a risk-weighted sum -> backward."""
    N, T, V, K = 2, 30, 7, 4
    rng = np.random.default_rng(8)
    logits = dev((2.0 * rng.standard_normal((N, T, V))).astype(np.float32)).requires_grad_(True)
    log_probs = torch.log_softmax(logits, -1)
    lx = i32([30, 22])
    hyps, hyp_lengths, hyp_utt = crf.ctc_sample(log_probs, lx, K, 1234)
    scores, inv = crf.ctc_logp(log_probs, hyps.cpu(), hyp_lengths.cpu(), lx, hyp_utt.cpu())
    assert not bool(inv.any()) and bool(torch.isfinite(scores).all())
    risk = dev(rng.uniform(0.0, 1.0, size=(N, K)).astype(np.float32))
    (torch.softmax(scores.view(N, K), -1) * risk).sum().backward()
    g = logits.grad
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and not bool(g[1, 22:].any())


def test_logp_refuses_long_hypotheses_only_with_a_gradient(crf):
    """Beyond 255 labels there is no gradient kernel: refused up front when log_probs requires grad, scored as ctc_score does otherwise."""
    N, T, V, L = 1, 300, 5, 256
    rng = np.random.default_rng(9)
    x = dev(logp_normal(rng, N, T, V))
    hyp = (np.arange(L) % 4 + 1).astype(np.int32)
    args = (i32(hyp), i32([L]), i32([T]), i32([0]))
    with pytest.raises(RuntimeError, match="255"):
        crf.ctc_logp(x.clone().requires_grad_(True), *args)
    scores, inv = crf.ctc_logp(x, *args)
    assert not scores.requires_grad and torch.equal(scores, crf.ctc_score(x, *args)) and not bool(inv.any())
