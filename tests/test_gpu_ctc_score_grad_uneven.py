"""GPU tests of the weighted multi-hypothesis CTC gradient (crf_ctc_score_grad, cat_amd/csrc/k_score_grad.hip) where
tests/test_gpu_ctc_score_grad.py does not go: log-probs whose cost per frame is uneven (tests/score_grad_ref.py: UNEVEN_CASES, held to
their regime by tests/test_score_grad_uneven_inputs.py), utterances of 3 000 frames, more hypotheses than one chunk of the reduce stage
lists, and every number of frames per reduce workgroup.  Reference, driver and tolerances are tests/score_grad_ref.py's: the fp64 oracle,
NaN-prefilled outputs, both layouts, TOL = 1e-4."""
import numpy as np
import pytest
import torch

from tests.score_grad_ref import TOL, UNEVEN_CASES, check_grad, fold, logp_normal, ref_gamma, run_grad, uneven_case
from tests.test_gpu_ctc_variants import MODES, _run
from tests.util import rel_err

pytestmark = pytest.mark.gpu


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


def check_call(c, g, sc, inv, w, N, positive, what):
    """Gradient, scores, invalid and -- for positive weights -- the rows' sums: row t < lx of an utterance sums to its hypotheses'
    weights (every hypothesis of these calls is live)."""
    ref = fold(c["gamma"], c["cost"], c["valid"], c["utt"], w, N)
    check_grad(g, ref, c["lx"], positive, what)
    assert np.array_equal(inv, 1 - c["valid"])
    ok = c["valid"] == 1
    assert np.all(np.abs(sc[ok] - c["cost"][ok]) <= TOL * np.abs(c["cost"][ok])), (what, sc, c["cost"])
    if positive:
        for u in range(N):
            sw = float(np.sum(np.asarray(w)[(np.asarray(c["utt"]) == u) & ok]))
            rows = g[u, :int(c["lx"][u])].astype(np.float64).sum(-1)
            assert np.all(np.abs(rows - sw) <= TOL * sw), (what, u, float(np.abs(rows - sw).max()), sw)
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. uneven cost per frame, in every instantiation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(UNEVEN_CASES))
def test_uneven_cost_profiles(crf, name):
    c = uneven_case(name)
    g, sc, inv = run_grad(crf._C, dev(c["logp"]), c["hyps"], c["utt"], c["lx"], c["blank"], c["w_pos"])
    assert crf._C.last_score_grad_kernel() == f"crf_ctc_score_grad_alpha_kernel<{c['nr']}>"
    check_call(c, g, sc, inv, c["w_pos"], 2, True, f"uneven {name}")


def test_uneven_cost_profile_mixed_weights(crf):
    c = uneven_case("right_wrong_right_L100")
    g, sc, inv = run_grad(crf._C, dev(c["logp"]), c["hyps"], c["utt"], c["lx"], c["blank"], c["w_mix"])
    ref = check_call(c, g, sc, inv, c["w_mix"], 2, False, "uneven right_wrong_right_L100 mixed")
    ref_abs = fold(c["gamma"], c["cost"], c["valid"], c["utt"], np.abs(c["w_mix"]), 2)
    assert np.linalg.norm(ref) >= 0.1 * np.linalg.norm(ref_abs), "the mixed-sign reference is cancellation noise"


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. long stationary utterances: the fp64 vectors over 3 000 frames; lx = 2 999 ends the prefetch batches of 8 / 8 / 4 / 2 frames unevenly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,nr", [(10, 1), (255, 8)])
def test_long_stationary_utterances(crf, L, nr):
    T, V, blank = 3000, 8, 0
    rng = np.random.default_rng(3000 + L)
    pool = np.arange(1, V)
    hyps = [pool[rng.integers(0, len(pool), size=n)].astype(np.int32) for n in (L, L, L // 2)]
    c = dict(hyps=hyps, utt=np.array([0, 1, 1]), lx=np.array([T, T - 1], dtype=np.int32), blank=blank)
    logp = logp_normal(rng, 2, T, V)
    c["gamma"], c["cost"], c["valid"] = ref_gamma(logp, hyps, c["utt"], c["lx"], blank)
    assert np.all(c["valid"] == 1) and np.all(np.isfinite(c["cost"]))
    w = rng.uniform(0.25, 2.0, size=3)
    g, sc, inv = run_grad(crf._C, dev(logp), hyps, c["utt"], c["lx"], blank, w)
    assert crf._C.last_score_grad_kernel() == f"crf_ctc_score_grad_alpha_kernel<{nr}>"
    check_call(c, g, sc, inv, w, 2, True, f"T = 3000, L = {L}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. more hypotheses than one chunk (256) of the reduce stage's list
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hypothesis_chunks(crf):
    """H = 600 over three utterances.  Live hypotheses: utterance 0 only at h >= 261 (its first chunk is empty), utterance 1 at
    h = 250 .. 260 and 505 .. 520 (across both chunk edges), utterance 2 at h = 599 alone.  Everything else is dead, each in one of five
    ways: weight 0, weight -0.0, a label whose column is -inf (twice as often), too long for its utterance's frames."""
    N, T, V, blank, dead_col, H = 3, 12, 6, 0, 5, 600
    lx = np.array([12, 9, 3], dtype=np.int32)
    rng = np.random.default_rng(600)
    logp = logp_normal(rng, N, T, V)
    logp[:, :, dead_col] = -np.inf
    live_pool = np.arange(1, dead_col)
    hyps, utt, w, live = [], np.zeros(H, dtype=np.int64), rng.uniform(0.25, 2.0, size=H), np.zeros(H, dtype=bool)
    for h in range(H):
        owner = 1 if 250 <= h <= 260 or 505 <= h <= 520 else 2 if h == 599 else 0 if h >= 261 and h % 7 else -1
        n = int(rng.integers(0, 5))
        a = live_pool[rng.integers(0, len(live_pool), size=n)].astype(np.int32)
        if owner == 2:
            a = a[:1]
        if owner >= 0:
            utt[h], live[h] = owner, True
        else:
            kind = h % 5
            utt[h] = h % 3
            if kind == 0:
                w[h] = 0.0
            elif kind == 1:
                w[h] = -0.0
            elif kind in (2, 3):
                a = np.append(a[:3], dead_col).astype(np.int32)
            else:
                utt[h], a = 2, live_pool[np.arange(4) % len(live_pool)].astype(np.int32)     # 4 labels in 3 frames
        hyps.append(a)
    assert not np.any(live[:250]) and not np.any(live & (utt == 0) & (np.arange(H) < 261)) and np.sum(live & (utt == 2)) == 1
    assert sorted({len(a) for a in hyps}) == [0, 1, 2, 3, 4]
    gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
    counted = (valid == 1) & np.isfinite(cost) & (w != 0)
    assert np.array_equal(counted, live), "the live hypotheses are the planned ones"
    assert np.any(valid == 0) and np.any((valid == 1) & np.isinf(cost)) and np.any(np.signbit(w) & (w == 0))
    ref = fold(gamma, cost, valid, utt, w, N)
    x = dev(logp)
    g, sc, inv = run_grad(crf._C, x, hyps, utt, lx, blank, w)
    check_grad(g, ref, lx, True, "H = 600")
    assert not np.any(g[:, :, dead_col])
    assert np.array_equal(inv, 1 - valid) and np.all(sc[(valid == 0) | np.isinf(cost)] == -np.inf)
    fin = (valid == 1) & np.isfinite(cost)
    assert np.all(np.abs(sc[fin] - cost[fin]) <= TOL * np.abs(cost[fin]))
    for u in range(N):
        sw = float(w[live & (utt == u)].sum())
        assert np.all(np.abs(g[u, :lx[u]].astype(np.float64).sum(-1) - sw) <= TOL * sw), u
    perm = rng.permutation(H)
    g2, sc2, inv2 = run_grad(crf._C, x, [hyps[i] for i in perm], utt[perm], lx, blank, w[perm], layouts=(False,))
    assert np.array_equal(sc2.view(np.int32), sc[perm].view(np.int32)) and np.array_equal(inv2, inv[perm])
    assert rel_err(g2, g) <= TOL
    check_grad(g2, ref, lx, True, "H = 600 permuted")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the reduce stage's geometry: FB = min(8, 8192 / V) frames per workgroup = 4, 3, 2, 1, 1
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,blank_last", [(2048, False), (2049, False), (4096, False), (4097, False), (4097, True), (8192, False)])
def test_reduce_stage_geometry(crf, V, blank_last):
    N, T = 3, 11
    lx = np.array([11, 7, 1], dtype=np.int32)
    blank = V - 1 if blank_last else 0
    top = V - 2 if blank_last else V - 1                     # the last column that is a label
    rng = np.random.default_rng(V + blank)
    lo = 0 if blank_last else 1
    draw = lambda n: rng.integers(lo, top + 1, size=n).astype(np.int32)
    hyps = [draw(3), np.array([top, lo, top], dtype=np.int32), draw(0), draw(5),
            draw(2), np.array([top], dtype=np.int32), draw(3),
            draw(0), np.array([top], dtype=np.int32), draw(1)]
    utt = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, 2])
    logp = logp_normal(rng, N, T, V)
    gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
    assert np.all(valid == 1) and np.all(np.isfinite(cost))
    w = rng.uniform(0.25, 2.0, size=len(hyps))
    c = dict(gamma=gamma, cost=cost, valid=valid, utt=utt, lx=lx)
    g, sc, inv = run_grad(crf._C, dev(logp), hyps, utt, lx, blank, w)
    check_call(c, g, sc, inv, w, N, True, f"V = {V} blank {blank}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the same profiles through the loss call's numerator (its chains rescale per frame)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "robust_ctc", "no_tilt"])
@pytest.mark.parametrize("name", ["right_wrong_L20", "wrong_right_L20", "right_wrong_L255"])
def test_uneven_cost_profiles_through_the_loss_call(crf, name, mode):
    c = uneven_case(name)
    hyps, lx = c["hyps"][:2], c["lx"]                        # one label sequence per utterance: the empty hypothesis stays out
    labels = np.concatenate(hyps).astype(np.int32)
    ly = np.array([len(a) for a in hyps], dtype=np.int32)
    costs, g, inv, _ = _run(crf._C, c["logp"], labels, lx, ly, c["blank"], False, MODES[mode])
    assert np.all(np.isfinite(g)) and not np.any(inv)
    print(f"[score_grad] loss call {name} {mode}: costs {costs} oracle {c['cost'][:2]}")
    assert np.allclose(costs, c["cost"][:2], rtol=TOL, atol=0), (costs, c["cost"][:2])
    for b in range(2):
        e = rel_err(g[b], c["gamma"][b])
        print(f"[score_grad] loss call {name} {mode} utterance {b}: rel_err {e:.3e}")
        assert e <= TOL, (b, e)
        assert np.allclose(g[b, :lx[b]].sum(-1), 1.0, atol=1e-4), b
        assert not np.any(g[b, lx[b]:])
