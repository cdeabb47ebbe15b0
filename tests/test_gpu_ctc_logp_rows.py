"""GPU tests of the weighted hypothesis-score gradient on DEVICE ROWS (ctc_crf.ctc_logp with CUDA hyps, ctc_crf._C.ctc_score_grad on a
ScoreRows, crf_ctc_score_grad_rows; cat_amd/csrc/k_rows.hip): the fp64 oracle and tolerances of tests/score_grad_ref.py, and the
CPU-hypotheses call for the bits of scores and invalid.  In the mixed list every hypothesis runs through the recursions of its own length
class, all classes into one occ section, one reduce launch behind them."""
import numpy as np
import pytest
import torch

from tests.score_grad_ref import SENT, TOL, check_grad, fold, i32, logp_normal, ref_gamma, run_grad
from tests.test_gpu_ctc_score_grad import LX1, N1, check_small, small_batch
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MIN = -2 ** 31
bits = lambda a: np.asarray(a).view(np.int32)


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def rows(hyps, W, fill=INT32_MIN):
    lab = torch.full((len(hyps), W), fill, dtype=torch.int32)
    for h, a in enumerate(hyps):
        lab[h, :len(a)] = i32(a)
    return lab.to(DEV), i32([len(h) for h in hyps]).to(DEV)


def run_grad_rows(core, x, lab_d, hl_d, hyp_utt, lx, blank, w=None, max_hyp_len=None, layouts=(False, True)):
    """run_grad (tests/score_grad_ref.py) on device rows: one _C.ctc_score_grad call per layout on a staged ScoreRows, into a grad prefilled
    with NaN and scores prefilled with a sentinel -> (grad [N,T,V] batch-major, scores [H], invalid [H]) as numpy."""
    H = hl_d.numel()
    utt_d = i32(hyp_utt).to(DEV)
    w_d = None if w is None else torch.tensor(np.asarray(w, dtype=np.float32)).to(DEV)
    out = {}
    for tm in layouts:
        xx = x.transpose(0, 1).contiguous() if tm else x
        sr = core.stage_score_rows(xx, lab_d, hl_d, i32(lx), utt_d, blank, tm, max_hyp_len=max_hyp_len, grad=True)
        g0 = torch.full(xx.shape, float("nan"), dtype=torch.float32, device=DEV)
        s0 = torch.full((H,), SENT, dtype=torch.float32, device=DEV)
        g, sc, inv = core.ctc_score_grad(xx, sr, w_d, blank, tm, grad_out=g0, scores_out=s0)
        assert g.data_ptr() == g0.data_ptr() and sc.data_ptr() == s0.data_ptr() and inv.dtype == torch.int32 and inv.shape == (H,)
        g = g.transpose(0, 1) if tm else g
        out[tm] = (g.cpu().numpy(), sc.cpu().numpy(), inv.cpu().numpy())
    g, sc, inv = out[layouts[0]]
    for tm in layouts:
        gg, ss, ii = out[tm]
        assert np.all(np.isfinite(gg)), ("NaN or inf left in grad", tm)
        assert not np.any(ss == SENT) and not np.any(np.isnan(ss)) and np.all((ii == 0) | (ii == 1))
        assert np.array_equal(bits(sc), bits(ss)) and np.array_equal(inv, ii), ("layouts differ", sc, ss)
        e = rel_err(gg, g) if np.abs(g).max() > 0 else float(np.abs(gg).max())
        assert e <= TOL, ("layouts differ", e)
    return g, sc, inv


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. a single class: the small batch of tests/test_gpu_ctc_score_grad.py
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, 5, 2])
def test_single_class(crf, blank):
    c = small_batch(blank)
    x = torch.tensor(c["logp"]).to(DEV)
    lab_d, hl_d = rows(c["hyps"], 15)
    for w, positive, what in ((None, True, "w=1"), (c["w_pos"], True, "w>0"), (c["w_mix"], False, "mixed")):
        g, sc, inv = run_grad_rows(crf._C, x, lab_d, hl_d, c["utt"], LX1, blank, w)
        assert crf._C.last_score_grad_kernel() == "crf_rows_grad_alpha_kernel<1>"
        check_small(c, g, sc, inv, w, positive, f"rows small blank {blank} {what}")
        _, sc_cpu, inv_cpu = run_grad(crf._C, x, c["hyps"], c["utt"], LX1, blank, w, layouts=(False,))
        assert np.array_equal(bits(sc), bits(sc_cpu)) and np.array_equal(inv, inv_cpu)
    # ctc_logp itself: scores and invalid are the CPU-hypotheses call's bits
    utt_d = i32(c["utt"]).to(DEV)
    s_d, i_d = crf.ctc_logp(x.clone().requires_grad_(True), lab_d, hl_d, i32(LX1), utt_d, blank)
    s_c, i_c = crf.ctc_logp(x.clone().requires_grad_(True), lab_d.cpu().clamp(min=0), hl_d.cpu(), i32(LX1), utt_d.cpu(), blank)
    assert s_d.requires_grad and not i_d.requires_grad
    assert torch.equal(s_d.detach().view(torch.int32), s_c.detach().view(torch.int32)) and torch.equal(i_d, i_c)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. mixed classes in one list
# ---------------------------------------------------------------------------------------------------------------------------------
N2, T2, V2 = 2, 420, 6
LX2 = np.array([400, 420], dtype=np.int32)
W_MIX = np.array([1.3, 0.0, -0.6, 0.8])
W_POS = np.array([0.5, 1.2, 0.7, 2.0])
_MIXED = {}


def mixed_batch():
    """Lengths 3, 40, 100 and 200 -- the four wave classes -- in shuffled order, all on utterance 0 (lx = 400 < T); utterance 1 owns
    none.  The fp64 reference is computed once, shared and left unchanged."""
    if not _MIXED:
        blank = 0
        rng = np.random.default_rng(8100)
        hyps = [rng.integers(1, V2, size=n).astype(np.int32) for n in (100, 3, 200, 40)]
        utt = np.zeros(4, dtype=np.int64)
        logp = logp_normal(rng, N2, T2, V2)
        gamma, cost, valid = ref_gamma(logp, hyps, utt, LX2, blank)
        assert np.all(valid == 1) and np.all(np.isfinite(cost))
        for v in (logp, gamma, cost, valid, utt):
            v.setflags(write=False)
        _MIXED.update(logp=logp, hyps=hyps, utt=utt, blank=blank, gamma=gamma, cost=cost, valid=valid)
    return _MIXED


def check_mixed(c, g, sc, inv, w, valid, positive, what):
    check_grad(g, fold(c["gamma"], c["cost"], valid, c["utt"], w, N2), LX2, positive, what)
    assert not np.any(g[0, 400:]) and not np.any(g[1]), "rows t >= lx and an utterance without hypotheses are exactly 0"
    assert np.array_equal(inv, 1 - valid) and np.all(sc[valid == 0] == -np.inf)
    ok = valid == 1
    assert np.all(np.abs(sc[ok] - c["cost"][ok]) <= TOL * np.abs(c["cost"][ok]))


def test_mixed_classes(crf):
    c = mixed_batch()
    x = torch.tensor(c["logp"]).to(DEV)
    lab_d, hl_d = rows(c["hyps"], 200)
    for w, positive in ((W_MIX, False), (W_POS, True)):
        g, sc, inv = run_grad_rows(crf._C, x, lab_d, hl_d, c["utt"], LX2, c["blank"], w)      # the default bound: min(W, 255) = 200
        assert crf._C.last_score_grad_kernel() == "crf_rows_grad_alpha_kernel<8>"
        check_mixed(c, g, sc, inv, w, c["valid"], positive, f"rows mixed classes positive={positive}")
        # every score is the CPU-hypotheses call's on that hypothesis alone: the kernel of its own class
        for h, hyp in enumerate(c["hyps"]):
            s1, i1 = crf._C.ctc_score(x, i32(hyp), i32([len(hyp)]), i32(LX2), i32([0]), c["blank"])
            assert bits(s1.cpu().numpy())[0] == bits(sc)[h] and int(i1.cpu()[0]) == 0, (h, len(hyp))
    # a hypothesis over the bound contributes nothing and is flagged; the others keep their bits
    g7, sc7, inv7 = run_grad_rows(crf._C, x, lab_d, hl_d, c["utt"], LX2, c["blank"], W_POS, max_hyp_len=127)
    assert crf._C.last_score_grad_kernel() == "crf_rows_grad_alpha_kernel<4>"
    valid7 = np.array([1, 1, 0, 1])
    check_mixed(c, g7, sc7, inv7, W_POS, valid7, True, "rows mixed classes, max_hyp_len = 127")
    assert np.array_equal(bits(sc7)[valid7 == 1], bits(sc)[valid7 == 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. raw bf16 output, the bound with a gradient, the three-liner
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fused_bf16_against_the_cpu_hypotheses_call(crf):
    """ctc_logp(fuse_log_softmax=True) + backward on bf16 raw output, device rows against CPU hypotheses: the same kernels on the same
    values up to the order of the reduce stage's LDS adds, held to the bound tests/test_gpu_ctc_score_grad_logits.py holds the fused call
    to against torch's autograd: |delta| <= 2^-8 |ref| + TOL max |ref|."""
    N, T, V, K = 2, 30, 7, 4
    rng = np.random.default_rng(18)
    x = torch.tensor(2.0 * rng.standard_normal((N, T, V))).to(torch.bfloat16).to(DEV)
    lx = i32([30, 22])
    hyps, hl, hu = crf.ctc_sample(x, lx, K, 4321)
    risk = torch.tensor(rng.uniform(0.0, 1.0, size=(N, K)).astype(np.float32)).to(DEV)
    grads, scores = [], []
    for args in ((hyps.cpu(), hl.cpu(), lx, hu.cpu()), (hyps, hl, lx, hu)):
        xb = x.clone().requires_grad_(True)
        s, inv = crf.ctc_logp(xb, *args, fuse_log_softmax=True)
        (torch.softmax(s.view(N, K), -1) * risk).sum().backward()
        assert xb.grad.dtype == torch.bfloat16 and not bool(inv.any())
        grads.append(xb.grad.double().cpu().numpy())
        scores.append(s.detach())
    assert torch.equal(scores[0].view(torch.int32), scores[1].view(torch.int32))
    ref, got = grads
    bound = 2.0 ** -8 * np.abs(ref) + TOL * np.abs(ref).max()
    print(f"[logp_rows] fused bf16: largest |delta| / bound {(np.abs(got - ref) / bound).max():.3f}, max |ref| {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 0 and np.all(np.abs(got - ref) <= bound) and not np.any(got[1, 22:])


def test_bound_above_255_is_refused_only_with_a_gradient(crf):
    x = torch.tensor(logp_normal(np.random.default_rng(9), 1, 40, 5)).to(DEV)
    lab_d, hl_d = rows([np.array([1, 2, 3], dtype=np.int32)], 300)
    args = (lab_d, hl_d, i32([40]), i32([0]).to(DEV))
    with pytest.raises(RuntimeError, match="max_hyp_len=256 exceeds 255"):
        crf.ctc_logp(x.clone().requires_grad_(True), *args, max_hyp_len=256)
    s, inv = crf.ctc_logp(x, *args, max_hyp_len=256)
    assert not s.requires_grad and bool(torch.isfinite(s).all()) and not bool(inv.any())
    s2, _ = crf.ctc_logp(x.clone().requires_grad_(True), *args)                 # the default with a gradient: min(W, 255)
    assert s2.requires_grad and torch.equal(s2.detach().view(torch.int32), s.view(torch.int32))


def test_mwer_three_liner_on_the_device(crf):
    """The docstring's recipe, nothing leaving the device: ctc_sample -> ctc_logp -> a risk-weighted sum -> backward."""
    N, T, V, K = 2, 30, 7, 4
    rng = np.random.default_rng(8)
    logits = torch.tensor((2.0 * rng.standard_normal((N, T, V))).astype(np.float32)).to(DEV).requires_grad_(True)
    log_probs = torch.log_softmax(logits, -1)
    input_lengths = i32([30, 22])
    risk = torch.tensor(rng.uniform(0.0, 1.0, size=(N, K)).astype(np.float32)).to(DEV)
    hyps, hyp_lengths, hyp_utt = crf.ctc_sample(log_probs, input_lengths, K, 1234)
    scores, inv = crf.ctc_logp(log_probs, hyps, hyp_lengths, input_lengths, hyp_utt)
    (torch.softmax(scores.view(N, K), -1) * risk.view(N, K)).sum().backward()
    g = logits.grad
    assert not bool(inv.any()) and bool(torch.isfinite(scores).all())
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and not bool(g[1, 22:].any())
