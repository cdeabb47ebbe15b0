"""What the tests of crf_ctc_score_grad / ctc_crf.ctc_logp share (a plain helper module): the fp64 reference -- tests.util.oracle_blank's gamma
on the activations REPEATED per hypothesis on the host, weighted and summed per utterance in fp64, valid hypotheses of finite cost only --
the driver of one call in both layouts on prefilled outputs, and the checks.

Tolerances are the project's own: TOL = 1e-4 (tests/test_gpu_ctc_variants.py), entry by entry on the posteriors >= 1e-3 for non-negative
weights (tests.util.post_err), against the largest entry and norm-wise for weights of mixed sign (tests.util.rel_err)."""
import numpy as np
import torch

from tests.util import log_softmax_np, oracle_blank, post_err, rel_err

TOL = 1e-4
SENT = 12345.0


def i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int64).reshape(-1), dtype=torch.int32)


def flat(hyps):
    return np.concatenate([np.asarray(h, dtype=np.int32) for h in hyps] + [np.zeros(0, dtype=np.int32)])


def logp_normal(rng, N, T, V):
    return log_softmax_np(rng.normal(0.0, 2.0, size=(N, T, V))).astype(np.float32)


def ref_gamma(logp, hyps, hyp_utt, lx, blank):
    """(gamma [H,T,V], +log p [H] fp64, valid [H]) of the fp64 oracle on the rows of each hypothesis's utterance."""
    hyp_utt = np.asarray(hyp_utt)
    rep = np.ascontiguousarray(np.asarray(logp)[hyp_utt])
    ly = np.array([len(h) for h in hyps], dtype=np.int32)
    return oracle_blank(rep, flat(hyps), np.asarray(lx, dtype=np.int32)[hyp_utt], ly, blank)


def fold(gamma, cost, valid, hyp_utt, w, N):
    """sum over the valid hypotheses of finite cost of w[h] * gamma[h], per utterance, fp64 -> [N,T,V]."""
    out = np.zeros((N,) + gamma.shape[1:], dtype=np.float64)
    w = np.ones(len(cost)) if w is None else np.asarray(w, dtype=np.float64)
    for h, u in enumerate(np.asarray(hyp_utt)):
        if valid[h] and np.isfinite(cost[h]):
            out[u] += w[h] * gamma[h].astype(np.float64)
    return out


def run_grad(core, x, hyps, hyp_utt, lx, blank, w=None, layouts=(False, True)):
    """x: [N,T,V] CUDA tensor, batch-major.  One _C.ctc_score_grad call per layout into a grad prefilled with NaN and scores prefilled with
    a sentinel -> (grad [N,T,V] batch-major, scores [H], invalid [H]) as numpy, after checking that nothing prefilled is left, that the
    scores of the layouts are the same bits and that the gradients agree to TOL."""
    H = len(hyps)
    meta = (i32(flat(hyps)), i32([len(h) for h in hyps]), i32(lx), i32(hyp_utt))
    w_d = None if w is None else torch.tensor(np.asarray(w, dtype=np.float32)).to(x.device)
    out = {}
    for tm in layouts:
        xx = x.transpose(0, 1).contiguous() if tm else x
        g0 = torch.full(xx.shape, float("nan"), dtype=torch.float32, device=x.device)
        s0 = torch.full((H,), SENT, dtype=torch.float32, device=x.device)
        g, sc, inv = core.ctc_score_grad(xx, meta, w_d, blank, tm, grad_out=g0, scores_out=s0)
        assert g.data_ptr() == g0.data_ptr() and sc.data_ptr() == s0.data_ptr() and inv.dtype == torch.int32 and inv.shape == (H,)
        g = g.transpose(0, 1) if tm else g
        out[tm] = (g.cpu().numpy(), sc.cpu().numpy(), inv.cpu().numpy())
        assert torch.equal(xx, x.transpose(0, 1).contiguous() if tm else x), "the call wrote to its input"
    g, sc, inv = out[layouts[0]]
    for tm in layouts:
        gg, ss, ii = out[tm]
        assert not np.any(np.isnan(gg)) and np.all(np.isfinite(gg)), ("NaN or inf left in grad", tm)
        assert not np.any(ss == SENT) and not np.any(np.isnan(ss)) and np.all((ii == 0) | (ii == 1))
        assert np.array_equal(sc.view(np.int32), ss.view(np.int32)) and np.array_equal(inv, ii), ("layouts differ", sc, ss)
        e = rel_err(gg, g) if np.abs(g).max() > 0 else float(np.abs(gg).max())
        assert e <= TOL, ("layouts differ", e)
    return g, sc, inv


def check_grad(g, ref, lx, positive, what=""):
    """g against the reference: the project's metric for the sign of the weights; frames at or past lx exactly 0."""
    for u, n in enumerate(np.asarray(lx)):
        assert not np.any(g[u, max(int(n), 0):]), (what, "frames past lx", u)
    pe = post_err(g, ref) if positive else None
    re = rel_err(g, ref) if np.abs(ref).max() > 0 else float(np.abs(g).max())
    print(f"[score_grad] {what}: post_err {pe} rel_err {re:.3e}")
    if positive:
        assert pe <= TOL, (what, "post_err", pe)
    assert re <= TOL, (what, "rel_err", re)
