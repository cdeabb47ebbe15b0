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


# ---------------------------------------------------------------------------------------------------------------------------------
# Log-probs whose cost per frame is UNEVEN: the frames are cut into len(phases) equal runs, each drawn from one phase kind around a
# planted path, so that the forward vector leaves the straight ramp (t + 1) * score / lx by thousands of nats.
# ---------------------------------------------------------------------------------------------------------------------------------
def peaked(k):
    """N(0, 1) plus k on the planted path's class: the hypothesis costs about 0 per frame."""
    return ("peaked", float(k))


def wrong(k):
    """N(0, 1) plus k on class (path[t] + 1) % V: the hypothesis pays about k per frame."""
    return ("wrong", float(k))


def flat_phase(sigma):
    """N(0, sigma): nothing is favoured, the hypothesis pays about log V per frame."""
    return ("flat", float(sigma))


def planted_path(hyp, T, blank):
    """path[t] = ext[min(t * S // T, S - 1)], ext the hypothesis interleaved with blanks, S = 2 L + 1: the states at an even pace."""
    S = 2 * len(hyp) + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = np.asarray(hyp, dtype=np.int64)
    return ext[np.minimum(np.arange(T) * S // T, S - 1)]


def phase_starts(T, n):
    """First frame of each of n equal runs of T frames, and T."""
    return [i * T // n for i in range(n + 1)]


def logp_phases(rng, hyp, T, V, blank, phases):
    """[T,V] fp32 log-probs: run i of the frames (phase_starts) from phases[i] -- peaked(k), wrong(k) or flat_phase(sigma) -- around
    planted_path(hyp), then log_softmax in fp64 and one cast to fp32.  Two phases: a cheap half and a costly one; three (right / wrong /
    right): the distance of the forward vector to the ramp changes sign."""
    path = planted_path(hyp, T, blank)
    raw = np.empty((T, V), dtype=np.float64)
    cut = phase_starts(T, len(phases))
    for (kind, a), t0, t1 in zip(phases, cut[:-1], cut[1:]):
        t = np.arange(t0, t1)
        if kind == "flat":
            raw[t0:t1] = rng.normal(0.0, a, size=(t1 - t0, V))
            continue
        raw[t0:t1] = rng.normal(0.0, 1.0, size=(t1 - t0, V))
        raw[t, path[t0:t1] if kind == "peaked" else (path[t0:t1] + 1) % V] += a
    m = raw.max(-1, keepdims=True)
    return (raw - m - np.log(np.exp(raw - m).sum(-1, keepdims=True))).astype(np.float32)


# The uneven calls of tests/test_gpu_ctc_score_grad_uneven.py (and of tests/test_score_grad_uneven_inputs.py, which holds their inputs to
# the regime they are meant for): name -> (V, L, phases of utterance 0, NR of the instantiation).  T = 1500, blank 0.
UNEVEN_T, UNEVEN_LX1 = 1500, 700
UNEVEN_CASES = {
    "right_wrong_L20": (8, 20, (peaked(20), wrong(20)), 1),
    "wrong_right_L20": (8, 20, (wrong(20), peaked(20)), 1),
    "right_wrong_right_L100": (8, 100, (peaked(20), wrong(50), peaked(20)), 4),   # (k = 50: at 20 this hypothesis finds a path at 9 nats a frame)
    "right_wrong_L255": (8, 255, (peaked(20), wrong(20)), 8),
    "confident_flat_V4096_L40": (4096, 40, (peaked(20), flat_phase(0.1)), 2),
}
_UNEVEN = {}


def uneven_case(name):
    """One call: utterance 0 (lx = T = 1500) holds the case's hypothesis on its phases; utterance 1 (lx = 700, the same phases over its
    700 frames, N(0, 2) behind them) holds a hypothesis of min(L, 12) labels and the empty one.  Weights positive, and of mixed sign.
    The fp64 reference is computed once per case, shared and left unchanged."""
    if name not in _UNEVEN:
        V, L, phases, nr = UNEVEN_CASES[name]
        T, blank = UNEVEN_T, 0
        rng = np.random.default_rng(sum(map(ord, name)))
        pool = np.arange(1, V if V <= 8 else 64)
        hyps = [pool[rng.integers(0, len(pool), size=L)].astype(np.int32), pool[rng.integers(0, len(pool), size=min(L, 12))].astype(np.int32),
                np.zeros(0, dtype=np.int32)]
        utt, lx = np.array([0, 1, 1]), np.array([T, UNEVEN_LX1], dtype=np.int32)
        logp = logp_normal(rng, 2, T, V)
        logp[0] = logp_phases(rng, hyps[0], T, V, blank, phases)
        logp[1, :UNEVEN_LX1] = logp_phases(rng, hyps[1], UNEVEN_LX1, V, blank, phases)
        gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
        w_pos = rng.uniform(0.25, 2.0, size=3)
        w_mix = np.array([1.0, -0.7, 0.4]) * rng.uniform(0.5, 1.5, size=3)
        for v in (logp, gamma, cost, valid, utt, lx, w_pos, w_mix):
            v.setflags(write=False)
        _UNEVEN[name] = dict(logp=logp, hyps=hyps, utt=utt, lx=lx, blank=blank, gamma=gamma, cost=cost, valid=valid, w_pos=w_pos, w_mix=w_mix,
                             nr=nr, change=phase_starts(T, len(phases))[1:-1])
    return _UNEVEN[name]


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
