"""What the tests of crf_ctc_score_grad_logits / ctc_crf.ctc_logp(fuse_log_softmax=True) share (a plain helper module): the parity cases, the
fp64 reference, the driver of one call in both layouts on prefilled outputs, and the checks.

Reference.  The input is RAW network output x in fp32 / bf16 / fp16; x^ is its exact fp32 upcast, so a quantised input costs no tolerance.
    grad[u][t][v] = sum over the live h of u of w_h * gamma_h[t][v]  -  W_u * softmax64(x^[u][t])[v],     W_u = sum of the live w_h,
gamma_h the occupancies of log_softmax(x^) by tests/score_grad_ref.py's fp64 oracle.  The oracle takes its activations in fp32, so
log_softmax computed in fp64 would be rounded on its way in; the occupancies do not depend on a constant added to a frame (every
alignment takes one entry of each frame), so the oracle runs on x^ ITSELF -- exact in fp32 -- and its gamma is that of log_softmax64(x^)
without that rounding.  Its cost is then the raw sum-product: score = cost - sum_{t < lx} lse64_t.
Tolerance: TOL = 1e-4, the project's (tests/score_grad_ref.py), by tests.util.rel_err -- against the largest entry and norm-wise."""
import numpy as np
import torch

from ctc_crf import _C as core
from tests.score_grad_ref import SENT, TOL, flat, fold, i32, ref_gamma, uneven_case
from tests.util import rel_err

_FEATURE = (core._lib.crf_ctc_score_grad_logits, core._lib.crf_ctc_score_grad_logits_workspace_bytes)   # (an AttributeError without the feature)

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KERNEL_DTYPE = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}
KERNEL_OF_L = {31: 1, 32: 2, 64: 4, 128: 8, 255: 8}                     # NR of the instantiation, from the call's longest hypothesis


def kernel_name(nr, dtype):
    return f"crf_ctc_score_grad_alpha_raw_kernel<{nr}, {KERNEL_DTYPE[dtype]}>"


def quantise(raw, dtype):
    """raw (fp64 numpy) -> (the CPU tensor of that dtype the call reads, its exact fp32 upcast as numpy)."""
    t = torch.tensor(np.asarray(raw, dtype=np.float64)).to(DTYPES[dtype])
    return t, t.float().numpy()


def raw_ref(x32, hyps, utt, lx, blank):
    """dict(gamma [H,T,V], cost [H] = +log p under log_softmax64(x^), valid [H], soft [N,T,V] = softmax64(x^), live [H])."""
    utt, lx = np.asarray(utt), np.asarray(lx, dtype=np.int32)
    gamma, raw_cost, valid = ref_gamma(x32, hyps, utt, lx, blank)
    x64 = np.asarray(x32, dtype=np.float64)
    m = x64.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(x64 - m).sum(-1))
    soft = np.exp(x64 - lse[..., None])
    cost = np.array([raw_cost[h] - lse[u, :max(int(lx[u]), 0)].sum() if np.isfinite(raw_cost[h]) else raw_cost[h] for h, u in enumerate(utt)])
    live = (valid == 1) & np.isfinite(cost)
    return dict(gamma=gamma, cost=cost, valid=valid, soft=soft, live=live)


def live_weight(r, utt, w, N, absolute=False):
    """[N]: the sum of the (absolute) weights of each utterance's live hypotheses, fp64."""
    w = np.ones(len(r["cost"])) if w is None else np.asarray(w, dtype=np.float64)
    out = np.zeros(N)
    for h, u in enumerate(np.asarray(utt)):
        if r["live"][h]:
            out[u] += abs(w[h]) if absolute else w[h]
    return out


def fold_raw(r, utt, w, lx):
    """The reference gradient [N,T,V] in fp64: the folded occupancies minus W_u softmax64 on the frames below lx."""
    N, T = r["soft"].shape[:2]
    below = (np.arange(T)[None, :] < np.asarray(lx)[:, None])[..., None]
    return fold(r["gamma"], r["cost"], r["valid"], utt, w, N) - live_weight(r, utt, w, N)[:, None, None] * r["soft"] * below


# ---------------------------------------------------------------------------------------------------------------------------------
# The parity cases of tests/test_gpu_ctc_score_grad_logits.py (and of tests/test_score_grad_logits_inputs.py, which holds their
# references to the regime the tolerance is meant for).  Each: dict(x: the CPU tensor the call reads [N,T,V], x32, hyps, utt, lx, blank,
# weights {name: [H] or None}, ref: raw_ref(...), dtype, nr), computed once, shared and left unchanged.
# ---------------------------------------------------------------------------------------------------------------------------------
N1, T1, V1 = 3, 48, 6
LX1 = np.array([48, 31, 9], dtype=np.int32)
FRAME_LX = (1, 2, 15, 16, 17, 33)
_CASES = {}


def _small(dtype, blank):
    """The small_batch shape of tests/test_gpu_ctc_score_grad.py (its hypotheses and weights: N = 3, ragged lx, an utterance with no
    hypothesis, two invalid hypotheses) on raw N(0, 2)."""
    from tests.test_gpu_ctc_score_grad import small_batch
    c = small_batch(blank)
    rng = np.random.default_rng(8100 + blank)
    x, x32 = quantise(rng.normal(0.0, 2.0, size=(N1, T1, V1)), dtype)
    return dict(x=x, x32=x32, hyps=c["hyps"], utt=c["utt"], lx=LX1, blank=blank, weights=dict(none=None, pos=c["w_pos"], mix=c["w_mix"]), nr=1)


def _one_instantiation(dtype, L):
    V, blank = 8, 0
    rng = np.random.default_rng(900 + L)
    pool = np.arange(1, V)
    rep = np.repeat(pool[rng.integers(0, len(pool), size=(L + 2) // 3)], 3)[:L].astype(np.int32)    # runs of three: many repeats
    hyps = [pool[rng.integers(0, len(pool), size=L)].astype(np.int32), rep, pool[rng.integers(0, len(pool), size=L // 2)].astype(np.int32)]
    reps = [int(np.sum(h[1:] == h[:-1])) for h in hyps]
    T = max(len(h) + r for h, r in zip(hyps, reps)) + 5
    x, x32 = quantise(rng.normal(0.0, 2.0, size=(2, T, V)), dtype)
    return dict(x=x, x32=x32, hyps=hyps, utt=np.array([0, 1, 1]), lx=np.array([T, T - 2], dtype=np.int32), blank=blank,
                weights=dict(pos=rng.uniform(0.25, 2.0, size=3)), nr=KERNEL_OF_L[L])


def _odd_v(dtype):
    """V = 7: rows of 16-bit elements start on 2-byte boundaries; the prefetch batches and the clamp to lx - 1; L = 0, 1 and L = lx exactly."""
    T, V, blank = 40, 7, 1
    rng = np.random.default_rng(77)
    pool = np.array([v for v in range(V) if v != blank])
    hyps, utt = [], []
    for u, n in enumerate(FRAME_LX):
        full = pool[(np.arange(n) + u) % len(pool)].astype(np.int32)        # L = lx, no repeats: ONE alignment
        for h in (full[:0], full[:1], full):
            hyps.append(h)
            utt.append(u)
    x, x32 = quantise(rng.normal(0.0, 2.0, size=(len(FRAME_LX), T, V)), dtype)
    return dict(x=x, x32=x32, hyps=hyps, utt=np.array(utt), lx=np.array(FRAME_LX, dtype=np.int32), blank=blank,
                weights=dict(pos=rng.uniform(0.25, 2.0, size=len(hyps))), nr=2)


def _shifted():
    """The fp32 log-probs of uneven_case("right_wrong_L20") (T = 1500, the cost per frame uneven) plus a constant per frame from N(0, 5):
    lse_t is far from 0.  The reference is computed from the shifted fp32 input itself."""
    c = uneven_case("right_wrong_L20")
    rng = np.random.default_rng(1500)
    x, x32 = quantise(c["logp"].astype(np.float64) + rng.normal(0.0, 5.0, size=c["logp"].shape[:2] + (1,)), "fp32")
    return dict(x=x, x32=x32, hyps=c["hyps"], utt=c["utt"], lx=c["lx"], blank=c["blank"], weights=dict(pos=c["w_pos"], mix=c["w_mix"]), nr=1)


DEAD = 3


def _dead(dtype):
    """A class column of -inf (every row keeps finite entries): the hypotheses that need it score -inf and are not live."""
    N, T, V, blank = 2, 24, 6, 0
    rng = np.random.default_rng(56)
    raw = rng.normal(0.0, 2.0, size=(N, T, V))
    raw[:, :, DEAD] = -np.inf
    x, x32 = quantise(raw, dtype)
    hyps = [np.array(a, dtype=np.int32) for a in ([1, 2, 4], [1, 3, 2], [], [3], [5, 5, 1], [2, 3, 3, 4])]
    return dict(x=x, x32=x32, hyps=hyps, utt=np.array([0, 0, 1, 1, 1, 0]), lx=np.array([24, 17], dtype=np.int32), blank=blank,
                weights=dict(pos=rng.uniform(0.25, 2.0, size=len(hyps))), nr=1)


PARITY_CASES = {}
for _d in DTYPES:
    for _b in (0, V1 - 1, 2):
        PARITY_CASES[f"small_{_d}_blank{_b}"] = (_small, (_d, _b))
for _d in ("bf16", "fp16"):
    for _L in sorted(KERNEL_OF_L):
        PARITY_CASES[f"L{_L}_{_d}"] = (_one_instantiation, (_d, _L))
    PARITY_CASES[f"odd_v_{_d}"] = (_odd_v, (_d,))
PARITY_CASES["shifted_fp32"] = (_shifted, ())
for _d in ("fp32", "bf16"):
    PARITY_CASES[f"dead_{_d}"] = (_dead, (_d,))


def parity_case(name):
    if name not in _CASES:
        f, a = PARITY_CASES[name]
        c = f(*a)
        c["dtype"] = a[0] if a else "fp32"
        c["ref"] = raw_ref(c["x32"], c["hyps"], c["utt"], c["lx"], c["blank"])
        for v in [c["x32"]] + list(c["ref"].values()):
            v.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# driver and checks (GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_grad_raw(x, hyps, hyp_utt, lx, blank, w=None, layouts=(False, True)):
    """x: [N,T,V] CUDA tensor of raw output, batch-major.  One _C.ctc_score_grad(fused=True) call per layout into a grad prefilled with NaN
    and scores prefilled with a sentinel -> (grad [N,T,V] batch-major, scores [H], invalid [H]) as numpy, after checking that nothing
    prefilled is left, that scores and invalid are _C.ctc_score(fused=True)'s bits in that layout, that the scores of the layouts are the
    same bits and that the gradients agree to TOL."""
    H = len(hyps)
    meta = (i32(flat(hyps)), i32([len(h) for h in hyps]), i32(lx), i32(hyp_utt))
    w_d = None if w is None else torch.tensor(np.asarray(w, dtype=np.float32)).to(x.device)
    out = {}
    for tm in layouts:
        xx = x.transpose(0, 1).contiguous() if tm else x
        keep = xx.clone()
        g0 = torch.full(xx.shape, float("nan"), dtype=torch.float32, device=x.device)
        s0 = torch.full((H,), SENT, dtype=torch.float32, device=x.device)
        g, sc, inv = core.ctc_score_grad(xx, meta, w_d, blank, tm, grad_out=g0, scores_out=s0, fused=True)
        assert g.data_ptr() == g0.data_ptr() and sc.data_ptr() == s0.data_ptr() and inv.dtype == torch.int32 and inv.shape == (H,)
        assert torch.equal(xx.view(torch.uint8), keep.view(torch.uint8)), "the call wrote to its input"
        s2, i2 = core.ctc_score(xx, *meta, blank, tm, True)
        assert torch.equal(sc.view(torch.int32), s2.view(torch.int32)) and torch.equal(inv, i2), ("not ctc_score(fused=True)'s bits", tm, sc, s2)
        g = g.transpose(0, 1) if tm else g
        out[tm] = (g.cpu().numpy(), sc.cpu().numpy(), inv.cpu().numpy())
    g, sc, inv = out[layouts[0]]
    for tm in layouts:
        gg, ss, ii = out[tm]
        assert not np.any(np.isnan(gg)) and np.all(np.isfinite(gg)), ("NaN or inf left in grad", tm)
        assert not np.any(ss == SENT) and not np.any(np.isnan(ss)) and np.all((ii == 0) | (ii == 1))
        assert np.array_equal(sc.view(np.int32), ss.view(np.int32)) and np.array_equal(inv, ii), ("layouts differ", sc, ss)
        e = rel_err(gg, g) if np.abs(g).max() > 0 else float(np.abs(gg).max())
        assert e <= TOL, ("layouts differ", e)
    return g, sc, inv


def check_raw(c, g, sc, inv, w, what=""):
    """g, sc, inv of case c under weights w against the reference: rel_err <= TOL; frames at or past lx and utterances without a live
    hypothesis exactly 0; every other row sums to 0 within TOL * sum |w| (the occupancies and the softmax both sum to 1); the scores to
    TOL |score|, -inf and invalid where the reference has them."""
    r, utt, lx = c["ref"], np.asarray(c["utt"]), np.asarray(c["lx"])
    N = g.shape[0]
    ref = fold_raw(r, utt, w, lx)
    wabs = live_weight(r, utt, w, N, absolute=True)
    nlive = np.bincount(utt[r["live"]], minlength=N)
    for u in range(N):
        assert not np.any(g[u, max(int(lx[u]), 0):]), (what, "frames past lx", u)
        if nlive[u] == 0:
            assert not np.any(g[u]), (what, "an utterance without a live hypothesis has a zero gradient", u)
        else:
            rows = np.abs(g[u, :int(lx[u])].astype(np.float64).sum(-1))
            print(f"[score_grad_logits] {what}: utterance {u} largest |row sum| {rows.max():.3e} of {TOL * wabs[u]:.3e}")
            assert np.all(rows <= TOL * wabs[u]), (what, "row sums", u, float(rows.max()))
    re = rel_err(g, ref) if np.abs(ref).max() > 0 else float(np.abs(g).max())
    print(f"[score_grad_logits] {what}: rel_err {re:.3e}")
    assert re <= TOL, (what, "rel_err", re)
    assert np.array_equal(inv, 1 - r["valid"]), (what, inv, r["valid"])
    assert np.all(sc[~r["live"]] == -np.inf)
    ok = r["live"]
    assert np.all(np.abs(sc[ok] - r["cost"][ok]) <= TOL * np.abs(r["cost"][ok])), (what, sc, r["cost"])
    return ref
