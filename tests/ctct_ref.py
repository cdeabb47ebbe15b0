"""The yardstick of the CTC-Transducer loss tests (a plain helper module): there is no other implementation of this loss to compare
against, so three independent ones are written here and held to each other by tests/test_ctct_api.py.

  (a) `lattice` / `ref_normalised` / `ref_logits`: the forward / backward recursion in numpy fp64 with the closed-form gradients, for
      normalised log-probabilities and for raw joiner output (log_softmax's backward folded in), one numpy operation per frame, so that
      1 024 columns stay fast;
  (b) `torch_cost`: the forward recursion in torch fp64 behind log_softmax, node by node, differentiated by autograd;
  (c) `brute_force`: every one of the V^T frame labellings (T <= 6, V <= 4), scored from row u = labels emitted so far and kept if its
      CTC collapse is y.

One utterance at a time: x is [T, U + 1, V], labels [U], none equal to the blank.  A path labels every frame with one class; blanks and
repeats collapse; frame t is read from row u = the number of labels emitted before it.  Per column two masses after t frames, Ab (ends in
a blank or in nothing) and An (ends in y_u):

    Ab[0][0] = 0;  Ab[t+1][u] = lse(Ab, An)[t][u] + b(t,u)
    An[t+1][u] = lse(An[t][u] + r(t,u), Ab[t][u-1] + e(t,u-1), An[t][u-1] + e(t,u-1) only if y_u != y_{u-1})
    cost = -lse(Ab[T][U], An[T][U])

A lattice without a finite path (T < U + repeats, or -inf entries) costs +inf and has a zero gradient."""
import itertools

import numpy as np
import torch

from tests.rnnt_ref import log_softmax

NINF = -np.inf


def _split(lp, labels, blank):
    """lp [T, U+1, V] -> b, r, e [T, U+1] (r[:, 0] = e[:, U] = -inf), skip [U+1] (y_{u+1} may follow y_u directly), labels int64 [U]."""
    T, U1, _ = lp.shape
    U = U1 - 1
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    assert labels.size == U
    b = lp[:, :, blank]
    r, e = np.full((T, U1), NINF), np.full((T, U1), NINF)
    if U:
        rows = np.arange(T)[:, None]
        r[:, 1:] = lp[:, 1:, :][rows, np.arange(U)[None, :], labels[None, :]]
        e[:, :U] = lp[:, :U, :][rows, np.arange(U)[None, :], labels[None, :]]
    skip = np.ones(U1, dtype=bool)
    if U >= 2:
        skip[1:U] = labels[1:] != labels[:-1]
    return b, r, e, skip, labels


def lattice(b, r, e, skip):
    """-> (cost, d cost / d b, d cost / d r, d cost / d e), each [T, U+1]."""
    T, U1 = b.shape
    U = U1 - 1
    Ab, An = np.full((T + 1, U1), NINF), np.full((T + 1, U1), NINF)
    Bb, Bn = np.full((T + 1, U1), NINF), np.full((T + 1, U1), NINF)
    S, X = np.full((T, U1), NINF), np.full((T, U1), NINF)
    Ab[0, 0] = 0.0
    Bb[T, U] = Bn[T, U] = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            S[t] = np.logaddexp(Ab[t], An[t])
            X[t] = np.where(skip, S[t], Ab[t])
            move = np.concatenate(([NINF], (X[t] + e[t])[:-1]))
            Ab[t + 1] = S[t] + b[t]
            An[t + 1] = np.logaddexp(An[t] + r[t], move)
        total = np.logaddexp(Ab[T, U], An[T, U])
        zero = np.zeros((T, U1))
        if not np.isfinite(total):
            return np.inf, zero, zero.copy(), zero.copy()
        up = np.full((T, U1), NINF)                   # Bn[t+1][u+1]
        for t in range(T - 1, -1, -1):
            up[t, :U] = Bn[t + 1, 1:]
            x = e[t] + up[t]
            c = b[t] + Bb[t + 1]
            Bb[t] = np.logaddexp(c, x)
            Bn[t] = np.logaddexp(np.logaddexp(c, r[t] + Bn[t + 1]), np.where(skip, x, NINF))

        def occ(v):
            return -np.exp(np.where(np.isnan(v), NINF, v))
        g_b = occ(S + b + Bb[1:] - total)
        g_r = occ(An[:T] + r + Bn[1:] - total)
        g_e = occ(X + e + up - total)
    return -total, g_b, g_r, g_e


def ref_normalised(log_probs, labels, blank=0):
    """log_probs [T, U+1, V] (any real numbers: nothing normalises them).  -> (cost, d cost / d log_probs)."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, U1, _ = lp.shape
    b, r, e, skip, labels = _split(lp, labels, blank)
    cost, g_b, g_r, g_e = lattice(b, r, e, skip)
    g = np.zeros_like(lp)
    g[:, :, blank] = g_b
    rows = np.arange(T)
    for u in range(U1 - 1):
        g[rows, u + 1, labels[u]] += g_r[:, u + 1]
        g[rows, u, labels[u]] += g_e[:, u]
    return cost, g


def ref_logits(x, labels, blank=0):
    """x [T, U+1, V] raw joiner output.  -> (cost of log_softmax(x), d cost / d x = g - softmax(x) * sum_v g)."""
    x = np.asarray(x, dtype=np.float64)
    lp = log_softmax(x)
    cost, g = ref_normalised(lp, labels, blank)
    with np.errstate(invalid="ignore"):
        sm = np.exp(lp)
    sm = np.where(np.isnan(sm), 0.0, sm)
    return cost, g - sm * g.sum(-1, keepdims=True)


def torch_cost(x, labels, blank=0, normalise=True):
    """(b): the cost as a torch fp64 scalar with autograd history back to x (a leaf made here), node by node; a dead term is left out of
    its sum (logsumexp of -inf's has a NaN gradient).  -> (cost, x); cost is +inf without history when there is no path."""
    x = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    lp = torch.log_softmax(x, -1) if normalise else x
    T, U1, _ = lp.shape
    U = U1 - 1
    y = [int(v) for v in np.asarray(labels).reshape(-1)]

    def lse(terms):
        terms = [v for v in terms if v is not None and bool(torch.isfinite(v))]
        if not terms:
            return None
        return torch.logsumexp(torch.stack(terms), 0) if len(terms) > 1 else terms[0]

    def plus(a, v):
        return None if a is None else a + v

    Ab = [torch.zeros((), dtype=torch.float64)] + [None] * U
    An = [None] * U1
    for t in range(T):
        nb, nn = [None] * U1, [None] * U1
        for u in range(U1):
            nb[u] = plus(lse([Ab[u], An[u]]), lp[t, u, blank])
            terms = []
            if u >= 1:
                terms.append(plus(An[u], lp[t, u, y[u - 1]]))
                terms.append(plus(Ab[u - 1], lp[t, u - 1, y[u - 1]]))
                if u == 1 or y[u - 1] != y[u - 2]:
                    terms.append(plus(An[u - 1], lp[t, u - 1, y[u - 1]]))
            nn[u] = lse(terms)
        Ab, An = nb, nn
    total = lse([Ab[U], An[U]])
    return (torch.tensor(float("inf"), dtype=torch.float64) if total is None else -total), x


def collapse(path, blank):
    out, prev = [], blank
    for c in path:
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return out


def brute_force(log_probs, labels, blank=0):
    """(c): -log of the sum over every frame labelling whose CTC collapse is y of its probability, frame t read from row u = the number of
    labels the labelling has emitted before t; T <= 6, V <= 4."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, U1, V = lp.shape
    y = [int(v) for v in np.asarray(labels).reshape(-1)]
    assert T <= 6 and V <= 4 and len(y) == U1 - 1
    paths = []
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) != y:
            continue
        s, u, prev = 0.0, 0, blank
        for t, c in enumerate(path):
            s += lp[t, u, c]
            if c != blank and c != prev:
                u += 1
            prev = c
        paths.append(s)
    if not paths:
        return np.inf
    paths = np.asarray(paths)
    m = paths.max()
    return np.inf if not np.isfinite(m) else -(m + np.log(np.sum(np.exp(paths - m))))


# ---- batches, as the GPU tests need them ----
def repeats(labels):
    labels = np.asarray(labels).reshape(-1)
    return int(np.sum(labels[1:] == labels[:-1])) if labels.size > 1 else 0


def draw_labels(rng, U, V, blank, budget):
    """U labels without the blank with at most `budget` adjacent equal pairs -- and at least one where U >= 2 and budget >= 1."""
    classes = [v for v in range(V) if v != blank]
    lab = [classes[int(k)] for k in rng.integers(0, len(classes), U)]
    assert len(classes) > 1 or max(U - 1, 0) <= budget, "a single class repeats everywhere"
    while repeats(lab) > budget:
        i = next(i for i in range(1, U) if lab[i] == lab[i - 1])
        free = [v for v in classes if v != lab[i - 1] and (i + 1 >= U or v != lab[i + 1])] or [v for v in classes if v != lab[i - 1]]
        lab[i] = free[int(rng.integers(0, len(free)))]
    if U >= 2 and budget >= 1 and repeats(lab) == 0:
        lab[U - 1] = lab[U - 2]
    return lab


def random_case(seed, T_n, U_n, V, blank=0, T=None, U1=None, scale=3.0, feasible=True):
    """Padded raw joiner output [N, T, U1, V] fp32 and labels [N, U1 - 1] int32 without the blank, drawn so that T_n >= U_n + repeats
    (feasible) and that adjacent equal labels occur wherever the lengths allow them; lx, ly as int lists."""
    rng = np.random.default_rng(seed)
    N = len(T_n)
    T = T or max(T_n)
    U1 = U1 or max(U_n) + 1
    x = (rng.standard_normal((N, T, U1, V)) * scale).astype(np.float32)
    labels = np.zeros((N, U1 - 1), dtype=np.int32)
    for n in range(N):
        budget = T_n[n] - U_n[n] if feasible else U1
        labels[n, :U_n[n]] = draw_labels(rng, U_n[n], V, blank, max(budget, 0) if V > 2 else U1)
        labels[n, U_n[n]:] = draw_labels(rng, U1 - 1 - U_n[n], V, blank, U1)
    return x, labels, [int(t) for t in T_n], [int(u) for u in U_n]


def batch_ref(x, labels, lx, ly, blank, fused):
    """(a) per utterance on a padded batch (x fp64-able [N, T, U1, V]) -> (costs [N], grad like x, zeros over the padding)."""
    x = np.asarray(x, dtype=np.float64)
    costs, grad = np.zeros(len(lx)), np.zeros_like(x)
    for n, (t, u) in enumerate(zip(lx, ly)):
        c, g = (ref_logits if fused else ref_normalised)(x[n, :t, :u + 1], labels[n, :u], blank)
        costs[n] = c
        grad[n, :t, :u + 1] = g
    return costs, grad
