"""The yardstick of the RNN-T loss tests (a plain helper module): there is no other implementation of this loss to compare against, so
three independent ones are written here and held to each other by tests/test_rnnt_api.py.

  (a) `lattice` / `ref_normalised` / `ref_logits`: the forward / backward recursion in numpy fp64 with the closed-form gradients, for
      normalised log-probabilities and for raw joiner output (log_softmax's backward folded in); `lattice_diag` is the same recursion a
      whole anti-diagonal at a time, for the lattices of a million nodes that `lattice` would take a minute for;
  (b) `torch_cost`: the forward recursion in torch fp64 behind log_softmax, differentiated by autograd;
  (c) `brute_force`: every alignment enumerated (T <= 4, U <= 3).

One utterance at a time: x is [T, U + 1, V], labels [U].  Blank moves t -> t + 1, label y[u] moves u -> u + 1, the path ends with a blank
at (T - 1, U).  A lattice without a finite path costs +inf and has a zero gradient."""
import itertools

import numpy as np
import torch


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x, axis=-1, keepdims=True)
    dead = ~np.isfinite(m)                            # a row of -inf has no normaliser: every entry stays -inf (the kernels' rule)
    m = np.where(dead, 0.0, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dead, -np.inf, x - m - np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True)))


def lattice(lb, ll):
    """lb [T, U+1]: log-prob of the blank at every node; ll [T, U]: of label y[u] at node (t, u).  -> (cost, d cost / d lb, d cost / d ll)."""
    lb, ll = np.asarray(lb, dtype=np.float64), np.asarray(ll, dtype=np.float64)
    T, U1 = lb.shape
    U = U1 - 1
    alpha = np.full((T, U1), -np.inf)
    beta = np.full((T + 1, U1 + 1), -np.inf)          # beta[T][U] = 0: behind the final blank
    alpha[0, 0] = 0.0
    for t in range(T):
        for u in range(U1):
            if t > 0:
                alpha[t, u] = np.logaddexp(alpha[t, u], alpha[t - 1, u] + lb[t - 1, u])
            if u > 0:
                alpha[t, u] = np.logaddexp(alpha[t, u], alpha[t, u - 1] + ll[t, u - 1])
    beta[T, U] = 0.0
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            v = beta[t + 1, u] + lb[t, u]
            if u < U:
                v = np.logaddexp(v, beta[t, u + 1] + ll[t, u])
            beta[t, u] = v
    return _close(alpha, beta, lb, ll)


def _close(alpha, beta, lb, ll):
    """alpha [T, U+1] and beta [T+1, U+2] (beta[T][U] = 0, the rest of the last row and column -inf) -> (cost, d cost / d lb, d cost / d ll)."""
    T, U1 = lb.shape
    U = U1 - 1
    total = alpha[T - 1, U] + lb[T - 1, U]
    g_lb, g_ll = np.zeros((T, U1)), np.zeros((T, U))
    if not np.isfinite(total):
        return np.inf, g_lb, g_ll
    with np.errstate(invalid="ignore"):
        e = alpha + lb + beta[1:, :U1] - total
        g_lb = -np.exp(np.where(np.isnan(e), -np.inf, e))
        if U:
            e = alpha[:, :U] + ll + beta[:T, 1:U1] - total
            g_ll = -np.exp(np.where(np.isnan(e), -np.inf, e))
    return -total, g_lb, g_ll


DIAG_FROM = 16384            # lattice nodes from which ref_normalised / ref_logits take lattice_diag (`lattice` needs a second there)


def lattice_diag(lb, ll):
    """`lattice` along the anti-diagonals d = t + u, a numpy operation per diagonal instead of a Python step per node: the same recursion,
    the same logaddexp per node, for lattices of a million nodes (1024 x 1024 in under a second).  tests/test_rnnt_api.py holds it to
    `lattice`."""
    lb, ll = np.asarray(lb, dtype=np.float64), np.asarray(ll, dtype=np.float64)
    T, U1 = lb.shape
    U = U1 - 1
    llp = np.full((T, U1), -np.inf)                   # no label behind the last one
    llp[:, :U] = ll
    alpha = np.full((T, U1), -np.inf)
    beta = np.full((T + 1, U1 + 1), -np.inf)
    alpha[0, 0] = 0.0
    beta[T, U] = 0.0
    for d in range(1, T + U):                         # alpha[t][u] from (t - 1, u) and (t, u - 1), both on diagonal d - 1
        u = np.arange(max(0, d - T + 1), min(d, U) + 1)
        t = d - u
        tp, up = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
        stay = np.where(t > 0, alpha[tp, u] + lb[tp, u], -np.inf)
        move = np.where(u > 0, alpha[t, up] + llp[t, up], -np.inf)
        alpha[t, u] = np.logaddexp(stay, move)
    for d in range(T + U - 1, -1, -1):                # beta[t][u] from (t + 1, u) and (t, u + 1), both on diagonal d + 1
        u = np.arange(max(0, d - T + 1), min(d, U) + 1)
        t = d - u
        beta[t, u] = np.logaddexp(beta[t + 1, u] + lb[t, u], beta[t, u + 1] + llp[t, u])
    return _close(alpha, beta, lb, ll)


def _lattice(lb, ll, diag=None):
    if diag is None:
        diag = lb.size >= DIAG_FROM
    return (lattice_diag if diag else lattice)(lb, ll)


def _split(lp, labels, blank):
    T, U1, _ = lp.shape
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    assert labels.size == U1 - 1
    lb = lp[:, :, blank]
    ll = lp[:, :U1 - 1, :][np.arange(T)[:, None], np.arange(U1 - 1)[None, :], labels[None, :]] if U1 > 1 else np.zeros((T, 0))
    return lb, ll, labels


def ref_normalised(log_probs, labels, blank=0, diag=None):
    """log_probs [T, U+1, V] (any real numbers: nothing normalises them).  -> (cost, d cost / d log_probs).  diag: True = lattice_diag,
    False = lattice, None = by the lattice's size (DIAG_FROM)."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, U1, _ = lp.shape
    lb, ll, labels = _split(lp, labels, blank)
    cost, g_lb, g_ll = _lattice(lb, ll, diag)
    g = np.zeros_like(lp)
    g[:, :, blank] = g_lb
    for u in range(U1 - 1):
        g[:, u, labels[u]] += g_ll[:, u]
    return cost, g


def ref_logits(x, labels, blank=0, diag=None):
    """x [T, U+1, V] raw joiner output.  -> (cost of log_softmax(x), d cost / d x = g - softmax(x) * sum_v g)."""
    x = np.asarray(x, dtype=np.float64)
    lp = log_softmax(x)
    cost, g = ref_normalised(lp, labels, blank, diag)
    with np.errstate(invalid="ignore"):
        sm = np.exp(lp)
    sm = np.where(np.isnan(sm), 0.0, sm)
    return cost, g - sm * g.sum(-1, keepdims=True)


def torch_cost(x, labels, blank=0, normalise=True):
    """(b): the cost as a torch fp64 scalar with autograd history back to x (a leaf made here).  -> (cost, x)."""
    x = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    lp = torch.log_softmax(x, -1) if normalise else x
    T, U1, _ = lp.shape
    ninf = torch.tensor(-float("inf"), dtype=torch.float64)
    a = [[None] * U1 for _ in range(T)]
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                a[t][u] = torch.zeros((), dtype=torch.float64)
                continue
            terms = []
            if t > 0:
                terms.append(a[t - 1][u] + lp[t - 1, u, blank])
            if u > 0:
                terms.append(a[t][u - 1] + lp[t, u - 1, int(labels[u - 1])])
            a[t][u] = torch.logsumexp(torch.stack(terms), 0) if len(terms) > 1 else terms[0]
            if not torch.isfinite(a[t][u]):
                a[t][u] = ninf                        # (no gradient through a dead node: logsumexp of -inf's has a NaN one)
    return -(a[T - 1][U1 - 1] + lp[T - 1, U1 - 1, blank]), x


def brute_force(log_probs, labels, blank=0):
    """(c): -log of the sum over every alignment of its probability; T <= 4, U <= 3."""
    lp = np.asarray(log_probs, dtype=np.float64)
    T, U1, _ = lp.shape
    U = U1 - 1
    assert T <= 4 and U <= 3
    paths = []
    for labs in itertools.combinations(range(T - 1 + U), U):      # which of the first T - 1 + U moves emit a label
        t = u = 0
        s = 0.0
        for k in range(T - 1 + U):
            if k in labs:
                s += lp[t, u, int(labels[u])]
                u += 1
            else:
                s += lp[t, u, blank]
                t += 1
        assert (t, u) == (T - 1, U)
        paths.append(s + lp[T - 1, U, blank])
    paths = np.asarray(paths)
    m = paths.max()
    return np.inf if not np.isfinite(m) else -(m + np.log(np.sum(np.exp(paths - m))))


# ---- batches, as the GPU tests need them ----
def random_case(seed, T_n, U_n, V, blank=0, T=None, U1=None, scale=3.0):
    """Padded raw joiner output [N, T, U1, V] fp32 and labels [N, U1 - 1] int32 without the blank; lx, ly as int lists."""
    rng = np.random.default_rng(seed)
    N = len(T_n)
    T = T or max(T_n)
    U1 = U1 or max(U_n) + 1
    x = (rng.standard_normal((N, T, U1, V)) * scale).astype(np.float32)
    labels = rng.integers(0, V - 1, (N, max(U1 - 1, 0))).astype(np.int32) if V > 1 else np.zeros((N, U1 - 1), np.int32)
    labels = labels + (labels >= blank)                                  # every column but the blank's
    return x, labels.astype(np.int32), [int(t) for t in T_n], [int(u) for u in U_n]


def batch_ref(x, labels, lx, ly, blank, fused):
    """(a) per utterance on a padded batch (x fp64-able [N, T, U1, V]) -> (costs [N], grad like x, zeros over the padding)."""
    x = np.asarray(x, dtype=np.float64)
    costs, grad = np.zeros(len(lx)), np.zeros_like(x)
    for n, (t, u) in enumerate(zip(lx, ly)):
        c, g = (ref_logits if fused else ref_normalised)(x[n, :t, :u + 1], labels[n, :u], blank)
        costs[n] = c
        grad[n, :t, :u + 1] = g
    return costs, grad


def to_compact(x, labels, lx, ly):
    """Padded [N, T, U1, V] (numpy or torch) and [N, U] -> compact rows [sum T_n (U_n + 1), V] and labels [sum U_n]."""
    cat = torch.cat if isinstance(x, torch.Tensor) else np.concatenate
    V = x.shape[-1]
    rows = cat([x[n, :t, :u + 1].reshape(-1, V) for n, (t, u) in enumerate(zip(lx, ly))])
    labs = cat([labels[n, :u] for n, u in enumerate(ly)])
    return rows, labs
