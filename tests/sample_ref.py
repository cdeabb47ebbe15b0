"""NumPy yardstick of ctc_sample / ctc_greedy (a plain helper module: tests/test_ctc_sample_api.py, tests/test_gpu_ctc_sample.py).

The contract (include/ctc_crf_hip.h crf_ctc_sample): draw k of frame t of utterance n uses the uniform
    u = (Philox4x32-10(counter = (t, n, k >> 2, offset), key = (seed & 0xffffffff, seed >> 32))[k & 3] >> 8) * 2^-24
and takes the smallest class whose fp32 running sum of w = exp(x - max x) exceeds u times the total.  The summation order is the kernel's,
so a draw is held to the fp64 CDF P of softmax(x) with a margin: class c is `admissible` iff w_c > 0 and P[c-1] - eps <= u < P[c] + eps."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) broadcastable against each other, key: two -> the four output words as uint64 arrays holding
    32-bit values (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the constants of Random123)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniforms(seed, offset, n, T, K):
    """u[t][k] in [0, 1) (fp64, exact multiples of 2^-24) of utterance index n, frames 0 .. T-1, draws 0 .. K-1."""
    t = np.arange(T, dtype=np.uint64)[:, None]
    q = np.arange((K + 3) // 4, dtype=np.uint64)[None, :]
    r = philox4x32_10((t, np.uint64(n), q, np.uint64(offset)), (seed & MASK, (seed >> 32) & MASK))
    words = np.stack(r, axis=-1).reshape(T, -1)[:, :K]            # [T][q][4] -> [T][4 q + j]
    return (words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def uniform(seed, offset, n, t, k):
    return float(uniforms(seed, offset, n, t + 1, k + 1)[t, k])


def admissible(x_row, u, eps):
    """x_row: [..., V] (any float dtype, read as fp64), u: [..., K] -> bool [..., K, V]: class c may be the draw of u.  A row of -inf only
    admits nothing (the contract emits the blank: checked by the caller)."""
    x = np.asarray(x_row, dtype=np.float64)
    m = np.max(x, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(x), 0.0, np.exp(x - np.where(np.isneginf(m), 0.0, m)))
    tot = np.sum(w, axis=-1, keepdims=True)
    P = np.cumsum(w, axis=-1) / np.where(tot > 0, tot, 1.0)
    lo = np.concatenate([np.zeros_like(P[..., :1]), P[..., :-1]], axis=-1)
    u = np.asarray(u, dtype=np.float64)[..., None]
    return (w > 0)[..., None, :] & (lo[..., None, :] - eps <= u) & (u < P[..., None, :] + eps)


def collapse(path, lx, blank):
    """The CTC map B on the first lx frames of `path`: frame t is kept iff path[t] != blank and (t == 0 or path[t] != path[t-1])."""
    return [int(path[t]) for t in range(lx) if path[t] != blank and (t == 0 or path[t] != path[t - 1])]


def expected_outputs(paths, lx, K, blank):
    """paths [N K][T] with the classes of the frames t < lx[n] (anything behind) -> (hyps [N K][T] padded with the blank, hyp_len [N K],
    paths with -1 behind lx) as int32 arrays: what the call must return for these frame paths."""
    paths = np.asarray(paths)
    H, T = paths.shape
    hyps = np.full((H, T), blank, dtype=np.int32)
    lens = np.zeros(H, dtype=np.int32)
    full = np.full((H, T), -1, dtype=np.int32)
    for h in range(H):
        n = max(0, min(int(lx[h // K]), T))
        seq = collapse(paths[h], n, blank)
        hyps[h, :len(seq)] = seq
        lens[h] = len(seq)
        full[h, :n] = paths[h, :n]
    return hyps, lens, full
