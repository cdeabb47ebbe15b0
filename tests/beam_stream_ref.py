"""Helpers of the streaming beam search tests (tests/test_gpu_ctc_beam_stream*.py): splits of T frames into chunks, the loop over the
chunk calls, the whole-utterance call as the yardstick, and the bit-for-bit comparison of the two.  The whole call is itself held to
tests/beam_ref.py / tests/beam_lm_ref.py by the tests of ctc_beam_search."""
import numpy as np
import torch

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SPLITS_130 = [(130,), (1,) * 130, (64, 64, 2), (63, 1, 66), (1, 129)]   # chunk ends on, before and behind the back-trace's 64-frame windows


def i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int64).reshape(-1), dtype=torch.int32)


def random_splits(T, n=3, seed=0):
    """n seeded splits of T frames into chunks of random lengths >= 1."""
    rng = np.random.default_rng([seed, T])
    out = []
    for _ in range(n):
        k = int(rng.integers(1, max(2, min(T, 9))))
        cuts = sorted(rng.choice(np.arange(1, T), size=min(k, T - 1), replace=False).tolist()) if T > 1 else []
        edges = [0] + cuts + [T]
        out.append(tuple(b - a for a, b in zip(edges, edges[1:])))
    return out


def splits_of(T, seed=0):
    """one chunk of T, T chunks of 1, three seeded random splits (and at T = 130 the window splits), without repeats."""
    s = [(T,), (1,) * T] + random_splits(T, 3, seed) + (SPLITS_130[2:] if T == 130 else [])
    return list(dict.fromkeys(s))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def chunk_lengths(lx, offset, n):
    return [int(min(max(l - offset, 0), n)) for l in lx]


def cpu(out, with_state=True):
    """a call's tensors as numpy (None stays None); the BeamState first where the call returns one"""
    head = (out[0],) if with_state else ()
    return head + tuple(None if t is None else t.cpu().numpy() for t in out[len(head):])


def whole(crf, x, lx, W, nbest, C, blank, time_major=False, fused=False, lm=None, alpha=0.0, beta=0.0):
    """ctc_beam_search -> dict(hyps [N nbest, T], len, score, trace [N, T, W], lm) as numpy."""
    out = crf.ctc_beam_search(x, i32(lx), W, nbest, C, blank, time_major, fused, return_trace=True, lm=lm, alpha=alpha, beta=beta,
                              return_lm_scores=lm is not None)
    o = cpu(out, with_state=False)
    return dict(hyps=o[0], len=o[1], score=o[3], trace=o[4], lm=o[5] if lm is not None else None)


def step(crf, chunk, lxc, state, W, nbest, C, blank, time_major=False, fused=False, lm=None, alpha=0.0, beta=0.0, cap=512, reset=None):
    """one ctc_beam_search_chunk call -> (state, dict as `whole` returns, the trace being the chunk's)"""
    out = crf.ctc_beam_search_chunk(chunk, lxc if torch.is_tensor(lxc) else i32(lxc), state, reset, W, nbest, C, blank, time_major, fused, lm,
                                    alpha, beta, cap, return_trace=True, return_lm_scores=lm is not None)
    o = cpu(out)
    return o[0], dict(hyps=o[1], len=o[2], score=o[4], trace=o[5], lm=o[6] if lm is not None else None)


def stream(crf, x, lx, split, W, nbest, C, blank, time_major=False, lx_on_device=False, on_chunk=None, **kw):
    """The chunk loop over x ([N,T,V], time_major: [T,N,V]; on the GPU) with the chunk lengths of `split`.  -> (state, the last call's dict
    with trace = the chunks' traces one after the other [N, T, W]).  on_chunk(j, frames so far, state, dict) after every call."""
    T = x.shape[0] if time_major else x.shape[1]
    assert sum(split) == T
    state, off, traces, res = None, 0, [], None
    for j, n in enumerate(split):
        chunk = (x[off:off + n] if time_major else x[:, off:off + n]).contiguous()
        lxc = i32(chunk_lengths(lx, off, n))
        state, res = step(crf, chunk, lxc.to(x.device) if lx_on_device else lxc, state, W, nbest, C, blank, time_major, **kw)
        traces.append(res["trace"])
        off += n
        if on_chunk:
            on_chunk(j, off, state, res)
    res = dict(res, trace=np.concatenate(traces, axis=1))
    return state, res


def assert_same(got, want, blank, what=""):
    """A chunk call's dict against a whole call's, bit for bit: lengths, scores, lm scores, traces (where both have one of the same
    length), the labels hyps[:len] and the blank behind them.  The rows are cap and T words long: compared over the shorter."""
    assert np.array_equal(got["len"], want["len"]), (what, got["len"], want["len"])
    assert np.array_equal(bits(got["score"]), bits(want["score"])), (what, got["score"], want["score"])
    if want["lm"] is not None:
        assert np.array_equal(bits(got["lm"]), bits(want["lm"])), (what, got["lm"], want["lm"])
    if got["trace"].shape == want["trace"].shape:
        assert np.array_equal(got["trace"], want["trace"]), (what, np.argwhere(got["trace"] != want["trace"])[:4])
    g, w = got["hyps"], want["hyps"]
    for h in range(g.shape[0]):
        n = min(int(want["len"][h]), g.shape[1], w.shape[1])
        assert np.array_equal(g[h, :n], w[h, :n]), (what, h, g[h, :n], w[h, :n])
        assert (g[h, n:] == blank).all(), (what, h)
