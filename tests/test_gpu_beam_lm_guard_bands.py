"""GPU test: crf_ctc_beam_lm through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as
tests/test_gpu_beam_guard_bands.py does for the LM-free call -- the outputs, the workspace (exactly as large as
crf_ctc_beam_lm_workspace_bytes says) AND the eight LM tables come from the 0xFF arena, bf16 activations with an odd V on rows that are
2-byte aligned only, lm_score_dev and trace_dev NULL and non-NULL.  No byte outside the call's own buffers may change, the tables and the
activations are unchanged afterwards, every output word is written, and the results equal those of the Python call on the same rows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ngram_ref
from tests.guard import Arena, DTYPES

pytestmark = pytest.mark.gpu
SENT = -77


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_beam_lm(core, x, lx, W, nbest, C, blank, normalize, lm, alpha, beta, time_major=False, with_optional=False, misalign=0):
    """x: CPU tensor [B,T,V] ([T,B,V] time-major).  -> (hyps, hyp_len, score, trace or None, lm_score or None) as numpy after the checks."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    H = B * nbest
    nws = core._lib.crf_ctc_beam_lm_workspace_bytes(B, T, V, W, C)
    assert nws == core._lib.crf_ctc_beam_workspace_bytes(B, T, V, W, C) and nws >= 4 * B * T * (2 * (min(C, V - 1) + 1) + W)
    nact = x.numel() * x.element_size()
    tabs = {name: torch.from_numpy(np.ascontiguousarray(a)) for name, a in lm.host_tables().items()}
    arena = Arena(dev, Arena.room([nact, 4 * B, 4 * H * T, 4 * H, 4 * H, 4 * H, 4 * B * T * W, nws] + [max(t.numel(), 1) * 4 for t in tabs.values()]))
    arena.carve("act", nact, misalign=misalign)
    arena.put("act", x)
    arena.carve("lx", 4 * B)
    arena.put("lx", torch.tensor(lx, dtype=torch.int32))
    for name, t in tabs.items():
        arena.carve("lm." + name, t.numel() * 4)
        arena.put("lm." + name, t)
    outs = (("hyps", H * T), ("hyp_len", H), ("score", H)) + ((("trace", B * T * W), ("lm_score", H)) if with_optional else ())
    for name, n in outs:
        arena.carve(name, 4 * n)
        arena.put(name, torch.full((n,), SENT, dtype=torch.int32))
    arena.carve("ws", nws)
    P, vp = arena.ptr, ctypes.c_void_p
    st = lm._struct(lambda name: P("lm." + name).value)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ctc_beam_lm(P("act"), DTYPES[x.dtype], 1 if time_major else 0, blank, 1 if normalize else 0, P("lx"), B, T, V, W, nbest,
                                       C, ctypes.byref(st), alpha, beta, P("hyps"), P("hyp_len"), P("score"),
                                       P("lm_score") if with_optional else vp(0), P("trace") if with_optional else vp(0), P("ws"), nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    for name, t in tabs.items():
        assert torch.equal(arena.get("lm." + name, torch.uint8), t.reshape(-1).view(torch.uint8)), f"the call wrote to the LM table {name}"
    got = {name: arena.get(name, torch.int32).numpy() for name, _ in outs}
    assert not any(np.any(a == SENT) for a in got.values()), "an output word was not written"
    return (got["hyps"].reshape(H, T), got["hyp_len"], got["score"].view(np.float32),
            got["trace"].reshape(B, T, W) if with_optional else None, got["lm_score"].view(np.float32) if with_optional else None)


# (73 x 65: several 64-frame chunks of the back-trace; 301: W = C = 64; 3: the smallest rows; 4096 / 8191: the row stage's two launches;
# 9 x 130 at W = nbest = 64: the trace comes back through ALL of lm_n's 64 x 64 words of LDS, in three chunks (lx = 130) and two (lx = 65))
@pytest.mark.parametrize("V,T,W,nbest,C,order", [(73, 65, 16, 5, 40, 3), (301, 17, 64, 64, 64, 4), (3, 30, 3, 2, 8, 2), (4096, 5, 16, 4, 64, 2),
                                                  (8191, 5, 64, 64, 40, 3), (9, 130, 64, 64, 8, 3)])
@pytest.mark.parametrize("time_major", [False, True])
def test_beam_lm_writes_only_its_own_memory(core, V, T, W, nbest, C, order, time_major):
    import ctc_crf
    B, blank = 3, V - 1
    rng = np.random.default_rng(V)
    x = torch.tensor((2.0 * rng.standard_normal((B, T, V))).astype(np.float32)).to(torch.bfloat16)
    lx = [T, 0, T // 2]
    lm = ctc_crf.NgramLM.from_ngrams(ngram_ref.random_model(21, V, order, fanout=5), V)
    xin = x.transpose(0, 1).contiguous() if time_major else x
    for normalize in (True, False):
        ref_h, ref_l, ref_s, ref_t, ref_m = core.ctc_beam_search(xin.to("cuda:0"), torch.tensor(lx, dtype=torch.int32), W, nbest, C, blank, time_major,
                                                                 normalize, True, lm, 0.8, 1.5, True)
        for with_optional in (False, True):
            hyps, hl, sc, tr, ls = run_beam_lm(core, xin, lx, W, nbest, C, blank, normalize, lm, 0.8, 1.5, time_major, with_optional, misalign=2)
            assert np.array_equal(hyps, ref_h.cpu().numpy()) and np.array_equal(hl, ref_l.cpu().numpy())
            assert np.array_equal(sc.view(np.int32), ref_s.cpu().numpy().view(np.int32))
            if with_optional:
                assert np.array_equal(tr, ref_t.cpu().numpy())
                assert np.array_equal(ls.view(np.int32), ref_m.cpu().numpy().view(np.int32))
