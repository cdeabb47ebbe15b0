"""GPU test: crf_ctc_beam_chunk through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as
tests/test_gpu_beam_guard_bands.py does for crf_ctc_beam -- both searches, the workspace exactly crf_ctc_beam_chunk_workspace_bytes, the two
states exactly B x crf_ctc_beam_state_record_bytes, trace_dev and lm_score_dev NULL and non-NULL, bf16 rows of odd V on 2-byte boundaries,
the chunk lengths only the C ABI takes (lx_chunk = (Tc + 5, -3, Tc)).  Two calls: a fresh one (state_in_dev NULL) and its continuation.
No byte outside the call's buffers may change, the input state must not change, every output word and every byte of the output records
must be written, and the results equal those of the Python call."""
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


def run_chunk(core, x, lx, W, nbest, C, blank, cap, normalize, lm, alpha, beta, state_in, with_trace, with_lm_score, misalign=0):
    """x: CPU tensor [B,Tc,V]; state_in: None or a CPU uint8 tensor [B, rec].  -> (state_out [B, rec] uint8, hyps [B nbest, cap], hyp_len,
    score bits, lm_score bits or None, trace or None) as numpy after the guard check."""
    dev = torch.device("cuda", 0)
    B, T, V = x.shape
    H = B * nbest
    rec = core._lib.crf_ctc_beam_state_record_bytes(W, cap)
    assert rec == (56 * W + 4 * W * cap + 15) // 16 * 16
    nws = core._lib.crf_ctc_beam_chunk_workspace_bytes(B, T, V, W, C)
    assert nws == core._lib.crf_ctc_beam_workspace_bytes(B, T, V, W, C)
    nact = x.numel() * x.element_size()
    arena = Arena(dev, Arena.room([nact, 4 * B, B * rec, B * rec, 4 * H * cap, 4 * H, 4 * H, 4 * H, 4 * B * T * W, nws]))
    arena.carve("act", nact, misalign=misalign)
    arena.put("act", x)
    arena.carve("lx", 4 * B)
    arena.put("lx", torch.tensor(lx, dtype=torch.int32))
    if state_in is not None:
        arena.carve("state_in", B * rec)
        arena.put("state_in", state_in)
    arena.carve("state_out", B * rec)
    outs = (("hyps", H * cap), ("hyp_len", H), ("score", H)) + ((("lm_score", H),) if with_lm_score else ()) + \
           ((("trace", B * T * W),) if with_trace else ())
    for name, n in outs:
        arena.carve(name, 4 * n)
        arena.put(name, torch.full((n,), SENT, dtype=torch.int32))
    arena.put("state_out", torch.full((B * rec,), 0xB5, dtype=torch.uint8))
    arena.carve("ws", nws)
    P, vp = arena.ptr, ctypes.c_void_p
    null = vp(0)
    tables = None
    if lm is not None:
        tables, _keep = lm.tables(dev)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ctc_beam_chunk(P("act"), DTYPES[x.dtype], 0, blank, 1 if normalize else 0, P("lx"), B, T, V, W, nbest, C,
                                          ctypes.byref(tables) if tables is not None else null, alpha, beta,
                                          P("state_in") if state_in is not None else null, null, P("state_out"), cap, P("hyps"), P("hyp_len"),
                                          P("score"), P("lm_score") if with_lm_score else null, P("trace") if with_trace else null, P("ws"),
                                          nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    if state_in is not None:
        assert torch.equal(arena.get("state_in", torch.uint8), state_in.reshape(-1)), "the call wrote to its input state"
    st = arena.get("state_out", torch.uint8, (B, rec)).numpy()
    got = [arena.get(name, torch.int32).numpy() for name, _ in outs]
    assert not any(np.any(g == SENT) for g in got)
    d = dict(zip([n for n, _ in outs], got))
    return st, d["hyps"].reshape(H, cap), d["hyp_len"], d["score"], d.get("lm_score"), d["trace"].reshape(B, T, W) if with_trace else None


@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
@pytest.mark.parametrize("V,T,W,nbest,C,cap", [(73, 9, 16, 5, 40, 12), (4096, 5, 16, 4, 64, 8), (9, 70, 64, 64, 8, 8192), (3, 30, 3, 2, 8, 7)])
def test_chunk_writes_only_its_own_memory(core, V, T, W, nbest, C, cap, with_lm):
    B, blank = 3, V - 1
    rng = np.random.default_rng(V)
    x = torch.tensor((2.0 * rng.standard_normal((B, 2 * T, V))).astype(np.float32)).to(torch.bfloat16)
    xs = (x[:, :T].contiguous(), x[:, T:].contiguous())
    lxs = ([T, 0, T // 2], [T + 5, -3, T])
    lm = alpha = beta = None
    import ctc_crf
    lm = ctc_crf.NgramLM.from_ngrams(ngram_ref.random_model(3, V, 2), V) if with_lm else None
    alpha, beta = (0.5, 0.25) if with_lm else (0.0, 0.0)
    for normalize in (True, False):
        for extras in (False, True):
            state_py, state_c = None, None
            for xc, lx in zip(xs, lxs):
                lx_py = torch.tensor([min(max(l, 0), T) for l in lx], dtype=torch.int32)
                ref = core.ctc_beam_search_chunk(xc.to("cuda:0"), lx_py, state_py, None, W, nbest, C, blank, False, normalize, lm, alpha, beta, cap,
                                                 True, with_lm)
                state_py = ref[0]
                st, hyps, hl, sc, lms, tr = run_chunk(core, xc, lx, W, nbest, C, blank, cap, normalize, lm, alpha, beta, state_c, extras,
                                                      extras and with_lm, misalign=2)   # rows on 2-byte boundaries (V is odd or the rows are)
                state_c = torch.tensor(st)
                assert np.array_equal(st, state_py.records.cpu().numpy()), "the records differ (or a byte of them was not written)"
                assert np.array_equal(hyps, ref[1].cpu().numpy()) and np.array_equal(hl, ref[2].cpu().numpy())
                assert np.array_equal(sc, ref[3].cpu().numpy().view(np.int32))
                if extras:
                    assert np.array_equal(tr, ref[4].cpu().numpy())
                    if with_lm:
                        assert np.array_equal(lms, ref[5].cpu().numpy().view(np.int32))
            assert hl.reshape(B, nbest)[0].max() > 0 and (tr is None or ((tr[1] == -1).all() and (tr[0] >= 0).any(axis=1).all()))
