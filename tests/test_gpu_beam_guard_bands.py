"""GPU test: crf_ctc_beam through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as
tests/test_gpu_sample_guard_bands.py does for the sampler -- the workspace exactly as large as crf_ctc_beam_workspace_bytes says, bf16
activations with an odd V on rows that are 2-byte aligned only, trace_dev NULL and non-NULL.  No byte outside the call's own buffers may
change, every output word must be written, and the results equal those of the Python call on the same rows.  Also the lengths only the
C ABI takes: lx > T and lx < 0."""
import ctypes

import numpy as np
import pytest
import torch

from tests import beam_ref
from tests.guard import Arena, DTYPES

pytestmark = pytest.mark.gpu
SENT = -77


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_beam(core, x, lx, W, nbest, C, blank, normalize, time_major=False, with_trace=False, misalign=0):
    """x: CPU tensor [B,T,V] ([T,B,V] time-major).  -> (hyps [B nbest,T], hyp_len, score, trace or None) as numpy after the guard check."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    H = B * nbest
    nws = core._lib.crf_ctc_beam_workspace_bytes(B, T, V, W, C)
    assert nws >= 4 * B * T * (2 * (min(C, V - 1) + 1) + W)
    nact = x.numel() * x.element_size()
    arena = Arena(dev, Arena.room([nact, 4 * B, 4 * H * T, 4 * H, 4 * H, 4 * B * T * W, nws]))
    arena.carve("act", nact, misalign=misalign)
    arena.put("act", x)
    arena.carve("lx", 4 * B)
    arena.put("lx", torch.tensor(lx, dtype=torch.int32))
    for name, n in (("hyps", H * T), ("hyp_len", H), ("score", H)) + ((("trace", B * T * W),) if with_trace else ()):
        arena.carve(name, 4 * n)
        arena.put(name, torch.full((n,), SENT, dtype=torch.int32))
    arena.carve("ws", nws)
    P, vp = arena.ptr, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ctc_beam(P("act"), DTYPES[x.dtype], 1 if time_major else 0, blank, 1 if normalize else 0, P("lx"), B, T, V, W, nbest,
                                    C, P("hyps"), P("hyp_len"), P("score"), P("trace") if with_trace else vp(0), P("ws"), nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    hyps, hl = arena.get("hyps", torch.int32, (H, T)).numpy(), arena.get("hyp_len", torch.int32).numpy()
    sc_bits = arena.get("score", torch.int32).numpy()
    tr = arena.get("trace", torch.int32, (B, T, W)).numpy() if with_trace else None
    assert not np.any(hyps == SENT) and not np.any(hl == SENT) and not np.any(sc_bits == SENT) and (tr is None or not np.any(tr == SENT))
    return hyps, hl, sc_bits.view(np.float32), tr


# (4096: the row stage's launch with four rows and 64 KiB of LDS per workgroup; 8191: an odd wide V, one row per workgroup;
# 9 x 130 at W = nbest = 64: the back-trace's LDS buffer at its full width, three chunks (lx = 130) and two (lx = 65))
@pytest.mark.parametrize("V,T,W,nbest,C", [(73, 65, 16, 5, 40), (301, 17, 64, 64, 64), (3, 30, 3, 2, 8), (4096, 5, 16, 4, 64), (8191, 5, 64, 64, 40),
                                           (9, 130, 64, 64, 8)])
@pytest.mark.parametrize("time_major", [False, True])
def test_beam_writes_only_its_own_memory(core, V, T, W, nbest, C, time_major):
    B, blank = 3, V - 1
    rng = np.random.default_rng(V)
    x = torch.tensor((2.0 * rng.standard_normal((B, T, V))).astype(np.float32)).to(torch.bfloat16)
    lx = [T, 0, T // 2]
    xin = x.transpose(0, 1).contiguous() if time_major else x
    for normalize in (True, False):
        ref_h, ref_l, ref_s, ref_t = core.ctc_beam_search(xin.to("cuda:0"), torch.tensor(lx, dtype=torch.int32), W, nbest, C, blank, time_major,
                                                          normalize, return_trace=True)
        for with_trace in (False, True):
            hyps, hl, sc, tr = run_beam(core, xin, lx, W, nbest, C, blank, normalize, time_major, with_trace, misalign=2)   # rows on 2-byte boundaries (V is odd)
            assert np.array_equal(hyps, ref_h.cpu().numpy()) and np.array_equal(hl, ref_l.cpu().numpy())
            assert np.array_equal(sc.view(np.int32), ref_s.cpu().numpy().view(np.int32))
            if with_trace:
                assert np.array_equal(tr, ref_t.cpu().numpy())
                for b in range(B):
                    pre = beam_ref.spell(tr[b], lx[b], W)
                    for r in range(nbest):
                        want = pre[r] or ()
                        assert hl[b * nbest + r] == len(want) and tuple(hyps[b * nbest + r, :len(want)]) == want
                        assert (hyps[b * nbest + r, len(want):] == blank).all()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("time_major", [False, True])
def test_lengths_outside_0_T(core, time_major, normalize):
    """lx[b] > T counts as T and lx[b] <= 0 as 0 (include/ctc_crf_hip.h) -- lengths the Python call refuses, so only the C ABI can bring
    them: lx = (T + 5, -3, T) on three utterances of which the last repeats the first.  The first equals the last and equals itself at
    lx = T bit for bit, the second is the empty prefix at score 0 with every trace word -1, and no byte outside the buffers changes."""
    B, T, V, W, nbest, C, blank = 3, 9, 73, 8, 4, 40, 72
    rng = np.random.default_rng(11)
    x = torch.tensor((2.0 * rng.standard_normal((B, T, V))).astype(np.float32)).to(torch.bfloat16)
    x[2] = x[0]
    xin = x.transpose(0, 1).contiguous() if time_major else x
    hyps, hl, sc, tr = run_beam(core, xin, [T + 5, -3, T], W, nbest, C, blank, normalize, time_major, with_trace=True, misalign=2)
    base = run_beam(core, xin, [T, 0, T], W, nbest, C, blank, normalize, time_major, with_trace=True, misalign=2)
    for got, want in zip((hyps, hl, sc, tr), base):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    hyps, hl, sc = hyps.reshape(B, nbest, T), hl.reshape(B, nbest), sc.reshape(B, nbest)
    for a in (hyps, hl, sc.view(np.int32), tr):
        assert np.array_equal(a[0], a[2])
    assert (tr[0] >= 0).any(axis=1).all() and hl[0].max() > 0 and np.isfinite(sc[0]).all()      # (all T frames of the first were searched)
    assert (tr[1] == -1).all() and (hl[1] == 0).all() and (hyps[1] == blank).all()
    assert sc[1, 0] == 0.0 and (sc[1, 1:] == -np.inf).all()
    nt = run_beam(core, xin, [T + 5, -3, T], W, nbest, C, blank, normalize, time_major, with_trace=False, misalign=2)
    assert np.array_equal(nt[0].reshape(B, nbest, T), hyps) and np.array_equal(nt[1].reshape(B, nbest), hl)
    assert np.array_equal(nt[2].view(np.int32).reshape(B, nbest), sc.view(np.int32))
