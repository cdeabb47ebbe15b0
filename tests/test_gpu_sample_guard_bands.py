"""GPU test: crf_ctc_sample through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as tests/test_gpu_guard_bands.py
does for the other kernel families -- the workspace exactly as large as crf_ctc_sample_workspace_bytes says, paths_dev NULL, bf16
activations with an odd V on rows that are 2-byte aligned only.  No byte outside the call's own buffers may change, every output word
must be written, and the results equal those of the Python call on the same rows."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sample_ref
from tests.guard import Arena, DTYPES

pytestmark = pytest.mark.gpu
SENT = -77


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_sample(core, x, lx, K, seed, offset, blank, time_major=False, greedy=False, misalign=0):
    """x: CPU tensor [B,T,V] ([T,B,V] time-major).  -> (hyps [B K,T], hyp_len [B K]) as numpy after the guard check."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    H = B * K
    nws = core._lib.crf_ctc_sample_workspace_bytes(B, T, V, K)
    assert nws >= 4 * H * T
    nact = x.numel() * x.element_size()
    arena = Arena(dev, Arena.room([nact, 4 * B, 4 * H * T, 4 * H, nws]))
    arena.carve("act", nact, misalign=misalign)
    arena.put("act", x)
    arena.carve("lx", 4 * B)
    arena.put("lx", torch.tensor(lx, dtype=torch.int32))
    arena.carve("hyps", 4 * H * T)
    arena.put("hyps", torch.full((H, T), SENT, dtype=torch.int32))
    arena.carve("hyp_len", 4 * H)
    arena.put("hyp_len", torch.full((H,), SENT, dtype=torch.int32))
    arena.carve("ws", nws)
    P, vp = arena.ptr, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ctc_sample(P("act"), DTYPES[x.dtype], 1 if time_major else 0, blank, P("lx"), B, T, V, K, seed, offset,
                                      1 if greedy else 0, P("hyps"), P("hyp_len"), vp(0), P("ws"), nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    hyps, hl = arena.get("hyps", torch.int32, (H, T)).numpy(), arena.get("hyp_len", torch.int32).numpy()
    assert not np.any(hyps == SENT) and not np.any(hl == SENT)
    return hyps, hl


@pytest.mark.parametrize("V,T,K", [(73, 65, 5), (301, 17, 3)])
@pytest.mark.parametrize("time_major", [False, True])
def test_sample_writes_only_its_own_memory(core, V, T, K, time_major):
    B, blank, seed, offset = 3, V - 1, 77, 9
    rng = np.random.default_rng(V)
    x = torch.tensor((2.0 * rng.standard_normal((B, T, V))).astype(np.float32)).to(torch.bfloat16)
    lx = [T, 0, T // 2]
    xin = x.transpose(0, 1).contiguous() if time_major else x
    hyps, hl = run_sample(core, xin, lx, K, seed, offset, blank, time_major, misalign=2)     # rows on 2-byte boundaries (V is odd)
    ref_h, ref_l, paths = core.ctc_sample(xin.to("cuda:0"), torch.tensor(lx, dtype=torch.int32), K, seed, offset, blank, time_major,
                                          return_paths=True)
    assert np.array_equal(hyps, ref_h.cpu().numpy()) and np.array_equal(hl, ref_l.cpu().numpy())
    want_h, want_l, _ = sample_ref.expected_outputs(paths.cpu().numpy(), lx, K, blank)
    assert np.array_equal(hyps, want_h) and np.array_equal(hl, want_l)
    g_h, g_l = run_sample(core, xin, lx, 1, 0, 0, blank, time_major, greedy=True, misalign=2)
    am = torch.argmax(x.float(), -1).numpy()
    want_h, want_l, _ = sample_ref.expected_outputs(am, lx, 1, blank)
    assert np.array_equal(g_h, want_h) and np.array_equal(g_l, want_l)
