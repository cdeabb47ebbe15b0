"""GPU test: crf_ctc_score_grad_logits through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as
tests/test_gpu_score_grad_guard_bands.py does for the log-prob call -- bf16 raw output with an odd V whose first row starts 2 bytes past a
multiple of 256 (every row on a 2-byte boundary only), the workspace exactly as large as crf_ctc_score_grad_logits_workspace_bytes says,
score_dev and invalid_dev NULL, both layouts.  No byte outside the call's own buffers may change, every word of grad must be written, and
the result is held to the reference of tests/score_grad_logits_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guard import Arena
from tests.score_grad_logits_ref import core, fold_raw, kernel_name, parity_case
from tests.score_grad_ref import TOL, flat, i32
from tests.util import rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("time_major", [False, True])
def test_score_grad_logits_writes_only_its_own_memory(time_major):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = parity_case("odd_v_bf16")
    dev = torch.device("cuda", 0)
    x = c["x"].transpose(0, 1).contiguous() if time_major else c["x"]
    B, T, V = c["x"].shape
    assert x.dtype == torch.bfloat16 and V % 2 == 1
    hyps, w = c["hyps"], c["weights"]["pos"]
    H = len(hyps)
    hl = i32([len(h) for h in hyps])
    max_l = int(hl.max())
    off = (torch.cumsum(hl, 0, dtype=torch.int32) - hl).to(torch.int32)
    nws = core._lib.crf_ctc_score_grad_logits_workspace_bytes(B, H, T, V, max_l)
    assert nws >= core._lib.crf_ctc_score_grad_workspace_bytes(B, H, T, V, max_l) + 4 * B * T
    ints = (("labels", i32(flat(hyps))), ("off", off), ("len", hl), ("utt", i32(c["utt"])), ("lx", i32(c["lx"])))
    arena = Arena(dev, Arena.room([2 * x.numel(), 4 * x.numel(), 4 * H, nws] + [4 * t.numel() for _, t in ints]))
    arena.carve("act", 2 * x.numel(), misalign=2)
    arena.put("act", x)
    for name, t in ints:
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    arena.carve("weight", 4 * H)
    arena.put("weight", torch.tensor(np.asarray(w, dtype=np.float32)))
    arena.carve("grad", 4 * x.numel())             # (0xFF: every float reads as NaN)
    arena.carve("ws", nws)
    P, vp = arena.ptr, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ctc_score_grad_logits(P("act"), 1, 1 if time_major else 0, c["blank"], P("labels"), P("off"), P("len"), P("utt"), P("lx"),
                                                 P("weight"), B, H, T, V, max_l, vp(0), vp(0), P("grad"), P("ws"), nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    assert core.last_score_grad_kernel() == kernel_name(c["nr"], "bf16")
    assert torch.equal(arena.get("act", torch.uint8), x.reshape(-1).view(torch.uint8)), "the call wrote to its input"
    g = arena.get("grad", torch.float32, tuple(x.shape)).numpy()
    assert not np.any(np.isnan(g))
    g = g.transpose(1, 0, 2) if time_major else g
    ref = fold_raw(c["ref"], c["utt"], w, c["lx"])
    for u, n in enumerate(c["lx"]):
        assert not np.any(g[u, int(n):])
    e = rel_err(g, ref)
    print(f"[score_grad_logits] guarded bf16 V = {V} time_major={time_major}: rel_err {e:.3e}")
    assert e <= TOL, e
