"""GPU test: crf_rnnt_simple_loss and crf_rnnt_simple_grad through the C ABI on buffers carved from a guard-banded arena (tests/guard.py,
64 KiB bands): f, g, the labels, the lengths, the weights and every output come from the 0xFF arena, each exactly as long as its sizes
say; the workspace is exactly crf_rnnt_simple_workspace_bytes long with the switch ws_gap set, so that untouched bytes follow every
section; `invalid` is NULL; rows of odd V in bf16 / fp16 (every second row starts on a 2-byte boundary), also with the tensors themselves
starting 2 bytes past a 16-byte boundary; the outputs prefilled with a sentinel; a second run with one of the two gradients NULL.  No
byte outside the calls' own buffers may change, no input may change, every output word must be written -- the workspace's partial sums
start as NaN (0xFF), so reading one that was never written shows -- and the results equal the yardstick's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rnnt_simple_ref
from tests.guard import GUARD, Arena
from tests.score_grad_ref import TOL

pytestmark = pytest.mark.gpu
DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SENT_F = 768.0               # (exact in bf16 and fp16)


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_simple(core, f, g, labels, lx, ly, weights, blank, want=(True, True), misalign=0):
    """f [N, T, V], g [N, U1, V]: CPU tensors of one dtype; labels CPU int32 [N, U1 - 1].  Forward, then backward on the same workspace.
    -> (cost [N], grad_f or None, grad_g or None) as CPU tensors, after the guard and input checks."""
    dev = torch.device("cuda", 0)
    (N, T, V), U1 = f.shape, g.shape[1]
    vp = ctypes.c_void_p
    esz = f.element_size()
    nws = core._lib.crf_rnnt_simple_workspace_bytes(N, T, U1, V)
    assert nws > 0
    sections = core.debug_rnnt_simple_ws_sections(N, T, U1, V)
    ins = [("labels", labels if labels.numel() else torch.zeros(1, dtype=torch.int32)), ("lx", torch.tensor(lx, dtype=torch.int32)),
           ("ly", torch.tensor(ly, dtype=torch.int32)), ("weight", torch.tensor(weights, dtype=torch.float32))]
    outs = [("cost", 4 * N, torch.float32)] + [(name, t.numel() * esz, t.dtype) for name, t, k in (("grad_f", f, want[0]), ("grad_g", g, want[1])) if k]
    arena = Arena(dev, Arena.room([f.numel() * esz, g.numel() * esz] + [4 * t.numel() for _, t in ins] + [n for _, n, _ in outs] + [nws]))
    for name, t in (("f", f), ("g", g)):
        arena.carve(name, t.numel() * esz, misalign=misalign)
        arena.put(name, t)
    for name, t in ins:
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    for name, n, dt in outs:
        arena.carve(name, n, misalign=0 if name == "cost" else misalign)
        arena.put(name, torch.full((n // torch.empty(0, dtype=dt).element_size(),), SENT_F, dtype=dt))
    arena.carve("ws", nws)
    P = lambda name: arena.ptr(name) if name in arena.carves else vp(0)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    head = (P("f"), P("g"), DTYPES[f.dtype], blank, P("labels"), P("lx"), P("ly"), N, T, U1, V)
    with torch.cuda.device(dev):
        rc = core._lib.crf_rnnt_simple_loss(*head, P("cost"), vp(0), P("ws"), nws, stream)
        assert rc == 0, core._lib.crf_last_error().decode()
        rc = core._lib.crf_rnnt_simple_grad(*head, P("weight"), P("grad_f"), P("grad_g"), P("ws"), nws, stream)
        assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check(sections)
    assert bool((arena.view("ws")[:sections[0][2]] != 0xFF).any()), "the calls did not use the carved workspace"
    for name, t in [("f", f), ("g", g)] + ins:
        assert torch.equal(arena.get(name, torch.uint8), t.contiguous().reshape(-1).view(torch.uint8)), f"a call wrote to {name}"
    cost = arena.get("cost", torch.float32)
    grads = [arena.get(name, t.dtype, tuple(t.shape)) if k else None for name, t, k in (("grad_f", f, want[0]), ("grad_g", g, want[1]))]
    assert not bool((cost == SENT_F).any()), "a cost was not written"
    for t in grads:
        assert t is None or (not bool((t.float() == SENT_F).any()) and bool(torch.isfinite(t.float()).all())), "a gradient word was not written"
    return cost, grads[0], grads[1]


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 9), (torch.bfloat16, 37), (torch.float16, 15), (torch.float32, 5), (torch.float32, 261)])
def test_simple_calls_write_only_their_own_memory(core, dtype, V):
    assert GUARD == 64 * 1024
    blank = 2
    T_n, U_n = [7, 4, 6, 1, 35], [3, 5, 0, 2, 33]                   # (35 frames: three chunks of 16, 34 rows: two register tiles)
    T, U1 = 37, 36                                                  # padded tensors larger than every lattice
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(V, T_n, U_n, V, blank, T, U1)
    lx[2] = 0                                                       # utterance 2 is invalid
    tf, tg = torch.from_numpy(f).to(dtype), torch.from_numpy(g).to(dtype)
    w = [1.0, -0.5, 2.0, 0.25, 3.0]
    good = [0, 1, 3, 4]
    glx, gly = [lx[n] for n in good], [ly[n] for n in good]
    rc, rf, rg = rnnt_simple_ref.batch_ref(tf.double().numpy()[good], tg.double().numpy()[good], labels[good], glx, gly, blank)
    scale = np.asarray(w)[good][:, None, None]
    rf, rg = rf * scale, rg * scale
    rel = 2.0 ** -8 if dtype != torch.float32 else 0.0
    core.debug_set("ws_gap", 1)
    try:
        for want, misalign in (((True, True), 0), ((True, False), 2 if dtype != torch.float32 else 4), ((False, True), 0)):
            cost, gf, gg = run_simple(core, tf, tg, torch.from_numpy(labels), lx, ly, w, blank, want=want, misalign=misalign)
            assert cost[2] == np.inf
            assert np.all(np.abs(cost.double().numpy()[good] - rc) <= TOL * np.abs(rc))
            for grad, ref in ((gf, rf), (gg, rg)):
                if grad is None:
                    continue
                assert not grad[2].float().any()
                assert np.all(np.abs(grad.double().numpy()[good] - ref) <= rel * np.abs(ref) + TOL * np.abs(ref).max())
    finally:
        core.debug_set("ws_gap", None)
