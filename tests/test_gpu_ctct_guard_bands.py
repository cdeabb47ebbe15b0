"""GPU test: crf_ctct_loss* and crf_ctct_grad* through the C ABI on buffers carved from a guard-banded arena (tests/guard.py): the joiner
output, the labels, the lengths, the weights and every output come from the 0xFF arena, each exactly as long as its sizes say; the
workspace is exactly crf_ctct_workspace_bytes long with the switch ws_gap set, so that untouched bytes follow every section; rows of odd V
in bf16 and fp16 (every second row starts on a 2-byte boundary), also with the tensor itself starting 2 bytes past a 16-byte boundary;
`invalid` NULL and non-NULL; the outputs prefilled with a sentinel.  No byte outside the calls' own buffers may change, no input may change,
every output word must be written, and the results equal the yardstick's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ctct_ref
from tests.guard import Arena
from tests.score_grad_ref import TOL

pytestmark = pytest.mark.gpu
DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SENT_I, SENT_F = -77, 768.0          # (768 is exact in bf16 and fp16)


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_ctct(core, x, labels, lx, ly, weights, blank, fused, N, T, U1, with_invalid=True, misalign=0):
    """x: CPU tensor [N, T, U1, V]; labels: CPU int32, flat.  Forward, then backward on the same workspace.
    -> (cost [N], invalid [N] or None, grad like x) as CPU tensors, after the guard and input checks."""
    dev = torch.device("cuda", 0)
    V = x.shape[-1]
    vp = ctypes.c_void_p
    esz = x.element_size()
    nws = core._lib.crf_ctct_workspace_bytes(N, T, U1, V)
    assert nws > 0
    sections = core.debug_ctct_ws_sections(N, T, U1, V)
    ins = [("labels", labels if labels.numel() else torch.zeros(1, dtype=torch.int32)), ("lx", torch.tensor(lx, dtype=torch.int32)),
           ("ly", torch.tensor(ly, dtype=torch.int32)), ("weight", torch.tensor(weights, dtype=torch.float32))]
    outs = [("cost", 4 * N, torch.float32, SENT_F)] + ([("invalid", 4 * N, torch.int32, SENT_I)] if with_invalid else []) + \
           [("grad", x.numel() * esz, x.dtype, SENT_F)]
    arena = Arena(dev, Arena.room([x.numel() * esz] + [4 * t.numel() for _, t in ins] + [n for _, n, _, _ in outs] + [nws]))
    arena.carve("x", x.numel() * esz, misalign=misalign)
    arena.put("x", x)
    for name, t in ins:
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    for name, n, dt, sent in outs:
        arena.carve(name, n, misalign=misalign if name == "grad" else 0)
        arena.put(name, torch.full((n // torch.empty(0, dtype=dt).element_size(),), sent, dtype=dt))
    arena.carve("ws", nws)
    P = lambda name: arena.ptr(name) if name in arena.carves else vp(0)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    head = (P("x"), DTYPES[x.dtype]) if fused else (P("x"),)
    mid = (blank, P("labels"), P("lx"), P("ly"), N, T, U1, V)
    with torch.cuda.device(dev):
        rc = (core._lib.crf_ctct_loss_logits if fused else core._lib.crf_ctct_loss)(*head, *mid, P("cost"), P("invalid"), P("ws"), nws, stream)
        assert rc == 0, core._lib.crf_last_error().decode()
        rc = (core._lib.crf_ctct_grad_logits if fused else core._lib.crf_ctct_grad)(*head, *mid, P("weight"), P("grad"), P("ws"), nws, stream)
        assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check(sections)
    assert bool((arena.view("ws")[:sections[0][2]] != 0xFF).any()), "the calls did not use the carved workspace"
    assert torch.equal(arena.get("x", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "a call wrote to its input"
    for name, t in ins:
        assert torch.equal(arena.get(name, torch.uint8), t.contiguous().reshape(-1).view(torch.uint8)), f"a call wrote to {name}"
    cost = arena.get("cost", torch.float32)
    inv = arena.get("invalid", torch.int32) if with_invalid else None
    grad = arena.get("grad", x.dtype, tuple(x.shape))
    assert not bool((cost == SENT_F).any()) and not bool((grad.float() == SENT_F).any()), "an output word was not written"
    assert inv is None or bool(((inv == 0) | (inv == 1)).all())
    return cost, inv, grad


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 9), (torch.bfloat16, 37), (torch.float16, 15), (torch.float32, 5), (None, 7)])
def test_ctct_calls_write_only_their_own_memory(core, dtype, V):
    blank = 2
    T_n, U_n = [7, 6, 6, 4, 8], [3, 5, 0, 2, 5]
    T, U1 = 8, 7                                                    # a padded tensor larger than every lattice
    x, labels, lx, ly = ctct_ref.random_case(V, T_n, U_n, V, blank, T, U1)
    lx[2] = 0                                                       # utterance 2 is invalid
    fused = dtype is not None
    t = torch.from_numpy(x).to(dtype) if fused else torch.log_softmax(torch.from_numpy(x), -1)
    w = [1.0, -0.5, 2.0, 0.25, 3.0]
    good = [0, 1, 3, 4]
    rc, rg = ctct_ref.batch_ref(t.double().numpy()[good], labels[good], [lx[n] for n in good], [ly[n] for n in good], blank, fused)
    assert np.isfinite(rc).all()
    rg = rg * np.asarray(w)[good][:, None, None, None]
    bound = (2.0 ** -8 if fused and dtype != torch.float32 else 0.0) * np.abs(rg) + TOL * np.abs(rg).max()
    core.debug_set("ws_gap", 1)
    try:
        for with_invalid, misalign in ((True, 0), (False, 2 if fused and dtype != torch.float32 else 4)):
            cost, inv, grad = run_ctct(core, t, torch.from_numpy(labels).reshape(-1), lx, ly, w, blank, fused, 5, T, U1,
                                       with_invalid=with_invalid, misalign=misalign)
            assert inv is None or inv.tolist() == [0, 0, 1, 0, 0]
            assert cost[2] == np.inf and not grad[2].float().any()
            assert np.all(np.abs(cost.double().numpy()[good] - rc) <= TOL * np.abs(rc))
            assert np.all(np.abs(grad.double().numpy()[good] - rg) <= bound)
    finally:
        core.debug_set("ws_gap", None)
