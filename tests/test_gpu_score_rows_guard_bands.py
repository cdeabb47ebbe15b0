"""GPU test: crf_ctc_score_rows and crf_ctc_score_grad_rows through the C ABI on buffers carved from a guard-banded arena
(tests/guard.py), as tests/test_gpu_score_grad_guard_bands.py does for the host-list call -- the workspace exactly as large as the
workspace function says, 256 untouched bytes behind every section (switch ws_gap), the optional outputs NULL, bf16 rows starting two bytes
past a multiple of 256, and the mixed-class list of tests/test_gpu_ctc_logp_rows.py (lengths 3, 40, 100, 200: four classes into one occ
section).  No byte outside a buffer or section may change, every word of the outputs is written, the results match the fp64 oracle."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guard import Arena
from tests.score_grad_logits_ref import fold_raw, quantise, raw_ref
from tests.score_grad_ref import SENT, TOL, check_grad, fold, i32
from tests.test_gpu_ctc_logp_rows import LX2, N2, T2, V2, W_POS, mixed_batch
from tests.util import rel_err

pytestmark = pytest.mark.gpu
INT32_MIN = -2 ** 31
ROW_W = 203                                    # words per row of hyps: odd, above the longest hypothesis


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_guarded(core, grad, x, hyps, utt, lx, blank, w, time_major, len_cap, null_outputs=False, misalign=0):
    """x: CPU tensor [B,T,V] ([T,B,V] time-major), fp32 log-probs or bf16 raw output.  One call of crf_ctc_score_grad_rows (grad) or
    crf_ctc_score_rows under ws_gap = 1 -> (grad in x's layout or None, scores [H] or None, invalid [H] or None) after the guard check."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    H = len(hyps)
    dtype = -1 if x.dtype == torch.float32 else 1
    lab = torch.full((H, ROW_W), INT32_MIN, dtype=torch.int32)
    for h, a in enumerate(hyps):
        lab[h, :len(a)] = i32(a)
    ints = (("hyps", lab), ("len", i32([len(h) for h in hyps])), ("utt", i32(utt)), ("lx", i32(lx)))
    want_score = not (grad and null_outputs)
    want_invalid, want_weight = not null_outputs, grad and w is not None and not null_outputs
    with core.debug_opts(ws_gap=1):
        nws = (core._lib.crf_ctc_score_grad_rows_workspace_bytes if grad else core._lib.crf_ctc_score_rows_workspace_bytes)(B, H, T, V, len_cap, dtype)
        assert nws > 0, core._lib.crf_last_error().decode()
        sections = core.debug_score_rows_ws_sections(grad, B, H, T, V, len_cap, dtype)
        nact = x.numel() * x.element_size()
        arena = Arena(dev, Arena.room([nact, 4 * x.numel(), 4 * H, 4 * H, 4 * H, nws] + [4 * t.numel() for _, t in ints]))
        arena.carve("act", nact, misalign=misalign)
        arena.put("act", x)
        for name, t in ints:
            arena.carve(name, 4 * t.numel())
            arena.put(name, t)
        if want_weight:
            arena.carve("weight", 4 * H)
            arena.put("weight", torch.tensor(np.asarray(w, dtype=np.float32)))
        if grad:
            arena.carve("grad", 4 * x.numel())    # (0xFF: every float reads as NaN)
        if want_score:
            arena.carve("score", 4 * H)
            arena.put("score", torch.full((H,), SENT, dtype=torch.float32))
        if want_invalid:
            arena.carve("invalid", 4 * H)
        arena.carve("ws", nws)
        vp = ctypes.c_void_p
        P = lambda name: arena.ptr(name) if name in arena.carves else vp(0)
        stream = vp(torch.cuda.current_stream(dev).cuda_stream)
        head = (P("act"), dtype, 1 if time_major else 0, blank, P("hyps"), ROW_W, P("len"), P("utt"), P("lx"))
        with torch.cuda.device(dev):
            if grad:
                rc = core._lib.crf_ctc_score_grad_rows(*head, P("weight"), B, H, T, V, len_cap, P("score"), P("invalid"), P("grad"), P("ws"), nws, stream)
            else:
                rc = core._lib.crf_ctc_score_rows(*head, B, H, T, V, len_cap, P("score"), P("invalid"), P("ws"), nws, stream)
        assert rc == 0, core._lib.crf_last_error().decode()
        torch.cuda.synchronize()
    arena.check(sections)
    assert bool((arena.view("ws")[sections[-1][1]:sections[-1][1] + sections[-1][2]] != 0xFF).any()), "the call did not use the carved workspace"
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    assert torch.equal(arena.get("hyps", torch.int32), lab.reshape(-1)), "the call wrote to the hypotheses"
    g = arena.get("grad", torch.float32, tuple(x.shape)).numpy() if grad else None
    sc = arena.get("score", torch.float32).numpy() if want_score else None
    inv = arena.get("invalid", torch.int32).numpy() if want_invalid else None
    assert g is None or not np.any(np.isnan(g))
    assert sc is None or not np.any(sc == SENT)
    assert inv is None or np.all((inv == 0) | (inv == 1))
    return g, sc, inv


def _layout(x, time_major):
    return x.transpose(0, 1).contiguous() if time_major else x


def _check_scores(sc, inv, cost, valid):
    ok = valid == 1
    assert np.array_equal(inv, 1 - valid) and np.all(sc[~ok] == -np.inf) and np.all(np.abs(sc[ok] - cost[ok]) <= TOL * np.abs(cost[ok]))


@pytest.mark.parametrize("len_cap", [200, 2047])
def test_score_rows_writes_only_its_own_memory(core, len_cap):
    c = mixed_batch()
    _, sc, inv = run_guarded(core, False, torch.tensor(c["logp"]), c["hyps"], c["utt"], LX2, c["blank"], None, False, len_cap)
    assert core.last_score_kernel() == ("crf_ctc_score_wave_kernel<8>" if len_cap == 200 else "crf_ctc_score_wg_kernel<8>")
    _check_scores(sc, inv, c["cost"], c["valid"])


@pytest.mark.parametrize("time_major", [False, True])
def test_score_grad_rows_writes_only_its_own_memory(core, time_major):
    c = mixed_batch()
    x = _layout(torch.tensor(c["logp"]), time_major)
    g, sc, inv = run_guarded(core, True, x, c["hyps"], c["utt"], LX2, c["blank"], W_POS, time_major, 255)
    assert core.last_score_grad_kernel() == "crf_rows_grad_alpha_kernel<8>"
    g = g.transpose(1, 0, 2) if time_major else g
    check_grad(g, fold(c["gamma"], c["cost"], c["valid"], c["utt"], W_POS, N2), LX2, True, f"guarded rows time_major={time_major}")
    assert not np.any(g[1])
    _check_scores(sc, inv, c["cost"], c["valid"])


def test_score_grad_rows_with_null_outputs_and_a_bound_below_the_longest(core):
    """score_dev, invalid_dev and weight_dev NULL (all weights 1); len_cap = 127: the hypothesis of 200 labels takes no part."""
    c = mixed_batch()
    g, sc, inv = run_guarded(core, True, torch.tensor(c["logp"]), c["hyps"], c["utt"], LX2, c["blank"], None, False, 127, null_outputs=True)
    assert sc is None and inv is None and core.last_score_grad_kernel() == "crf_rows_grad_alpha_kernel<4>"
    check_grad(g, fold(c["gamma"], c["cost"], np.array([1, 1, 0, 1]), c["utt"], None, N2), LX2, True, "guarded rows, NULL outputs, len_cap 127")
    _, sc, inv = run_guarded(core, False, torch.tensor(c["logp"]), c["hyps"], c["utt"], LX2, c["blank"], None, False, 127, null_outputs=True)
    assert inv is None and sc[2] == -np.inf and np.all(np.isfinite(sc[[0, 1, 3]]))


_RAW = {}


def raw_mixed():
    """mixed_batch's hypotheses on bf16 raw output N(0, 2); the reference on its exact fp32 upcast, computed once."""
    if not _RAW:
        c = mixed_batch()
        xb, x32 = quantise(np.random.default_rng(8200).normal(0.0, 2.0, size=(N2, T2, V2)), "bf16")
        _RAW.update(x=xb, ref=raw_ref(x32, c["hyps"], c["utt"], LX2, c["blank"]))
    return _RAW


@pytest.mark.parametrize("time_major", [False, True])
def test_bf16_rows_on_two_byte_alignment(core, time_major):
    c, r = mixed_batch(), raw_mixed()
    x = _layout(r["x"], time_major)
    ref = r["ref"]
    assert np.all(ref["valid"] == 1) and np.all(np.isfinite(ref["cost"]))
    _, sc, inv = run_guarded(core, False, x, c["hyps"], c["utt"], LX2, c["blank"], None, time_major, 200, misalign=2)
    _check_scores(sc, inv, ref["cost"], ref["valid"])
    g, sc2, inv2 = run_guarded(core, True, x, c["hyps"], c["utt"], LX2, c["blank"], W_POS, time_major, 200, misalign=2)
    assert core.last_score_grad_kernel() == "crf_rows_grad_alpha_raw_kernel<8, bf16>"
    assert np.array_equal(sc.view(np.int32), sc2.view(np.int32)) and np.array_equal(inv, inv2)
    g = g.transpose(1, 0, 2) if time_major else g
    want = fold_raw(ref, c["utt"], W_POS, LX2)
    e = rel_err(g, want)
    print(f"[rows guard] bf16 time_major={time_major}: rel_err {e:.3e}")
    assert e <= TOL and not np.any(g[0, 400:]) and not np.any(g[1])
