"""GPU test: crf_ctc_score_grad through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as
tests/test_gpu_sample_guard_bands.py does for the sampler -- the workspace exactly as large as crf_ctc_score_grad_workspace_bytes says,
one state per lane (NR = 1) and eight (NR = 8), and V = 8192 (the largest row the reduce stage keeps in LDS), both layouts.  No byte outside the call's own buffers may change, every word of grad, scores
and invalid must be written, and the results are those of tests/test_gpu_ctc_score_grad.py's first test."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guard import Arena
from tests.score_grad_ref import SENT, check_grad, flat, fold, i32, logp_normal, ref_gamma
from tests.test_gpu_ctc_score_grad import LX1, N1, small_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_guarded(core, x, hyps, utt, lx, blank, w, time_major):
    """x: CPU tensor [B,T,V] ([T,B,V] time-major).  -> (grad in x's layout, scores [H], invalid [H]) as numpy after the guard check."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    H = len(hyps)
    hl = i32([len(h) for h in hyps])
    max_l = int(hl.max())
    lab = i32(flat(hyps)) if int(hl.sum()) else torch.zeros(1, dtype=torch.int32)
    off = (torch.cumsum(hl, 0, dtype=torch.int32) - hl).to(torch.int32)
    nws = core._lib.crf_ctc_score_grad_workspace_bytes(B, H, T, V, max_l)
    assert nws >= 8 * H * T * (2 * max_l + 1)
    nact = 4 * x.numel()
    ints = (("labels", lab), ("off", off), ("len", hl), ("utt", i32(utt)), ("lx", i32(lx)))
    arena = Arena(dev, Arena.room([nact, nact, 4 * H, 4 * H, 4 * H, nws] + [4 * t.numel() for _, t in ints]))
    arena.carve("act", nact)
    arena.put("act", x)
    for name, t in ints:
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    arena.carve("weight", 4 * H)
    arena.put("weight", torch.tensor(np.asarray(w, dtype=np.float32)))
    arena.carve("grad", nact)                  # (0xFF: every float reads as NaN)
    arena.carve("score", 4 * H)
    arena.put("score", torch.full((H,), SENT, dtype=torch.float32))
    arena.carve("invalid", 4 * H)
    arena.carve("ws", nws)
    P, vp = arena.ptr, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ctc_score_grad(P("act"), 1 if time_major else 0, blank, P("labels"), P("off"), P("len"), P("utt"), P("lx"),
                                          P("weight"), B, H, T, V, max_l, P("score"), P("invalid"), P("grad"), P("ws"), nws, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    g = arena.get("grad", torch.float32, tuple(x.shape)).numpy()
    sc, inv = arena.get("score", torch.float32).numpy(), arena.get("invalid", torch.int32).numpy()
    assert not np.any(np.isnan(g)) and not np.any(sc == SENT) and np.all((inv == 0) | (inv == 1))
    return g, sc, inv


@pytest.mark.parametrize("time_major", [False, True])
def test_score_grad_writes_only_its_own_memory_nr1(core, time_major):
    blank = 2
    c = small_batch(blank)
    x = torch.tensor(c["logp"])
    g, sc, inv = run_guarded(core, x.transpose(0, 1).contiguous() if time_major else x, c["hyps"], c["utt"], LX1, blank, c["w_pos"], time_major)
    assert core.last_score_grad_kernel() == "crf_ctc_score_grad_alpha_kernel<1>"
    g = g.transpose(1, 0, 2) if time_major else g
    check_grad(g, fold(c["gamma"], c["cost"], c["valid"], c["utt"], c["w_pos"], N1), LX1, True, f"guarded NR = 1 time_major={time_major}")
    assert not np.any(g[1]) and np.array_equal(inv, 1 - c["valid"])
    ok = c["valid"] == 1
    assert np.all(np.isinf(sc[~ok])) and np.all(np.abs(sc[ok] - c["cost"][ok]) <= 1e-4 * np.abs(c["cost"][ok]))


_WIDE = {}


def wide_batch():
    """V = 8192, the most the reduce stage takes: one frame per workgroup, its LDS row 32 KiB; the last class is a label."""
    if not _WIDE:
        N, T, V, blank = 2, 5, 8192, 0
        rng = np.random.default_rng(8192)
        hyps = [np.array([V - 1, 1, V - 1], dtype=np.int32), rng.integers(1, V, size=2).astype(np.int32), np.zeros(0, np.int32),
                np.array([V - 1], dtype=np.int32)]
        utt, lx = [0, 0, 1, 1], [5, 3]
        logp = logp_normal(rng, N, T, V)
        gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
        assert valid.tolist() == [1, 1, 1, 1]
        _WIDE.update(logp=logp, hyps=hyps, utt=utt, lx=lx, blank=blank, gamma=gamma, cost=cost, valid=valid, w=rng.uniform(0.25, 2.0, size=4))
    return _WIDE


@pytest.mark.parametrize("time_major", [False, True])
def test_score_grad_writes_only_its_own_memory_v8192(core, time_major):
    c = wide_batch()
    x = torch.tensor(c["logp"])
    g, sc, inv = run_guarded(core, x.transpose(0, 1).contiguous() if time_major else x, c["hyps"], c["utt"], c["lx"], c["blank"], c["w"], time_major)
    assert core.last_score_grad_kernel() == "crf_ctc_score_grad_alpha_kernel<1>"
    g = g.transpose(1, 0, 2) if time_major else g
    check_grad(g, fold(c["gamma"], c["cost"], c["valid"], c["utt"], c["w"], 2), c["lx"], True, f"guarded V = 8192 time_major={time_major}")
    assert not np.any(inv) and np.all(np.abs(sc - c["cost"]) <= 1e-4 * np.abs(c["cost"]))


_LONG = {}


def long_batch():
    if not _LONG:
        N, T, V, blank = 2, 150, 6, 0
        rng = np.random.default_rng(88)
        pool = np.arange(1, V)
        hyps = [pool[(np.arange(130) * 2) % 5].astype(np.int32), pool[rng.integers(0, 5, size=7)].astype(np.int32), np.zeros(0, np.int32),
                pool[rng.integers(0, 5, size=145)].astype(np.int32)]              # the last: L + repeats > lx, invalid
        utt, lx = [0, 1, 1, 1], [150, 141]
        logp = logp_normal(rng, N, T, V)
        gamma, cost, valid = ref_gamma(logp, hyps, utt, lx, blank)
        assert valid.tolist() == [1, 1, 1, 0]
        _LONG.update(logp=logp, hyps=hyps, utt=utt, lx=lx, blank=blank, gamma=gamma, cost=cost, valid=valid, w=rng.uniform(0.25, 2.0, size=4))
    return _LONG


@pytest.mark.parametrize("time_major", [False, True])
def test_score_grad_writes_only_its_own_memory_nr8(core, time_major):
    c = long_batch()
    x = torch.tensor(c["logp"])
    g, sc, inv = run_guarded(core, x.transpose(0, 1).contiguous() if time_major else x, c["hyps"], c["utt"], c["lx"], c["blank"], c["w"], time_major)
    assert core.last_score_grad_kernel() == "crf_ctc_score_grad_alpha_kernel<8>"
    g = g.transpose(1, 0, 2) if time_major else g
    check_grad(g, fold(c["gamma"], c["cost"], c["valid"], c["utt"], c["w"], 2), c["lx"], True, f"guarded NR = 8 time_major={time_major}")
    assert np.array_equal(inv, 1 - c["valid"]) and sc[3] == -np.inf
