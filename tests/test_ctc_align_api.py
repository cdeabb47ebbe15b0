"""CPU tests (no GPU) of the forced alignment's C ABI -- crf_ctc_align_workspace_bytes, crf_ctc_align (include/ctc_crf_hip.h) -- and of
the fp64 NumPy Viterbi the GPU tests measure against (tests/align_ref.py), which is itself held to a brute force over all frame labellings."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import align_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_symbols_exported_and_surface(core):
    import ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in ("crf_ctc_align_workspace_bytes", "crf_ctc_align"):
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    assert callable(ctc_crf.ctc_align) and callable(core.ctc_align)


def test_workspace_bytes_positive_monotone_and_limits(core):
    ws = core._lib.crf_ctc_align_workspace_bytes
    base = ws(4, 100, 72, 10)
    assert base > 0
    # 2 bits per (frame, state) at the least
    assert base >= 4 * 100 * 21 * 2 // 8
    for B in (1, 2, 4, 64, 256):
        for T in (1, 15, 16, 17, 100, 1500, 3000):
            for L in (0, 1, 31, 32, 255, 256, 2047):
                w = ws(B, T, 72, L)
                assert w > 0
                assert ws(B + 1, T, 72, L) >= w and ws(B, T + 1, 72, L) >= w
                assert L == 2047 or ws(B, T, 72, L + 1) >= w
                assert w >= B * T * (2 * L + 1) * 2 // 8
    assert ws(64, 1500, 72, 2047) > ws(64, 1500, 72, 100) and ws(64, 3000, 72, 100) > ws(64, 1500, 72, 100) and ws(128, 1500, 72, 100) > ws(64, 1500, 72, 100)
    assert ws(4, 100, 8192, 10) > 0 and ws(4, 100, 72, 2047) > 0
    assert ws(4, 100, 8193, 10) < 0 and b"8192" in core._lib.crf_last_error()
    assert ws(4, 100, 72, 2048) < 0 and b"2047" in core._lib.crf_last_error()
    assert ws(0, 100, 72, 10) < 0 and ws(4, 0, 72, 10) < 0 and ws(4, 100, 0, 10) < 0 and ws(4, 100, 72, -1) < 0
    assert ws(1 << 20, 1 << 12, 72, 10) < 0            # B * T > INT32_MAX


def _call(core, ptrs=None, time_major=0, blank=0, B=2, T=10, V=8, L=3, ws_bytes=None):
    """crf_ctc_align with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(act=0x1000, labels=0x2000, off=0x3000, lx=0x4000, ly=0x5000, pos=0x6000, score=0x7000, invalid=0x8000, ws=0x9000)
    p.update(ptrs or {})
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_align_workspace_bytes(B, T, V, L))
    vp = ctypes.c_void_p
    rc = core._lib.crf_ctc_align(vp(p["act"]), time_major, blank, vp(p["labels"]), vp(p["off"]), vp(p["lx"]), vp(p["ly"]), B, T, V, L,
                                 vp(p["pos"]), vp(p["score"]), vp(p["invalid"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_argument_errors_without_gpu(core):
    for name in ("act", "labels", "off", "lx", "ly", "pos", "score", "ws"):
        rc, msg = _call(core, {name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _call(core, blank=blank)
        assert rc == ERR_ARG and "blank" in msg, (blank, rc, msg)
    rc, msg = _call(core, V=8193)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    rc, msg = _call(core, L=2048)
    assert rc == ERR_UNSUPPORTED and "2047" in msg, (rc, msg)
    rc, msg = _call(core, B=1 << 20, T=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "INT32_MAX" in msg, (rc, msg)
    for B, T, V, L in ((0, 10, 8, 3), (2, 0, 8, 3), (2, 10, 0, 3), (2, 10, 8, -1)):
        rc, msg = _call(core, B=B, T=T, V=V, L=L, ws_bytes=1 << 20)
        assert rc == ERR_ARG and msg, (B, T, V, L, rc, msg)
    need = core._lib.crf_ctc_align_workspace_bytes(2, 10, 8, 3)
    for short in (0, 1, need - 1):
        rc, msg = _call(core, ws_bytes=short)
        assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)


def test_python_argument_checks_without_gpu(core):
    """What the binding refuses before it touches the device (host-resident metadata)."""
    import torch
    import ctc_crf
    x = torch.zeros(1, 4, 5)
    with pytest.raises(AssertionError):
        ctc_crf.ctc_align(x, torch.tensor([1], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), torch.tensor([1], dtype=torch.int32))  # not on the GPU


def _cases():
    """Every transcript over the non-blank classes of V = 3 with L <= 3 (repeats included), T <= 6, blank at 0, 1 and 2."""
    V = 3
    for blank in range(V):
        pool = [c for c in range(V) if c != blank]
        for L in range(0, 4):
            for labels in itertools.product(pool, repeat=L):
                for T in range(1, 7):
                    yield blank, labels, T


def test_numpy_viterbi_against_brute_force():
    """Score and path of tests/align_ref.viterbi = the best of all V^T labellings that collapse to the transcript, on continuous random
    inputs (no ties: distinct paths have distinct sums with probability one; checked: the runner-up is at least 1e-9 away or absent)."""
    rng = np.random.default_rng(20260)
    V = 3
    n = nvalid = 0
    for blank, labels, T in _cases():
        x = np.log(rng.dirichlet(np.ones(V), size=T))
        score, pos = align_ref.viterbi(x, labels, blank)
        bscore, bseq = align_ref.brute_force(x, labels, blank)
        n += 1
        if not align_ref.fits(labels, T):
            assert pos is None and score == -np.inf and bseq is None, (blank, labels, T)
            continue
        nvalid += 1
        assert bseq is not None and abs(score - bscore) <= 1e-12 * max(1.0, abs(bscore)), (blank, labels, T, score, bscore)
        assert np.array_equal(align_ref.pos_to_classes(pos, labels, blank), bseq), (blank, labels, T)
        align_ref.check_path(np.concatenate([pos, [-2, -2]]), labels, T, blank)
        assert abs(align_ref.path_score(x, pos, labels, T, blank) - score) <= 1e-12 * max(1.0, abs(score))
    assert n == 3 * 15 * 6 and nvalid > n // 2


def test_numpy_viterbi_tie_rule_and_dead_paths():
    """Uniform inputs: every alignment ties, and the rule (stay, then advance, then skip; state 2L before 2L-1 at the end) picks the one
    that reaches the final blank as early as it can and stays there (the back-trace prefers 'stay' from the end backwards): each label
    once from frame 0 on, a blank only between equal labels, then trailing blanks."""
    V, blank = 4, 0
    x = np.full((9, V), np.log(0.25))
    score, pos = align_ref.viterbi(x, [1, 2, 2, 3], blank)
    assert abs(score - 9 * np.log(0.25)) < 1e-12
    align_ref.check_path(pos, [1, 2, 2, 3], 9, blank)
    assert pos.tolist() == [0, 1, -1, 2, 3, -1, -1, -1, -1]
    # -inf columns: one alignment left / none left
    x = np.full((3, V), -np.inf)
    x[0, 1] = x[1, 0] = x[2, 1] = np.log(0.5)
    score, pos = align_ref.viterbi(x, [1, 1], blank)
    assert pos.tolist() == [0, -1, 1] and abs(score - 3 * np.log(0.5)) < 1e-12
    x[1, 0] = -np.inf
    assert align_ref.viterbi(x, [1, 1], blank) == (-np.inf, None)
    assert align_ref.viterbi(np.zeros((2, V)), [1, 1], blank) == (-np.inf, None)      # L + repeats > lx
    score, pos = align_ref.viterbi(np.log(np.full((3, V), 0.25)), [], blank)
    assert pos.tolist() == [-1, -1, -1]
