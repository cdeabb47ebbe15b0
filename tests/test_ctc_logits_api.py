"""CPU tests (no GPU) of the raw-network-output twins of the numerator-only C ABI -- crf_ctc_fwd_bwd_logits, crf_ctc_align_logits_workspace_bytes,
crf_ctc_align_logits (include/ctc_crf_hip.h) -- of the Python keywords on top of them, and of the score formula of the alignment on raw
logits: raw Viterbi sum minus the fp64 sum of the frames' lse, held to a brute force under log_softmax."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import align_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
NEW = ("crf_ctc_fwd_bwd_logits", "crf_ctc_align_logits_workspace_bytes", "crf_ctc_align_logits")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_symbols_exported_and_keywords(core):
    import ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    m = ctc_crf.WARP_CTC_LOSS()
    assert (m.size_average, m.blank_label, m.fuse_log_softmax, m.time_major) == (True, 0, False, False)
    assert m.ctc == ctc_crf._WARP_CTC_GPU.apply                      # the defaults are today's module
    m = ctc_crf.WARP_CTC_LOSS(size_average=False, blank_label=3, fuse_log_softmax=True, time_major=True)
    assert (m.size_average, m.blank_label, m.fuse_log_softmax, m.time_major) == (False, 3, True, True)
    assert m.ctc == ctc_crf._WARP_CTC_LOGITS_GPU.apply
    assert ctc_crf.WARP_CTC_LOSS(time_major=True).ctc == ctc_crf._WARP_CTC_GPU.apply
    sig = inspect.signature(ctc_crf.ctc_align)
    assert sig.parameters["fuse_log_softmax"].default is False
    assert list(sig.parameters)[:6] == ["log_probs", "labels", "input_lengths", "label_lengths", "blank", "time_major"]
    assert inspect.signature(core.ctc_align).parameters["fused"].default is False


def test_python_argument_checks_without_gpu():
    import torch
    import ctc_crf
    args = (torch.tensor([1], dtype=torch.int32), torch.tensor([4], dtype=torch.int32), torch.tensor([1], dtype=torch.int32))
    with pytest.raises(AssertionError, match="network output"):
        ctc_crf.ctc_align(torch.zeros(1, 4, 5, dtype=torch.float64), *args, fuse_log_softmax=True)
    with pytest.raises(AssertionError, match="network output"):
        ctc_crf.WARP_CTC_LOSS(fuse_log_softmax=True)(torch.zeros(1, 4, 5, dtype=torch.float64), *args)
    with pytest.raises(AssertionError):
        ctc_crf.ctc_align(torch.zeros(1, 4, 5, dtype=torch.bfloat16), *args, fuse_log_softmax=True)   # not on the GPU


def test_logits_workspace_bytes(core):
    ws, ws0 = core._lib.crf_ctc_align_logits_workspace_bytes, core._lib.crf_ctc_align_workspace_bytes
    for B in (1, 2, 4, 64, 256):
        for T in (1, 15, 16, 17, 100, 1500, 3000):
            for L in (0, 1, 255, 256, 2047):
                w = ws(B, T, 72, L)
                assert w >= ws0(B, T, 72, L) + 4 * B * T
                assert ws(B + 1, T, 72, L) >= w and ws(B, T + 1, 72, L) >= w
    assert ws(128, 1500, 72, 100) > ws(64, 1500, 72, 100) and ws(64, 3000, 72, 100) > ws(64, 1500, 72, 100)
    assert ws(4, 100, 8192, 10) > 0 and ws(4, 100, 72, 2047) > 0
    assert ws(4, 100, 8193, 10) < 0 and b"8192" in core._lib.crf_last_error()
    assert ws(4, 100, 72, 2048) < 0 and b"2047" in core._lib.crf_last_error()
    assert ws(0, 100, 72, 10) < 0 and ws(4, 0, 72, 10) < 0 and ws(4, 100, 0, 10) < 0 and ws(4, 100, 72, -1) < 0
    assert ws(1 << 20, 1 << 12, 72, 10) < 0            # B * T > INT32_MAX


def _align(core, ptrs=None, dtype=1, time_major=0, blank=0, B=2, T=10, V=8, L=3, ws_bytes=None):
    """crf_ctc_align_logits with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(act=0x1000, labels=0x2000, off=0x3000, lx=0x4000, ly=0x5000, pos=0x6000, score=0x7000, invalid=0x8000, ws=0x9000)
    p.update(ptrs or {})
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_align_logits_workspace_bytes(B, T, V, L))
    vp = ctypes.c_void_p
    rc = core._lib.crf_ctc_align_logits(vp(p["act"]), dtype, time_major, blank, vp(p["labels"]), vp(p["off"]), vp(p["lx"]), vp(p["ly"]),
                                        B, T, V, L, vp(p["pos"]), vp(p["score"]), vp(p["invalid"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_align_logits_argument_errors_without_gpu(core):
    for name in ("act", "labels", "off", "lx", "ly", "pos", "score", "ws"):
        rc, msg = _align(core, {name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for dtype in (-1, 3):
        rc, msg = _align(core, dtype=dtype)
        assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _align(core, blank=blank)
        assert rc == ERR_ARG and "blank" in msg, (blank, rc, msg)
    rc, msg = _align(core, V=8193)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    rc, msg = _align(core, L=2048)
    assert rc == ERR_UNSUPPORTED and "2047" in msg, (rc, msg)
    rc, msg = _align(core, B=1 << 20, T=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "INT32_MAX" in msg, (rc, msg)
    for B, T, V, L in ((0, 10, 8, 3), (2, 0, 8, 3), (2, 10, 0, 3), (2, 10, 8, -1)):
        rc, msg = _align(core, B=B, T=T, V=V, L=L, ws_bytes=1 << 20)
        assert rc == ERR_ARG and msg, (B, T, V, L, rc, msg)
    need = core._lib.crf_ctc_align_logits_workspace_bytes(2, 10, 8, 3)
    for dtype in (0, 1, 2):
        for short in (0, 1, core._lib.crf_ctc_align_workspace_bytes(2, 10, 8, 3), need - 1):
            rc, msg = _align(core, dtype=dtype, ws_bytes=short)
            assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)


def _ctc(core, ptrs=None, dtype=1, time_major=0, blank=0, B=2, T=10, V=8, L=3, c_ctc=1.0, ws_bytes=None):
    """crf_ctc_fwd_bwd_logits with fake device pointers."""
    p = dict(act=0x1000, labels=0x2000, off=0x3000, lx=0x4000, ly=0x5000, grad=0x6000, loss=0x7000, costs=0x8000, invalid=0x8800, ws=0x9000)
    p.update(ptrs or {})
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_workspace_bytes(None, B, T, V, L))
    vp = ctypes.c_void_p
    rc = core._lib.crf_ctc_fwd_bwd_logits(vp(p["act"]), dtype, time_major, blank, vp(p["labels"]), vp(p["off"]), vp(p["lx"]), vp(p["ly"]),
                                          B, T, V, L, c_ctc, vp(p["grad"]), vp(p["loss"]), vp(p["costs"]), vp(p["invalid"]), vp(p["ws"]),
                                          ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_ctc_logits_argument_errors_without_gpu(core):
    for name in ("act", "labels", "off", "lx", "ly", "grad", "loss", "ws"):
        rc, msg = _ctc(core, {name: 0})
        assert rc == ERR_ARG and msg, (name, rc, msg)
    for dtype in (-1, 3):
        for tm in (0, 1):
            rc, msg = _ctc(core, dtype=dtype, time_major=tm)
            assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
    rc, msg = _ctc(core, c_ctc=0.0)
    assert rc == ERR_ARG and "c_ctc" in msg, (rc, msg)
    for blank in (-1, 8):
        rc, msg = _ctc(core, blank=blank, time_major=1)
        assert rc == ERR_ARG and "blank" in msg, (blank, rc, msg)
    rc, msg = _ctc(core, V=8193)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    rc, msg = _ctc(core, L=2048)
    assert rc == ERR_UNSUPPORTED and "2047" in msg, (rc, msg)
    rc, msg = _ctc(core, B=1 << 20, T=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG, (rc, msg)
    need = core._lib.crf_workspace_bytes(None, 2, 10, 8, 3)
    for tm in (0, 1):
        rc, msg = _ctc(core, time_major=tm, blank=5, ws_bytes=need - 1)          # time-major and a blank inside get as far as the workspace
        assert rc == ERR_WORKSPACE and str(need) in msg, (rc, msg)


def emulate_score(x, labels, blank):
    """The contract of crf_ctc_align_logits in NumPy: the Viterbi path on the RAW values (fp32 sums in frame order are what the kernel
    forms; the tiny case here is summed in fp64), score = raw best sum - sum_t lse_t with lse_t = m_t + log sum_v exp(x_tv - m_t)."""
    x = np.asarray(x, dtype=np.float64)
    raw, pos = align_ref.viterbi(x, labels, blank)
    if pos is None:
        return -np.inf, None
    m = x.max(-1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(-1))
    return float(raw - lse.sum()), pos


def test_score_formula_against_brute_force_under_log_softmax():
    """Every alignment takes one entry per frame, so the best raw path is the best path under log_softmax and its score there is the raw
    sum minus the frames' lse: against the brute force over all V^T labellings on log_softmax in fp64."""
    rng = np.random.default_rng(77)
    V = 3
    n = 0
    for blank in range(V):
        pool = [c for c in range(V) if c != blank]
        for labels in ([], [pool[0]], [pool[1], pool[0]], [pool[0], pool[0]], [pool[0], pool[1], pool[1]]):
            for T in (1, 3, 5, 6):
                x = rng.normal(0.0, 2.0, size=(T, V))
                score, pos = emulate_score(x, labels, blank)
                m = x.max(-1, keepdims=True)
                lsm = x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))
                bscore, bseq = align_ref.brute_force(lsm, labels, blank)
                if not align_ref.fits(labels, T):
                    assert pos is None and score == -np.inf and bseq is None
                    continue
                n += 1
                assert abs(score - bscore) <= 1e-12 * max(1.0, abs(bscore)), (blank, labels, T, score, bscore)
                assert np.array_equal(align_ref.pos_to_classes(pos, labels, blank), bseq), (blank, labels, T)
    assert n >= 40
