"""CPU tests (no GPU) of the raw-output score gradient's C ABI -- crf_ctc_score_grad_logits_workspace_bytes, crf_ctc_score_grad_logits
(include/ctc_crf_hip.h) -- and of what ctc_crf.ctc_logp(fuse_log_softmax=...) takes and refuses before it touches the device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.conftest import ROOT
from tests.score_grad_logits_ref import core

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_score_grad_logits_workspace_bytes", "crf_ctc_score_grad_logits")


def test_symbols_exported_and_declared():
    import ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctc_crf_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\s*\(" % s, hdr), s
    for f in (core.stage_score_meta, core.ctc_score_staged, core.ctc_score_grad):
        names = list(inspect.signature(f).parameters)
        assert names[-1] == "fused" and inspect.signature(f).parameters["fused"].default is False, (f.__name__, names)
    par = inspect.signature(ctc_crf.ctc_logp).parameters
    assert list(par)[-1] == "fuse_log_softmax" and par["fuse_log_softmax"].default is False
    doc = ctc_crf.ctc_logp.__doc__
    assert "fuse_log_softmax" in doc and "ctc_sample(" in doc and "ctc_logp(" in doc and ".backward()" in doc and "255" in doc


def _al(n):
    return (n + 255) & ~255


def test_workspace_bytes():
    ws, ws32 = core._lib.crf_ctc_score_grad_logits_workspace_bytes, core._lib.crf_ctc_score_grad_workspace_bytes
    for B in (1, 3, 16):
        for H in (1, 5, 160):
            for T in (1, 15, 17, 1500):
                for L in (0, 1, 31, 32, 63, 64, 127, 128, 255):
                    assert ws(B, H, T, 72, L) == ws32(B, H, T, 72, L) + _al(4 * B * T), (B, H, T, L)      # (a section ends on a multiple of 256)
    for bad in ((0, 5, 10, 8, 3), (-1, 5, 10, 8, 3), (2, 0, 10, 8, 3), (2, 5, 0, 8, 3), (2, 5, 10, 0, 3), (2, 5, 10, 8, -1)):
        assert ws32(*bad) == -1 and ws(*bad) == -1 and core._lib.crf_last_error(), bad
    assert ws(1 << 20, 5, 1 << 12, 72, 3) == -1 and b"INT32_MAX" in core._lib.crf_last_error()
    assert ws(2, 5, 10, 8, 256) == -1 and b"255" in core._lib.crf_last_error()
    assert ws(2, 5, 10, 8192, 3) > 0 and ws(2, 5, 10, 8193, 3) == -1 and b"8192" in core._lib.crf_last_error()


PTRS = dict(act=0x1000, labels=0x2000, off=0x3000, len=0x4000, utt=0x5000, lx=0x6000, weight=0x6800, score=0x7000, invalid=0x8000, grad=0x8800,
            ws=0x9000)


def _call(ptrs=None, dtype=1, time_major=0, blank=0, B=2, H=5, T=10, V=8, L=3, ws_bytes=None):
    """The entry point with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_score_grad_logits_workspace_bytes(B, H, T, V, L))
    rc = core._lib.crf_ctc_score_grad_logits(vp(p["act"]), dtype, time_major, blank, vp(p["labels"]), vp(p["off"]), vp(p["len"]), vp(p["utt"]),
                                             vp(p["lx"]), vp(p["weight"]), B, H, T, V, L, vp(p["score"]), vp(p["invalid"]), vp(p["grad"]),
                                             vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_argument_errors_without_gpu():
    for dtype in (-1, 3, 7):
        rc, msg = _call(dtype=dtype)
        assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
    for dtype in (0, 1, 2):
        for name in ("act", "labels", "off", "len", "utt", "lx", "grad", "ws"):
            rc, msg = _call({name: 0}, dtype=dtype)
            assert rc == ERR_ARG and "null" in msg and "crf_ctc_score_grad_logits" in msg, (name, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _call(blank=blank)
        assert rc == ERR_ARG and "blank" in msg and str(blank) in msg, (blank, rc, msg)
    for kw in (dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(T=0), dict(V=0), dict(L=-1)):
        rc, msg = _call(ws_bytes=1 << 20, **kw)
        assert rc == ERR_ARG and msg, (kw, rc, msg)
    rc, msg = _call(B=1 << 20, T=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "INT32_MAX" in msg, (rc, msg)
    rc, msg = _call(L=256, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "255" in msg, (rc, msg)
    rc, msg = _call(V=8193, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    need = core._lib.crf_ctc_score_grad_logits_workspace_bytes(2, 5, 10, 8, 3)
    need32 = core._lib.crf_ctc_score_grad_workspace_bytes(2, 5, 10, 8, 3)
    assert need == need32 + _al(4 * 2 * 10)
    for short in (0, 1, need32, need - 1):              # (the log-prob call's workspace is too small: it has no room for the lse values)
        rc, msg = _call(ws_bytes=short)
        assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)


def _i32(*a):
    return torch.tensor(a, dtype=torch.int32)


def test_ctc_logp_refuses_what_it_does_not_take():
    import ctc_crf
    N, T, V = 2, 6, 5
    args = (_i32(1, 2, 3, 4), _i32(2, 0, 2), _i32(6, 4), _i32(1, 0, 0))
    with pytest.raises(RuntimeError, match="float16.*float64"):           # fp64 is no network output either
        ctc_crf.ctc_logp(torch.zeros(N, T, V, dtype=torch.float64), *args, fuse_log_softmax=True)
    for dt in (torch.float32, torch.bfloat16, torch.float16):            # taken: refused for being on the CPU only
        with pytest.raises(RuntimeError, match="GPU"):
            ctc_crf.ctc_logp(torch.zeros(N, T, V, dtype=dt), *args, fuse_log_softmax=True)
    with pytest.raises(RuntimeError, match="float32.*bfloat16"):          # the default is today's: fp32 log-probs only
        ctc_crf.ctc_logp(torch.zeros(N, T, V, dtype=torch.bfloat16), *args)
    with pytest.raises(RuntimeError, match="float32.*bfloat16"):
        ctc_crf.ctc_logp(torch.zeros(N, T, V, dtype=torch.bfloat16), *args, fuse_log_softmax=False)
