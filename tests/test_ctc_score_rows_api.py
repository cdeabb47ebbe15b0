"""CPU tests (no GPU) of the device-rows score calls' C ABI -- crf_ctc_score_rows, crf_ctc_score_grad_rows and their workspace functions
(include/ctc_crf_hip.h), with fake device pointers that are never dereferenced: every error is answered before any HIP call -- and of
what ctc_crf.ctc_score / ctc_logp refuse from the placement of their arguments alone."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.conftest import ROOT

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_score_rows_workspace_bytes", "crf_ctc_score_rows", "crf_ctc_score_grad_rows_workspace_bytes", "crf_ctc_score_grad_rows",
           "crf_debug_score_rows_ws_sections", "crf_debug_score_rows_ws_section_names")
PTRS = dict(act=0x1000, hyps=0x2000, len=0x4000, utt=0x5000, lx=0x6000, weight=0x6800, score=0x7000, invalid=0x8000, grad=0x8800, ws=0x9000)


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def _al(n):
    return (n + 255) & ~255


def _ncls(cap):
    return 1 + sum(cap > e for e in (31, 63, 127, 255, 511, 1023))


def _call(core, grad, ptrs=None, dtype=-1, time_major=0, blank=0, stride=40, B=2, H=5, T=10, V=8, cap=31, ws_bytes=None):
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    wsf = core._lib.crf_ctc_score_grad_rows_workspace_bytes if grad else core._lib.crf_ctc_score_rows_workspace_bytes
    if ws_bytes is None:
        ws_bytes = max(wsf(B, H, T, V, cap, dtype), 1 << 20)
    head = (vp(p["act"]), dtype, time_major, blank, vp(p["hyps"]), stride, vp(p["len"]), vp(p["utt"]), vp(p["lx"]))
    if grad:
        rc = core._lib.crf_ctc_score_grad_rows(*head, vp(p["weight"]), B, H, T, V, cap, vp(p["score"]), vp(p["invalid"]), vp(p["grad"]), vp(p["ws"]),
                                               ws_bytes, vp(0))
    else:
        rc = core._lib.crf_ctc_score_rows(*head, B, H, T, V, cap, vp(p["score"]), vp(p["invalid"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_symbols_exported_and_declared(core):
    import ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctc_crf_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in core.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
    par = inspect.signature(ctc_crf.ctc_score).parameters
    assert list(par)[-1] == "max_hyp_len" and par["max_hyp_len"].default is None
    assert inspect.signature(ctc_crf.ctc_logp).parameters["max_hyp_len"].default is None
    for doc in (ctc_crf.ctc_score.__doc__, ctc_crf.ctc_logp.__doc__):
        assert "max_hyp_len" in doc and "NOT an" in doc and "-inf" in doc
    doc = ctc_crf.ctc_logp.__doc__
    assert "workspace" in doc and "NOT with the true lengths" in doc and "hyps.cpu()" not in doc
    assert "NO value of a device tensor is read on the host" in core.stage_score_rows.__doc__


def test_workspace_bytes(core):
    ws, wsg = core._lib.crf_ctc_score_rows_workspace_bytes, core._lib.crf_ctc_score_grad_rows_workspace_bytes
    for B, H, T in ((1, 1, 1), (3, 5, 17), (16, 160, 1500)):
        for cap in (0, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047):
            n = _ncls(cap)
            plan = 2 * _al(4 * H) + 3 * _al(4 * n * H)
            assert ws(B, H, T, 72, cap, -1) == plan, (B, H, T, cap)
            for dtype in (0, 1, 2):
                assert ws(B, H, T, 72, cap, dtype) == plan + _al(4 * B * T), (B, H, T, cap, dtype)
            if cap <= 255:
                occ = _al(8 * H * T * 64 * (1 << (n - 1)))
                assert wsg(B, H, T, 72, cap, -1) == occ + _al(4 * H) + plan, (B, H, T, cap)
                assert wsg(B, H, T, 72, cap, 1) == occ + _al(4 * H) + plan + _al(4 * B * T), (B, H, T, cap)
    for f in (ws, wsg):
        for bad in ((0, 5, 10, 8, 3, -1), (2, 0, 10, 8, 3, -1), (2, 5, 0, 8, 3, -1), (2, 5, 10, 0, 3, -1), (2, 5, 10, 8, -1, -1), (2, 5, 10, 8, 3, 3),
                    (2, 5, 10, 8, 3, -2)):
            assert f(*bad) == -1 and core._lib.crf_last_error(), bad
        assert f(1 << 20, 5, 1 << 12, 72, 3, -1) == -1 and b"INT32_MAX" in core._lib.crf_last_error()
    assert ws(2, 5, 10, 8, 2047, -1) > 0 and ws(2, 5, 10, 8, 2048, -1) == -1 and b"2047" in core._lib.crf_last_error()
    assert wsg(2, 5, 10, 8, 255, -1) > 0 and wsg(2, 5, 10, 8, 256, -1) == -1 and b"255" in core._lib.crf_last_error()
    assert wsg(2, 5, 10, 8192, 3, -1) > 0 and wsg(2, 5, 10, 8193, 3, -1) == -1 and b"8192" in core._lib.crf_last_error()
    assert ws(2, 5, 10, 8193, 3, -1) > 0                       # (the scores have no limit on V)


def test_sections_by_name(core):
    sec = core.debug_score_rows_ws_sections(True, 2, 5, 10, 8, 100, 1)
    assert [s[0] for s in sec] == ["occ", "hscore", "hyp_off", "cls", "len", "cscore", "cinvalid", "lse"]
    assert sec[0][1] == 0 and all(o % 256 == 0 for _, o, _ in sec) and all(a[1] + a[2] <= b[1] for a, b in zip(sec, sec[1:]))
    assert sec[-1][1] + sec[-1][2] <= core._lib.crf_ctc_score_grad_rows_workspace_bytes(2, 5, 10, 8, 100, 1)
    assert dict((n, b) for n, _, b in sec)["occ"] == 8 * 5 * 10 * 256 and dict((n, b) for n, _, b in sec)["len"] == 4 * 3 * 5
    sec = core.debug_score_rows_ws_sections(False, 2, 5, 10, 8, 600, -1)
    assert [s[0] for s in sec] == ["hyp_off", "cls", "len", "cscore", "cinvalid"] and sec[2][2] == 4 * 6 * 5
    with core.debug_opts(ws_gap=1):
        gap = core.debug_score_rows_ws_sections(False, 2, 5, 10, 8, 600, 0)
        assert [s[0] for s in gap][-1] == "lse" and all(b[1] - (a[1] + a[2]) >= 256 for a, b in zip(gap, gap[1:]))
        assert core._lib.crf_ctc_score_rows_workspace_bytes(2, 5, 10, 8, 600, 0) >= gap[-1][1] + gap[-1][2] + 256


@pytest.mark.parametrize("grad", [False, True])
def test_errors_before_any_hip_call(core, grad):
    call = lambda **kw: _call(core, grad, **kw)
    # (a good call cannot be made without a device: everything below fails a check, nothing is launched)
    must = ("act", "hyps", "len", "utt", "lx", "ws") + (("grad",) if grad else ("score",))
    for name in must:
        rc, msg = call(ptrs={name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for dtype in (-2, 3, 7):
        rc, msg = call(dtype=dtype)
        assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
    for kw in (dict(B=0), dict(H=0), dict(T=0), dict(V=0), dict(stride=0), dict(stride=-4), dict(cap=-1), dict(B=-1)):
        rc, msg = call(ws_bytes=1 << 20, **kw)
        assert rc == ERR_ARG, (kw, rc, msg)
    rc, msg = call(H=1 << 20, stride=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "hyp_stride > INT32_MAX" in msg, (rc, msg)
    rc, msg = call(B=1 << 20, T=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "B * T > INT32_MAX" in msg, (rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = call(blank=blank)
        assert rc == ERR_ARG and "blank" in msg, (blank, rc, msg)
    limit = 255 if grad else 2047
    rc, msg = call(cap=limit + 1, stride=4096, ws_bytes=1 << 40)
    assert rc == ERR_UNSUPPORTED and str(limit) in msg, (rc, msg)
    if grad:
        rc, msg = call(V=8193, ws_bytes=1 << 40)
        assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    for dtype in (-1, 1):
        need = (core._lib.crf_ctc_score_grad_rows_workspace_bytes if grad else core._lib.crf_ctc_score_rows_workspace_bytes)(2, 5, 10, 8, 31, dtype)
        rc, msg = call(dtype=dtype, ws_bytes=need - 1)
        assert rc == ERR_WORKSPACE and str(need) in msg, (rc, msg, need)


def test_binding_refuses_from_placement_alone():
    """What can be reached without a device: max_hyp_len with CPU hypotheses, before the complaint about log_probs itself.  (A mix of
    CPU and CUDA tensors needs a CUDA tensor: tests/test_gpu_ctc_score_rows.py.)"""
    import ctc_crf
    N, T, V = 2, 10, 8
    hyps, hl, lx = torch.zeros(2, 3, dtype=torch.int32), torch.tensor([2, 3], dtype=torch.int32), torch.tensor([10, 10], dtype=torch.int32)
    for f in (ctc_crf.ctc_score, ctc_crf.ctc_logp):
        with pytest.raises(RuntimeError, match="max_hyp_len"):
            f(torch.zeros(N, T, V), hyps, hl, lx, max_hyp_len=3)
        with pytest.raises(RuntimeError, match="max_hyp_len"):
            f(torch.zeros(N, T, V), hyps, hl, lx, torch.tensor([0, 1], dtype=torch.int32), max_hyp_len=0)
        with pytest.raises(RuntimeError, match="must be on the GPU"):       # (None: today's path and today's message)
            f(torch.zeros(N, T, V), hyps, hl, lx, max_hyp_len=None)
