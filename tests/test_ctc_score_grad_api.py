"""CPU tests (no GPU) of the score gradient's C ABI -- crf_ctc_score_grad_workspace_bytes, crf_ctc_score_grad, crf_last_score_grad_kernel
(include/ctc_crf_hip.h) -- and of what ctc_crf.ctc_logp refuses before it touches the device."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_score_grad_workspace_bytes", "crf_ctc_score_grad", "crf_last_score_grad_kernel")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    assert callable(core.ctc_score_grad) and callable(core.last_score_grad_kernel) and callable(ctc_crf.ctc_logp)
    assert ctc_crf.ctc_logp is cat_amd.ctc_crf.ctc_logp
    doc = ctc_crf.ctc_logp.__doc__
    assert "ctc_sample(" in doc and "ctc_logp(" in doc and ".backward()" in doc and "255" in doc


def test_workspace_bytes(core):
    ws = core._lib.crf_ctc_score_grad_workspace_bytes
    for B in (1, 3, 16):
        for H in (1, 5, 160):
            for T in (1, 15, 17, 1500):
                for L in (0, 1, 31, 32, 63, 64, 127, 128, 255):
                    w = ws(B, H, T, 72, L)
                    assert w >= 8 * H * T * (2 * L + 1), (B, H, T, L, w)      # (the forward vectors are kept in fp64)
                    assert ws(B + 1, H, T, 72, L) >= w and ws(B, H + 1, T, 72, L) >= w and ws(B, H, T + 1, 72, L) >= w
                    assert L == 255 or ws(B, H, T, 72, L + 1) >= w
    assert ws(16, 160, 1500, 72, 250) > ws(16, 160, 1500, 72, 20) and ws(16, 320, 1500, 72, 20) > ws(16, 160, 1500, 72, 20)
    for bad in ((0, 5, 10, 8, 3), (-1, 5, 10, 8, 3), (2, 0, 10, 8, 3), (2, 5, 0, 8, 3), (2, 5, 10, 0, 3), (2, 5, 10, 8, -1)):
        assert ws(*bad) == -1 and core._lib.crf_last_error(), bad
    assert ws(1 << 20, 5, 1 << 12, 72, 3) == -1 and b"INT32_MAX" in core._lib.crf_last_error()
    assert ws(2, 5, 10, 8, 256) == -1 and b"255" in core._lib.crf_last_error()
    assert ws(2, 5, 10, 8192, 3) > 0 and ws(2, 5, 10, 8193, 3) == -1 and b"8192" in core._lib.crf_last_error()


PTRS = dict(act=0x1000, labels=0x2000, off=0x3000, len=0x4000, utt=0x5000, lx=0x6000, weight=0x6800, score=0x7000, invalid=0x8000, grad=0x8800,
            ws=0x9000)


def _call(core, ptrs=None, time_major=0, blank=0, B=2, H=5, T=10, V=8, L=3, ws_bytes=None):
    """The entry point with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_score_grad_workspace_bytes(B, H, T, V, L))
    rc = core._lib.crf_ctc_score_grad(vp(p["act"]), time_major, blank, vp(p["labels"]), vp(p["off"]), vp(p["len"]), vp(p["utt"]), vp(p["lx"]),
                                      vp(p["weight"]), B, H, T, V, L, vp(p["score"]), vp(p["invalid"]), vp(p["grad"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_argument_errors_without_gpu(core):
    for name in ("act", "labels", "off", "len", "utt", "lx", "grad", "ws"):
        rc, msg = _call(core, {name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _call(core, blank=blank)
        assert rc == ERR_ARG and "blank" in msg and str(blank) in msg, (blank, rc, msg)
    for kw in (dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(T=0), dict(V=0), dict(L=-1)):
        rc, msg = _call(core, ws_bytes=1 << 20, **kw)
        assert rc == ERR_ARG and msg, (kw, rc, msg)
    rc, msg = _call(core, B=1 << 20, T=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "INT32_MAX" in msg, (rc, msg)
    rc, msg = _call(core, L=256, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "255" in msg, (rc, msg)
    rc, msg = _call(core, V=8193, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    need = core._lib.crf_ctc_score_grad_workspace_bytes(2, 5, 10, 8, 3)
    assert need >= 8 * 5 * 10 * 7
    for short in (0, 1, need - 1):
        rc, msg = _call(core, ws_bytes=short)
        assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)


def _i32(*a):
    return torch.tensor(a, dtype=torch.int32)


def test_ctc_logp_refuses_what_it_does_not_take():
    import ctc_crf
    N, T, V = 2, 6, 5
    args = (_i32(1, 2, 3, 4), _i32(2, 0, 2), _i32(6, 4), _i32(1, 0, 0))
    with pytest.raises(RuntimeError, match="GPU"):                       # CPU activations: there is no CPU path
        ctc_crf.ctc_logp(torch.zeros(N, T, V), *args)
    with pytest.raises(RuntimeError, match="float32.*float64"):
        ctc_crf.ctc_logp(torch.zeros(N, T, V, dtype=torch.float64), *args)
    with pytest.raises(RuntimeError, match="float32.*bfloat16"):
        ctc_crf.ctc_logp(torch.zeros(N, T, V, dtype=torch.bfloat16), *args)
