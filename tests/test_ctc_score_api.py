"""CPU tests (no GPU) of the hypothesis scores' C ABI -- crf_ctc_score, crf_ctc_score_logits_workspace_bytes, crf_ctc_score_logits
(include/ctc_crf_hip.h) -- and of the host checks and the metadata staging of the Python binding (cat_amd/ctc_crf/_C.py ctc_score)."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_score", "crf_ctc_score_logits_workspace_bytes", "crf_ctc_score_logits", "crf_last_score_kernel")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_symbols_exported_and_surface(core):
    import ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    assert callable(ctc_crf.ctc_score) and callable(core.ctc_score) and callable(core.last_score_kernel)
    import cat_amd.ctc_crf
    assert ctc_crf.ctc_score is cat_amd.ctc_crf.ctc_score
    assert "autograd" in ctc_crf.ctc_score.__doc__


def test_workspace_bytes(core):
    ws = core._lib.crf_ctc_score_logits_workspace_bytes
    for B in (1, 2, 4, 64, 256):
        for T in (1, 15, 16, 17, 100, 1500, 3000):
            for V in (1, 7, 72, 300, 100000):
                w = ws(B, T, V)
                assert w >= 4 * B * T
                assert ws(B + 1, T, V) >= w and ws(B, T + 1, V) >= w
    assert ws(128, 1500, 72) > ws(64, 1500, 72) and ws(64, 3000, 72) > ws(64, 1500, 72)
    assert ws(0, 100, 72) < 0 and ws(4, 0, 72) < 0 and ws(4, 100, 0) < 0 and ws(-1, 100, 72) < 0
    assert ws(1 << 20, 1 << 12, 72) < 0 and b"INT32_MAX" in core._lib.crf_last_error()


PTRS = dict(act=0x1000, labels=0x2000, off=0x3000, len=0x4000, utt=0x5000, lx=0x6000, score=0x7000, invalid=0x8000, ws=0x9000)


def _call(core, logits=False, ptrs=None, dtype=0, time_major=0, blank=0, B=2, H=5, T=10, V=8, L=3, ws_bytes=None):
    """The two entry points with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    tail = (time_major, blank, vp(p["labels"]), vp(p["off"]), vp(p["len"]), vp(p["utt"]), vp(p["lx"]), B, H, T, V, L, vp(p["score"]),
            vp(p["invalid"]))
    if logits:
        if ws_bytes is None:
            ws_bytes = max(0, core._lib.crf_ctc_score_logits_workspace_bytes(B, T, V))
        rc = core._lib.crf_ctc_score_logits(vp(p["act"]), dtype, *tail, vp(p["ws"]), ws_bytes, vp(0))
    else:
        rc = core._lib.crf_ctc_score(vp(p["act"]), *tail, vp(0))
    return rc, core._lib.crf_last_error().decode()


@pytest.mark.parametrize("logits", [False, True])
def test_argument_errors_without_gpu(core, logits):
    for name in ("act", "labels", "off", "len", "utt", "lx", "score") + (("ws",) if logits else ()):
        rc, msg = _call(core, logits, {name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _call(core, logits, blank=blank)
        assert rc == ERR_ARG and "blank" in msg and str(blank) in msg, (blank, rc, msg)
    for kw in (dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(T=0), dict(V=0), dict(L=-1)):
        rc, msg = _call(core, logits, ws_bytes=1 << 20, **kw)
        assert rc == ERR_ARG and msg, (kw, rc, msg)
    rc, msg = _call(core, logits, B=1 << 20, T=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "INT32_MAX" in msg, (rc, msg)
    rc, msg = _call(core, logits, L=2048)
    assert rc == ERR_UNSUPPORTED and "2047" in msg, (rc, msg)
    if logits:
        for dtype in (-1, 3, 17):
            rc, msg = _call(core, True, dtype=dtype)
            assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
        need = core._lib.crf_ctc_score_logits_workspace_bytes(2, 10, 8)
        assert need >= 4 * 2 * 10
        for short in (0, 1, need - 1):
            rc, msg = _call(core, True, ws_bytes=short)
            assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)


def _i32(*a):
    return torch.tensor(a, dtype=torch.int32)


def test_binding_host_checks(core):
    """What the binding refuses before it touches the device: each with the offending value in the message."""
    N, T, V = 2, 6, 5
    lx = _i32(6, 4)
    flat, hl, hu = _i32(1, 2, 3, 4), _i32(2, 0, 2), _i32(1, 0, 0)
    meta, H, max_l = core._stage_score_meta(flat, hl, lx, hu, N, T, V, 0)
    assert (H, max_l) == (3, 2)
    with pytest.raises(RuntimeError, match=r"hyp_utt must lie in \[0, N-1=1\].*2"):
        core._stage_score_meta(flat, hl, lx, _i32(1, 2, 0), N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"hyp_utt must lie.*-1"):
        core._stage_score_meta(flat, hl, lx, _i32(1, -1, 0), N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"expect 3 entries of hyp_utt.*got 2"):
        core._stage_score_meta(flat, hl, lx, _i32(1, 0), N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"expect 2 hypotheses, got 3"):          # hyp_utt=None: H = N
        core._stage_score_meta(flat, hl, lx, None, N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"expect 2 input lengths, got 3"):
        core._stage_score_meta(flat, hl, _i32(6, 4, 4), hu, N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"sum\(label_lengths\)=5 exceeds len\(labels\)=4"):
        core._stage_score_meta(flat, _i32(2, 1, 2), lx, hu, N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"expect 3 rows of hyps.*got 2"):
        core._stage_score_meta(_i32(1, 2, 3, 4).reshape(2, 2), hl, lx, hu, N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"max\(hyp_lengths\)=2 exceeds the row length 1"):
        core._stage_score_meta(_i32(1, 2, 3).reshape(3, 1), hl, lx, hu, N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"labels must lie in \[1, V-1=4\]"):     # a label equal to the blank 0
        core._stage_score_meta(_i32(1, 0, 3, 4), hl, lx, hu, N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"without the blank 3.*the blank itself"):
        core._stage_score_meta(_i32(1, 2, 3, 4), hl, lx, hu, N, T, V, 3)
    with pytest.raises(RuntimeError, match=r"labels must lie"):                      # a label >= V
        core._stage_score_meta(_i32(1, 2, 5, 4), hl, lx, hu, N, T, V, 0)
    with pytest.raises(RuntimeError, match=r"frame lengths must lie in \[0, T=6\]"):
        core._stage_score_meta(flat, hl, _i32(7, 4), hu, N, T, V, 0)
    import ctc_crf
    with pytest.raises(RuntimeError, match="GPU"):                                   # CPU activations: there is no CPU path
        ctc_crf.ctc_score(torch.zeros(N, T, V), flat, hl, lx, hu)
    with pytest.raises(AssertionError):
        ctc_crf.ctc_score(torch.zeros(N, T, V, dtype=torch.float64), flat, hl, lx, hu)


def test_padded_and_flat_forms_stage_the_same_metadata(core):
    N, T, V, blank = 3, 20, 9, 4
    rows = [[1, 2, 2], [], [8, 0, 3, 5, 7], [6], [0, 0]]
    hl = _i32(*[len(r) for r in rows])
    hu = _i32(2, 0, 0, 1, 2)
    lx = _i32(20, 11, 7)
    flat = _i32(*[c for r in rows for c in r])
    padded = torch.full((5, 7), blank, dtype=torch.int64)        # padding holds the BLANK (and the row is longer than needed): never staged
    for h, r in enumerate(rows):
        padded[h, :len(r)] = torch.tensor(r, dtype=torch.int64)
    a, Ha, La = core._stage_score_meta(flat, hl, lx, hu, N, T, V, blank)
    b, Hb, Lb = core._stage_score_meta(padded, hl.long(), lx.long(), hu.long(), N, T, V, blank)
    assert (Ha, La) == (Hb, Lb) == (5, 5)
    assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b)
    # the layout the call slices: lx | lengths | offsets | utterances | labels
    assert a.tolist() == [20, 11, 7] + [3, 0, 5, 1, 2] + [0, 3, 3, 8, 9] + [2, 0, 0, 1, 2] + flat.tolist()
    # hyp_utt=None: the identity
    c, Hc, _ = core._stage_score_meta(flat[:9], hl[:3], lx, None, N, T, V, blank)
    assert Hc == 3 and c[3 + 6:3 + 9].tolist() == [0, 1, 2]
