"""CPU tests (no GPU) of ctc_beam_search: the NumPy yardstick itself (tests/beam_ref.py: against brute force over all V^T labellings, a
hand-worked case, the event counters of the GPU tests' seeded inputs, `replay` on its own trace and on a negative control), the host
checks of the Python binding (cat_amd/ctc_crf/_C.py ctc_beam_search) and the C ABI's answers before any HIP call (include/ctc_crf_hip.h
crf_ctc_beam_workspace_bytes, crf_ctc_beam)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import beam_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_beam_workspace_bytes", "crf_ctc_beam", "crf_last_beam_kernel")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_reference_against_brute_force():
    """V = 3, T <= 6, every blank, a beam that holds every prefix (at most 41 at T = 6), C = V - 1: the search is exact -- every label
    sequence of finite mass is returned, with the sum over its paths to 1e-12."""
    for T in range(0, 7):
        x = beam_ref.make_inputs(100 + T, 1, max(T, 1), 3)[0]
        for blank in range(3):
            want = {k: v for k, v in beam_ref.brute(x, T, blank).items() if v > -np.inf}
            assert len(want) <= 41
            got = beam_ref.search(x, T, 64, 64, 2, blank)["nbest"]
            assert len(got) == len(want) and {k for k, _ in got} == set(want), (T, blank)
            for k, v in got:
                assert abs(v - want[k]) <= 1e-12, (T, blank, k, v, want[k])
            assert all(a[1] >= b[1] for a, b in zip(got, got[1:]))
    # raw rows with normalize: the scores of log_softmax
    x = (3.0 * np.random.default_rng(5).standard_normal((5, 3))).astype(np.float32)
    want = beam_ref.brute(x, 5, 1, normalize=True)
    for k, v in beam_ref.search(x, 5, 64, 64, 2, 1, normalize=True)["nbest"]:
        assert abs(v - want[k]) <= 1e-12


def test_hand_worked_case():
    """Two frames over (blank, a, b), probabilities (0.5, 0.3, 0.2) and (0.4, 0.5, 0.1), W = 2, C = 2.
    Frame 0: () 0.5, (a) 0.3, (b) 0.2 -> beam [(), (a)].
    Frame 1: stay ()  = 0.5 * 0.4 = 0.20;  stay (a) = pb' 0.3 * 0.4 + pnb' [0.3 * 0.5 repeat + 0.5 * 0.5 merged from ()] = 0.52;
             () + b = 0.5 * 0.1 = 0.05;  (a) + b = 0.03;  (a) + a = 0.5 * pb(a) = 0 -- dropped.  -> beam [(a) 0.52, () 0.20]."""
    x = np.log(np.array([[0.5, 0.3, 0.2], [0.4, 0.5, 0.1]]))
    r = beam_ref.search(x, 2, 2, 2, 2, 0)
    assert [k for k, _ in r["nbest"]] == [(1,), ()]
    assert np.allclose([v for _, v in r["nbest"]], np.log([0.52, 0.20]), rtol=0, atol=1e-14)
    assert r["trace"].tolist() == [[0, 0 + 64 * 2], [1, 0]] and r["merged"] == 1 and r["reentered"] == 0
    assert beam_ref.spell(r["trace"], 2, 2) == [(1,), ()]
    # without the merge (a) would carry 0.27 only and the extension would take a slot of its own
    bad = beam_ref.search(x, 2, 2, 2, 2, 0, merge=False)
    assert [k for k, _ in bad["nbest"]] == [(1,), (1,)]
    # W = 1, top_classes = 1 (class a alone at both frames): () 0.5, then () + a = 0.5 * 0.5 = 0.25 beats the stay 0.5 * 0.4 = 0.20
    r = beam_ref.search(x, 2, 1, 1, 1, 0)
    assert r["nbest"][0][0] == (1,) and abs(r["nbest"][0][1] - np.log(0.25)) < 1e-14 and r["trace"].tolist() == [[0], [64 * 2]]
    # lx = 0: the empty prefix at score 0, no trace
    r = beam_ref.search(x, 0, 2, 2, 2, 0)
    assert r["nbest"] == [((), 0.0)] and (r["trace"] == -1).all()


@pytest.fixture(scope="module")
def case_runs():
    """search on every seeded case of the GPU replay test, once."""
    out = []
    for seed, V, W, C, T, lxs, blank in beam_ref.REPLAY_CASES:
        x = beam_ref.make_inputs(seed, len(lxs), T, V)
        out.append([(x[b], lx, beam_ref.search(x[b], lx, W, W, C, blank)) for b, lx in enumerate(lxs)])
    return out


def test_seeded_cases_raise_both_events(case_runs):
    """Every seeded input of the GPU replay test in which two prefixes can meet at all (W >= 2, more than one frame) merges an extension
    into a beam prefix, and the narrow-beam cases over two labels (V = 3, W = 2 .. 4, T = 30: the drop-and-re-enter path) and the
    list as a whole also see a parent that re-entered merge into a child that had stayed."""
    tot = 0
    for case, runs in zip(beam_ref.REPLAY_CASES, case_runs):
        seed, V, W, C, T, lxs, blank = case
        merged, reentered = sum(r["merged"] for _, _, r in runs), sum(r["reentered"] for _, _, r in runs)
        tot += reentered
        if W >= 2 and T > 1:
            assert merged >= 1, (case, merged)
        if V == 3:
            assert W in (2, 3, 4) and T == 30 and merged >= 1 and reentered >= 1, (case, merged, reentered)
    assert tot >= 3


def test_replay_accepts_its_own_trace_and_sees_a_missing_merge(case_runs):
    """replay reports 0 on beam_ref's own trace, with the same prefixes and scores; on the trace of the same search with the merge left
    out (the negative control) it reports a violation wherever that search differed at all, and it does differ in the merging cases."""
    seen = 0
    for case, runs in zip(beam_ref.REPLAY_CASES, case_runs):
        seed, V, W, C, T, lxs, blank = case
        for x, lx, r in runs:
            rp = beam_ref.replay(x, lx, r["trace"], W, C, blank)
            assert rp["excess"] == 0 and rp["why"] is None, (case, lx, rp["why"])
            got = [(p, s) for p, s in zip(rp["prefixes"], rp["scores"]) if p is not None]
            assert [p for p, _ in got] == [p for p, _ in r["nbest"]] == [p for p in beam_ref.spell(r["trace"], max(0, min(lx, T)), W) if p is not None]
            assert np.array_equal([s for _, s in got], [s for _, s in r["nbest"]])
            if V <= 5 and r["merged"]:
                bad = beam_ref.search(x, lx, W, W, C, blank, merge=False)
                rb = beam_ref.replay(x, lx, bad["trace"], W, C, blank)
                if not np.array_equal(bad["trace"], r["trace"]):
                    assert rb["excess"] == np.inf and rb["why"], (case, lx)
                    seen += 1
    assert seen >= 4
    # a trace that picks a worse candidate: the excess is the relative gap
    x = np.log(np.array([[0.5, 0.3, 0.2], [0.4, 0.5, 0.1]]))
    tr = np.array([[0, 0 + 64 * 3], [0, 1]], dtype=np.int32)                       # frame 0 keeps (b) 0.2 instead of (a) 0.3
    rp = beam_ref.replay(x, 1, tr, 2, 2, 0)
    assert abs(rp["excess"] - (np.log(0.3) - np.log(0.2)) / abs(np.log(0.2))) < 1e-12 and rp["prefixes"] == [(), (2,)]
    assert beam_ref.replay(x, 2, tr, 2, 2, 0)["excess"] > rp["excess"]              # (frame 1: () + a at 0.25 beats the stay of (b) at 0.15)
    tr = np.array([[0, -1], [0, -1]], dtype=np.int32)                               # a slot left empty beside finite candidates
    assert beam_ref.replay(x, 2, tr, 2, 2, 0)["excess"] == np.inf


def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    assert callable(ctc_crf.ctc_beam_search) and ctc_crf.ctc_beam_search is cat_amd.ctc_crf.ctc_beam_search
    assert callable(core.ctc_beam_search) and callable(core.last_beam_kernel)
    assert "CTCBeamDecoder" in ctc_crf.ctc_beam_search.__doc__ and "KenLM" in ctc_crf.ctc_beam_search.__doc__


def test_workspace_bytes(core):
    """At least the three sections, a multiple of 256, monotone in every argument; the ranges."""
    ws = core._lib.crf_ctc_beam_workspace_bytes
    for B in (1, 3, 16):
        for T in (1, 63, 64, 1500):
            for V in (1, 2, 41, 72, 5000, 8192):
                for W in (1, 16, 63):
                    for C in (1, 40, 63):
                        w = ws(B, T, V, W, C)
                        rs = min(C, V - 1) + 1
                        assert w >= 4 * B * T * (2 * rs + W) and w % 256 == 0, (B, T, V, W, C, w)
                        assert ws(B + 1, T, V, W, C) >= w and ws(B, T + 1, V, W, C) >= w
                        assert ws(B, T, V, W + 1, C) >= w and ws(B, T, V, W, C + 1) >= w
                        assert V == 8192 or ws(B, T, V + 1, W, C) >= w
    assert ws(16, 1500, 72, 16, 40) == 4 * 16 * 1500 * (41 + 41 + 16)                 # (every section a multiple of 256 as it is)
    for bad in ((0, 10, 8, 4, 4), (2, 0, 8, 4, 4), (2, 10, 0, 4, 4), (-1, 10, 8, 4, 4), (2, 10, 8, 0, 4), (2, 10, 8, 65, 4), (2, 10, 8, 4, 0),
                (2, 10, 8, 4, 65), (2, 10, 8, -3, 4)):
        assert ws(*bad) == -1 and core._lib.crf_last_error(), bad
    assert ws(1 << 20, 1 << 12, 72, 4, 4) == -1 and b"B * T > INT32_MAX" in core._lib.crf_last_error()
    assert ws(2, 10, 8193, 4, 4) == -1 and b"8192" in core._lib.crf_last_error()


PTRS = dict(act=0x1000, lx=0x2000, hyps=0x3000, len=0x4000, score=0x5000, trace=0x6000, ws=0x7000)


def _call(core, ptrs=None, dtype=0, time_major=0, blank=0, normalize=0, B=2, T=10, V=8, W=4, nbest=2, C=5, ws_bytes=None):
    """crf_ctc_beam with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_beam_workspace_bytes(B, T, V, W, C))
    rc = core._lib.crf_ctc_beam(vp(p["act"]), dtype, time_major, blank, normalize, vp(p["lx"]), B, T, V, W, nbest, C, vp(p["hyps"]),
                                vp(p["len"]), vp(p["score"]), vp(p["trace"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_argument_errors_without_gpu(core):
    for name in ("act", "lx", "hyps", "len", "score", "ws"):
        rc, msg = _call(core, {name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for dtype in (-1, 3, 17):
        rc, msg = _call(core, dtype=dtype)
        assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
    for normalize in (-1, 2):
        rc, msg = _call(core, normalize=normalize)
        assert rc == ERR_ARG and "normalize" in msg and str(normalize) in msg, (normalize, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _call(core, blank=blank)
        assert rc == ERR_ARG and "blank" in msg and str(blank) in msg, (blank, rc, msg)
    for kw in (dict(B=0), dict(B=-3), dict(T=0), dict(T=-1), dict(V=0)):
        rc, msg = _call(core, ws_bytes=1 << 20, **kw)
        assert rc == ERR_ARG and msg, (kw, rc, msg)
    for W in (0, -1, 65, 1000):
        rc, msg = _call(core, W=W, nbest=1, ws_bytes=1 << 20)
        assert rc == ERR_ARG and "beam width" in msg and str(W) in msg, (W, rc, msg)
    for C in (0, -1, 65):
        rc, msg = _call(core, C=C, ws_bytes=1 << 20)
        assert rc == ERR_ARG and "top_classes" in msg and str(C) in msg, (C, rc, msg)
    for nbest in (0, -1, 5, 64):
        rc, msg = _call(core, nbest=nbest)
        assert rc == ERR_ARG and "nbest" in msg and str(nbest) in msg, (nbest, rc, msg)
    rc, msg = _call(core, B=1 << 20, T=1 << 12, ws_bytes=1 << 50)
    assert rc == ERR_ARG and "B * T > INT32_MAX" in msg, (rc, msg)
    rc, msg = _call(core, V=8193, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    need = core._lib.crf_ctc_beam_workspace_bytes(2, 10, 8, 4, 5)
    assert need >= 4 * 2 * 10 * (6 + 6 + 4)
    for short in (0, 1, need - 1):
        rc, msg = _call(core, ws_bytes=short)
        assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)
    assert core.last_beam_kernel() in ("", "crf_beam_row_kernel<f32>", "crf_beam_row_kernel<bf16>", "crf_beam_row_kernel<f16>")


def _i32(*a):
    return torch.tensor(a, dtype=torch.int32)


def test_binding_host_checks():
    """What the binding refuses before it touches the device -- on CPU tensors: the last check of all is the device's."""
    import ctc_crf
    N, T, V = 2, 6, 5
    x, lx = torch.zeros(N, T, V), _i32(6, 4)
    fn = lambda **kw: ctc_crf.ctc_beam_search(kw.pop("x", x), kw.pop("lx", lx), **kw)
    with pytest.raises(RuntimeError, match="GPU"):                                     # CPU activations: there is no CPU path
        fn()
    with pytest.raises(RuntimeError, match="GPU"):
        fn(x=torch.zeros(T, N, V), time_major=True, beam_size=64, nbest=64, top_classes=64, fuse_log_softmax=True, return_trace=True)
    for dtype in (torch.float64, torch.int32):
        with pytest.raises(RuntimeError, match=r"float32, bfloat16 or float16.*" + str(dtype).replace(".", r"\.")):
            fn(x=torch.zeros(N, T, V, dtype=dtype))
    for blank in (-1, 5, 70):
        with pytest.raises(RuntimeError, match=rf"blank must lie in \[0, V-1=4\], got {blank}"):
            fn(blank=blank)
    for W in (0, -1, 65):
        with pytest.raises(RuntimeError, match=rf"beam_size must lie in \[1, 64\], got {W}"):
            fn(beam_size=W)
    for nbest in (0, 17):
        with pytest.raises(RuntimeError, match=rf"nbest must lie in \[1, beam_size=16\], got {nbest}"):
            fn(nbest=nbest)
    for C in (0, 65):
        with pytest.raises(RuntimeError, match=rf"top_classes must lie in \[1, 64\], got {C}"):
            fn(top_classes=C)
    with pytest.raises(RuntimeError, match=r"expect 2 input lengths, got 3"):
        fn(lx=_i32(6, 4, 4))
    with pytest.raises(RuntimeError, match=r"expect 6 input lengths, got 2"):          # time-major: N is the second dimension
        fn(time_major=True)
    with pytest.raises(RuntimeError, match=r"frame lengths must lie in \[0, T=6\], got max 7"):
        fn(lx=_i32(7, 4))
    with pytest.raises(RuntimeError, match=r"got 2 dimensions"):
        fn(x=torch.zeros(T, V))
