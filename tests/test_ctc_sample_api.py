"""CPU tests (no GPU) of ctc_sample / ctc_greedy: the NumPy yardstick itself (tests/sample_ref.py: Philox4x32-10 against the Random123
known answers, the collapse against a brute-force statement), the host checks of the Python binding (cat_amd/ctc_crf/_C.py ctc_sample) and
the C ABI's answers before any HIP call (include/ctc_crf_hip.h crf_ctc_sample_workspace_bytes, crf_ctc_sample)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import sample_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_sample_workspace_bytes", "crf_ctc_sample", "crf_last_sample_kernel")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = " ".join("%08x" % int(w) for w in sample_ref.philox4x32_10(counter, key))
        assert got == want, (counter, key, got)


def test_uniforms_follow_the_counter_layout():
    """counter = (t, n, k >> 2, offset), key = (seed_lo, seed_hi); draw k takes word k & 3, its top 24 bits."""
    seed, offset, n = 0x299f31d0a4093822, 0x03707344, 0x85a308d3
    u = sample_ref.uniforms(seed, offset, n, 3, 9)
    assert u.shape == (3, 9) and np.all(u >= 0) and np.all(u < 1)
    for t, k in ((0, 0), (2, 3), (1, 4), (2, 8)):
        r = sample_ref.philox4x32_10((t, n, k >> 2, offset), (seed & 0xffffffff, seed >> 32))
        assert u[t, k] == (int(r[k & 3]) >> 8) / 2.0 ** 24
        assert sample_ref.uniform(seed, offset, n, t, k) == u[t, k]
    # the third known answer, read as uniforms: t = 0x243f6a88 does not fit a frame loop, so through the words themselves
    r = sample_ref.philox4x32_10((0x243f6a88, n, 0x13198a2e, offset), (seed & 0xffffffff, seed >> 32))
    assert [int(w) >> 8 for w in r] == [0xd16cfe, 0x94fdcc, 0x5001e4, 0x24126e]
    # K does not move the draws below it
    assert np.array_equal(sample_ref.uniforms(5, 1, 2, 4, 65)[:, :5], sample_ref.uniforms(5, 1, 2, 4, 5))


def test_collapse_against_brute_force():
    """All 3^6 paths over {0, 1, 2}, every blank, every length: merge runs of equal classes, then drop the blanks."""
    for blank in (0, 1, 2):
        for path in itertools.product(range(3), repeat=6):
            for lx in range(7):
                want = [c for c, _ in itertools.groupby(path[:lx]) if c != blank]
                assert sample_ref.collapse(path, lx, blank) == want, (path, lx, blank)
    hyps, lens, full = sample_ref.expected_outputs(np.array([[1, 1, 0, 1, 2, 2], [0, 0, 0, 0, 0, 0], [2, 1, 2, 1, 2, 1], [1, 1, 1, 1, 1, 1]]),
                                                   [6, 6, 4, 0], 1, 0)
    assert hyps.tolist() == [[1, 1, 2, 0, 0, 0], [0] * 6, [2, 1, 2, 1, 0, 0], [0] * 6]
    assert lens.tolist() == [3, 0, 4, 0]
    assert full.tolist() == [[1, 1, 0, 1, 2, 2], [0] * 6, [2, 1, 2, 1, -1, -1], [-1] * 6]


def test_admissible_set():
    with np.errstate(divide="ignore"):
        x = np.log(np.array([0.25, 0.0, 0.5, 0.25]))
    a = sample_ref.admissible(x, np.array([0.0, 0.2, 0.25, 0.5, 0.75 - 1e-9, 0.99]), 1e-6)
    assert a.shape == (6, 4)
    assert [np.nonzero(r)[0].tolist() for r in a] == [[0], [0], [0, 2], [2], [2, 3], [3]]       # class 1 has weight 0: never admissible
    assert not sample_ref.admissible(np.full(3, -np.inf), np.array([0.3]), 1e-6).any()


def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    for name in ("ctc_sample", "ctc_greedy"):
        assert callable(getattr(ctc_crf, name)) and getattr(ctc_crf, name) is getattr(cat_amd.ctc_crf, name)
    assert callable(core.ctc_sample) and callable(core.last_sample_kernel)
    assert "Philox4x32-10" in ctc_crf.ctc_sample.__doc__ and "argmax" in ctc_crf.ctc_greedy.__doc__


def test_workspace_bytes(core):
    ws = core._lib.crf_ctc_sample_workspace_bytes
    for B in (1, 3, 16, 256):
        for T in (1, 63, 64, 65, 1500):
            for V in (1, 72, 256, 257, 5000, 8192):
                for K in (1, 3, 4, 65):
                    w = ws(B, T, V, K)
                    assert w >= 4 * B * K * T and w % 256 == 0
                    assert ws(B + 1, T, V, K) >= w and ws(B, T + 1, V, K) >= w and ws(B, T, V, K + 1) >= w
    assert ws(16, 1500, 72, 10) == 4 * 16 * 10 * 1500                                  # (a multiple of 256 as it is)
    for bad in ((0, 10, 8, 1), (2, 0, 8, 1), (2, 10, 0, 1), (2, 10, 8, 0), (-1, 10, 8, 1), (2, 10, 8, -4)):
        assert ws(*bad) == -1 and core._lib.crf_last_error(), bad
    assert ws(1 << 20, 1 << 12, 72, 1) == -1 and b"B * T > INT32_MAX" in core._lib.crf_last_error()
    assert ws(1 << 20, 4, 72, 1 << 12) == -1 and b"B * K > INT32_MAX" in core._lib.crf_last_error()
    assert ws(2, 10, 8193, 1) == -1 and b"8192" in core._lib.crf_last_error()
    assert ws(1, (1 << 31) - 1, 8, (1 << 31) - 1) == -1 and b"too large" in core._lib.crf_last_error()


PTRS = dict(act=0x1000, lx=0x2000, hyps=0x3000, len=0x4000, paths=0x5000, ws=0x6000)


def _call(core, ptrs=None, dtype=0, time_major=0, blank=0, B=2, T=10, V=8, K=3, seed=1, offset=0, greedy=0, ws_bytes=None):
    """crf_ctc_sample with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_sample_workspace_bytes(B, T, V, K))
    rc = core._lib.crf_ctc_sample(vp(p["act"]), dtype, time_major, blank, vp(p["lx"]), B, T, V, K, seed, offset, greedy, vp(p["hyps"]),
                                  vp(p["len"]), vp(p["paths"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_argument_errors_without_gpu(core):
    for name in ("act", "lx", "hyps", "len", "ws"):
        rc, msg = _call(core, {name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for dtype in (-1, 3, 17):
        rc, msg = _call(core, dtype=dtype)
        assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _call(core, blank=blank)
        assert rc == ERR_ARG and "blank" in msg and str(blank) in msg, (blank, rc, msg)
    for kw in (dict(B=0), dict(B=-3), dict(T=0), dict(T=-1), dict(V=0), dict(K=0), dict(K=-2)):
        rc, msg = _call(core, ws_bytes=1 << 20, **kw)
        assert rc == ERR_ARG and msg, (kw, rc, msg)
    for K in (2, 3, 64):
        rc, msg = _call(core, K=K, greedy=1)
        assert rc == ERR_ARG and "greedy" in msg and str(K) in msg, (K, rc, msg)
    rc, msg = _call(core, B=1 << 20, T=1 << 12, K=1, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "B * T > INT32_MAX" in msg, (rc, msg)
    rc, msg = _call(core, B=1 << 20, T=4, K=1 << 12, ws_bytes=1 << 40)
    assert rc == ERR_ARG and "B * K > INT32_MAX" in msg, (rc, msg)
    rc, msg = _call(core, V=8193, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    need = core._lib.crf_ctc_sample_workspace_bytes(2, 10, 8, 3)
    assert need >= 4 * 2 * 3 * 10
    for short in (0, 1, need - 1):
        rc, msg = _call(core, ws_bytes=short)
        assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)


def _i32(*a):
    return torch.tensor(a, dtype=torch.int32)


def test_binding_host_checks():
    """What the binding refuses before it touches the device -- on CPU tensors: the last check of all is the device's."""
    import ctc_crf
    N, T, V = 2, 6, 5
    x, lx = torch.zeros(N, T, V), _i32(6, 4)
    for fn in (lambda **kw: ctc_crf.ctc_sample(kw.pop("x", x), kw.pop("lx", lx), kw.pop("K", 3), kw.pop("seed", 1), **kw),
               lambda **kw: ctc_crf.ctc_greedy(kw.pop("x", x), kw.pop("lx", lx), **kw)):
        with pytest.raises(RuntimeError, match="GPU"):                                 # CPU activations: there is no CPU path
            fn()
        with pytest.raises(RuntimeError, match="GPU"):
            fn(x=torch.zeros(T, N, V), time_major=True)
        for dtype in (torch.float64, torch.int32):
            with pytest.raises(RuntimeError, match=r"float32, bfloat16 or float16.*" + str(dtype).replace(".", r"\.")):
                fn(x=torch.zeros(N, T, V, dtype=dtype))
        for blank in (-1, 5, 70):
            with pytest.raises(RuntimeError, match=rf"blank must lie in \[0, V-1=4\], got {blank}"):
                fn(blank=blank)
        with pytest.raises(RuntimeError, match=r"expect 2 input lengths, got 3"):
            fn(lx=_i32(6, 4, 4))
        with pytest.raises(RuntimeError, match=r"expect 6 input lengths, got 2"):      # time-major: N is the second dimension
            fn(time_major=True)
        with pytest.raises(RuntimeError, match=r"frame lengths must lie in \[0, T=6\], got max 7"):
            fn(lx=_i32(7, 4))
        with pytest.raises(RuntimeError, match=r"got 2 dimensions"):
            fn(x=torch.zeros(T, V))
    sample = ctc_crf.ctc_sample
    for K in (0, -1):
        with pytest.raises(RuntimeError, match=rf"n_samples must be at least 1, got {K}"):
            sample(x, lx, K, 1)
    for seed in (-1, 1 << 64):
        with pytest.raises(RuntimeError, match=r"seed must lie in \[0, 2\^64\), got " + str(seed)):
            sample(x, lx, 3, seed)
    for offset in (-1, 1 << 32):
        with pytest.raises(RuntimeError, match=r"offset must lie in \[0, 2\^32\), got " + str(offset)):
            sample(x, lx, 3, 1, offset)
    with pytest.raises(RuntimeError, match="GPU"):                                     # the largest seed and offset pass the checks
        sample(x, lx, 3, (1 << 64) - 1, (1 << 32) - 1)
    with pytest.raises(RuntimeError, match=r"one path per utterance, got n_samples=2"):
        ctc_crf._C.ctc_sample(x, lx, 2, 0, greedy=True)
