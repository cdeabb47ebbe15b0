"""GPU tests: time-major activations and a blank column other than 0 in EVERY numerator kernel variant, against the fp64 oracle.

The host picks the numerator's kernels from the batch's longest label sequence and from V (crf_host.hip loss_impl):
  * chains crf_ctc_pair_kernel<NR> and their log-domain fallback crf_robust_ctc_kernel<NR> (+ crf_robust_ctc_fix_kernel):
    NR = ceil((2 Lmax + 1) / 512) rounded up to 1, 2, 4, 8  -- Lmax 255 | 256, 511 | 512, 1023 | 1024, 2047;
  * the grad pass crf_grad_ctc_kernel<2 / 4 / 16> (2 Lmax + 1 <= 512 / 1024 / 4096, V <= 1024), else -- V > 1024 or the no_fast_grad
    switch -- the generic crf_grad_kernel;
  * crf_prep_kernel<16> (V <= 256) or <64>, the latter with its register path (V <= 1024) or its two passes over the row.
Each is run here in both layouts, with the blank at 0, at V - 1 and inside, on a gradient buffer filled with NaN and a workspace
filled with NaN bit patterns, so that a row a kernel skips or writes at the wrong address shows.  Also: activations of more than
2^31 elements, the C API's output contract (include/ctc.h) on poisoned outputs, and -inf activations."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from tests.util import crf_env, ctc_batch, log_softmax_np, oracle_blank, post_err, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAN = float("nan")
INVALID_VALUE = 2


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


@pytest.fixture
def poison(crf):
    """loss_fwd_bwd fills its workspace with NaN / -1 bit patterns before the call (_C.set_debug_poison)."""
    crf._C.set_debug_poison(True)
    yield
    crf._C.set_debug_poison(False)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(core, logits, labels, lx, ly, blank, time_major, switches=None):
    """loss_fwd_bwd with c_ctc = -1 (gradient = +gamma) into a NaN-filled grad_out -> (costs [B] f64, grad [B,T,V] f32, invalid [B],
    numerator fallback count).  logits [B,T,V] float32 numpy; handed over as [T,B,V] when time_major."""
    x = torch.tensor(logits, device="cuda:0")
    if time_major:
        x = x.transpose(0, 1).contiguous()
    g_out = torch.full_like(x, NAN)
    with crf_env(**(switches or {})):
        _, g, ex = core.loss_fwd_bwd(x, torch.tensor(labels), torch.tensor(lx), torch.tensor(ly), 0.0, -1.0, None, True,
                                     time_major=time_major, blank=blank, grad_out=g_out)
        nfb = core.last_fallback_counts(_stream())[1]
    assert g.data_ptr() == g_out.data_ptr()
    g = g.cpu().numpy()
    if time_major:
        g = np.ascontiguousarray(g.transpose(1, 0, 2))
    return ex["costs_ctc"].cpu().numpy().astype(np.float64), g, ex["invalid"].cpu().numpy(), nfb


def _check(costs, g, invalid, c64, g64, lx, tol_grad=TOL, what=""):
    """Costs, posteriors entry by entry, the whole gradient, the frames' sums and the rows past lx (exactly 0), utterance by utterance."""
    assert np.all(invalid == 0), (what, invalid)
    for b in range(len(lx)):
        n = int(lx[b])
        assert abs(costs[b] - c64[b]) <= TOL * max(1.0, abs(c64[b])), (what, b, costs[b], c64[b])
        assert post_err(g[b, :n], g64[b, :n]) <= TOL, (what, b, post_err(g[b, :n], g64[b, :n]))
        assert rel_err(g[b], g64[b]) <= tol_grad, (what, b, rel_err(g[b], g64[b]))
        assert np.allclose(g[b, :n].sum(-1), 1.0, rtol=0, atol=1e-4), (what, b, float(np.abs(g[b, :n].sum(-1) - 1).max()))
        assert np.all(g[b, n:] == 0.0), (what, b, "rows past lx")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the variant matrix: one ragged batch per label-length boundary
# ---------------------------------------------------------------------------------------------------------------------------------
LMAX = [255, 256, 511, 512, 1023, 1024, 2047]
V_MATRIX = 72
MODES = {"default": {}, "robust_ctc": dict(robust_ctc=1), "no_tilt": dict(ctc_tilt=0), "no_fast_grad": dict(no_fast_grad=1),
         "aux_stream": dict(aux_stream=1)}
_CACHE = {}


def _variant_batch(Lmax, blank):
    """A long utterance at Lmax over T = 2 Lmax + 60 frames, a short one with repeated labels, a short one without; labels avoid the
    blank (label 0 is an ordinary label when blank != 0).  -> (logits [3,T,V], labels, lx, ly, +gamma [3,T,V], +log p [3]), cached."""
    key = (Lmax, blank)
    if key not in _CACHE:
        V = V_MATRIX
        rng = np.random.default_rng(1000 + Lmax + 7 * blank)
        T = 2 * Lmax + 60
        lx = np.array([T, T // 3, T // 5], dtype=np.int32)
        ly = np.array([Lmax, min(40, Lmax // 8), 7], dtype=np.int32)
        pool = np.array([v for v in range(V) if v != blank])
        lab = [pool[rng.integers(0, len(pool), size=int(ly[0]))],
               np.repeat(pool[rng.integers(0, len(pool), size=(int(ly[1]) + 2) // 3)], 3)[:int(ly[1])],   # runs of three: repeats
               pool[rng.integers(0, len(pool), size=int(ly[2]))]]
        labels = np.concatenate(lab).astype(np.int32)
        logits = log_softmax_np(rng.normal(0.0, 1.5, size=(3, T, V))).astype(np.float32)
        g64, c64, valid = oracle_blank(logits, labels, lx, ly, blank)
        assert valid.all() and np.isfinite(c64).all()
        _CACHE[key] = (logits, labels, lx, ly, g64, c64)
    return _CACHE[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("blank", [0, V_MATRIX - 1, V_MATRIX // 2 + 3])
@pytest.mark.parametrize("Lmax", LMAX)
def test_numerator_variant_matrix(crf, poison, Lmax, blank, mode):
    """Every chain / fallback / grad instantiation the label length selects, in both layouts, with the blank at 0, V - 1 and inside:
    against the fp64 oracle, and time-major against batch-major (costs bit for bit: the chains' sums have one order; the gradient to 1e-6
    of its largest entry: the grad pass adds a frame's posteriors with float atomics)."""
    logits, labels, lx, ly, g64, c64 = _variant_batch(Lmax, blank)
    T = logits.shape[1]
    tol = 5e-4 if T >= 3000 else TOL      # (test_gpu_parity.py::test_ctc_label_length_variants' bound at these lengths)
    out = {}
    for tm in (False, True):
        costs, g, inv, nfb = _run(crf._C, logits, labels, lx, ly, blank, tm, MODES[mode])
        if mode == "robust_ctc":
            assert nfb == len(lx), nfb        # every utterance through the log-domain chains and the fix kernel
        _check(costs, g, inv, c64, g64, lx, tol, what=(mode, "time-major" if tm else "batch-major"))
        out[tm] = (costs, g)
    assert np.array_equal(out[True][0], out[False][0])
    assert np.abs(out[True][1] - out[False][1]).max() <= 1e-6 * np.abs(out[False][1]).max()


def test_forced_robust_numerator_only(crf, poison):
    """The `robust` switch (every utterance through the fallbacks) on a numerator-only call takes the numerator's log-domain chains, never
    crf_robust_grad_kernel -- the denominator's fallback, which reads batch-major rows and column 0: time-major, blank inside."""
    logits, labels, lx, ly, g64, c64 = _variant_batch(511, V_MATRIX // 2 + 3)
    for tm in (True, False):
        costs, g, inv, nfb = _run(crf._C, logits, labels, lx, ly, V_MATRIX // 2 + 3, tm, dict(robust=1))
        assert nfb == len(lx)
        _check(costs, g, inv, c64, g64, lx, what=("robust", tm))
        assert crf._C.last_fallback_counts(_stream())[0] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. vocabulary boundaries and activations beyond 2^31 elements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank_at_end", [False, True])
@pytest.mark.parametrize("V", [37, 256, 257, 1024, 1025, 5000, 8192])
def test_vocabulary_boundaries(crf, poison, V, blank_at_end):
    """crf_prep_kernel<16> (V <= 256) and <64> (register path to 1024, two passes beyond), crf_grad_ctc_kernel (V <= 1024) and the generic
    crf_grad_kernel (V > 1024), both layouts, blank 0 and V - 1."""
    blank = V - 1 if blank_at_end else 0
    logits, labels, lx, ly = ctc_batch(77 + V, 3, 100, V, 40, blank, repeats=True)
    g64, c64, valid = oracle_blank(logits, labels, lx, ly, blank)
    assert valid.all()
    out = {}
    for tm in (False, True):
        costs, g, inv, _ = _run(crf._C, logits, labels, lx, ly, blank, tm)
        _check(costs, g, inv, c64, g64, lx, what=(V, blank, tm))
        out[tm] = (costs, g)
    assert np.array_equal(out[True][0], out[False][0])
    assert np.abs(out[True][1] - out[False][1]).max() <= 1e-6 * np.abs(out[False][1]).max()


def test_vocabulary_over_the_limit_is_refused(crf):
    V = 8193
    x = torch.zeros(2, 6, V, device="cuda:0").log_softmax(-1)
    args = (torch.tensor([1, 2], dtype=torch.int32), torch.tensor([6, 5], dtype=torch.int32), torch.tensor([1, 1], dtype=torch.int32))
    for tm in (False, True):
        with pytest.raises(RuntimeError, match="V > 8192"):
            crf._C.loss_fwd_bwd(x.transpose(0, 1).contiguous() if tm else x, args[0], args[1], args[2], 0.0, -1.0, None, True, time_major=tm)
    st, _, _ = _api(crf, x.transpose(0, 1).contiguous(), np.array([1, 2]), np.array([1, 1]), np.array([6, 5]), V, 0)
    assert st == INVALID_VALUE


class Opt(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("blank_label", ctypes.c_int)]


def _capi(so):
    lib = ctypes.CDLL(so)
    ip = ctypes.POINTER(ctypes.c_int)
    lib.get_workspace_size.argtypes = [ip, ip, ctypes.c_int, ctypes.c_int, Opt, ctypes.POINTER(ctypes.c_size_t)]
    lib.get_workspace_size.restype = ctypes.c_int
    lib.compute_ctc_loss.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ip, ip, ip, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                     ctypes.c_void_p, Opt]
    lib.compute_ctc_loss.restype = ctypes.c_int
    return lib


def _api(crf, act, labels, ly, lx, V, blank, grads=True, stream=None, so=None, sync=True):
    """compute_ctc_loss on the time-major activations `act` (a CUDA tensor, [maxT, B, V] or longer) with a NaN-filled gradient buffer (zeros
    for the reference's library) and a NaN-filled workspace, both made on `stream` -> (status, costs [B] as float64 (NaN-initialised host memory), grads tensor or None)."""
    lib = _capi(so or crf._C.LIB_PATH)
    B = len(lx)
    ly_a, lx_a = np.ascontiguousarray(ly, dtype=np.int32), np.ascontiguousarray(lx, dtype=np.int32)
    lab_a = np.ascontiguousarray(labels, dtype=np.int32) if len(labels) else np.zeros(1, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    st = stream or torch.cuda.current_stream()
    opt = Opt(ctypes.c_void_p(st.cuda_stream), int(blank))
    size = ctypes.c_size_t(0)
    rc = lib.get_workspace_size(ip(ly_a), ip(lx_a), V, B, opt, ctypes.byref(size))
    if rc != 0:
        return rc, None, None
    # (the reference's kernel leaves the rows past input_lengths alone: its callers zero the buffer)
    fill = 0.0 if so is not None and os.path.realpath(so) == os.path.realpath(_ref_lib_path()) else NAN
    with torch.cuda.stream(st):
        g = torch.full_like(act, fill) if grads else None
        ws = torch.full(((size.value + 3) // 4,), NAN, device=act.device)
    costs = np.full(B, np.nan, dtype=np.float32)
    rc = lib.compute_ctc_loss(act.data_ptr(), g.data_ptr() if grads else None, ip(lab_a), ip(ly_a), ip(lx_a), V, B,
                              costs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ws.data_ptr(), opt)
    if sync:
        st.synchronize()
    del ws
    return rc, costs.astype(np.float64), g


def _gather_check(g, time_major, cols, lx, ref_g, what):
    """Large case: utterance b's columns cols[b] of the gradient g (a CUDA tensor, [B,T,V] or [T,B,V]) against the oracle's ref_g[b]
    ([T, 1 + U]), its frames' sums, then those columns set to 0 in place -- after which every entry of g must be exactly 0 (every other
    column, every row past lx: the buffer started as NaN)."""
    B = len(lx)
    for b in range(B):
        n = int(lx[b])
        gb = g[:, b] if time_major else g[b]
        c = torch.tensor(cols[b], device=g.device)
        sub = gb[:n].index_select(1, c).cpu().numpy()
        r = ref_g[b, :n, :len(cols[b])]
        assert post_err(sub, r) <= TOL, (what, b, post_err(sub, r))
        assert rel_err(sub, r) <= TOL, (what, b, rel_err(sub, r))
        s = gb[:n].double().sum(-1).cpu().numpy()
        assert np.allclose(s, 1.0, rtol=0, atol=1e-4), (what, b, float(np.abs(s - 1).max()))
        gb[:n].index_fill_(1, c, 0.0)
    nz = sum(int(torch.count_nonzero(g[i:i + 8])) for i in range(0, g.shape[0], 8))
    assert nz == 0, (what, nz, "entries outside the utterances' blank and label columns (or past lx) are not 0")


def test_activations_beyond_2_31_elements(crf, poison):
    """B = 128, T = 3400, V = 5000: 2.18e9 floats, so the last utterances' rows (batch-major) and the last frames' rows (time-major) lie
    beyond 2^31 elements -- 64-bit row addresses in prep (two passes), the chains, the generic grad kernel.  The reference is the fp64
    oracle on each utterance's blank and label columns alone (CTC reads no other column)."""
    B, T, V = 128, 3400, 5000
    assert B * T * V > 2 ** 31
    if torch.cuda.mem_get_info()[0] < 48 * 2 ** 30:
        pytest.skip("needs 48 GB of free device memory")
    blank = V - 1
    rng = np.random.default_rng(2031)
    lx = np.array([T - (b * 37) % 500 for b in range(B)], dtype=np.int32)
    lx[-1] = T                                           # (the last utterance's rows are the last of the batch-major tensor)
    ly = rng.integers(20, 61, size=B).astype(np.int32)
    labs, cols, rel = [], [], []
    for b in range(B):
        x = rng.integers(0, V - 1, size=int(ly[b]))
        x[-3:] = V - 2 - rng.integers(0, 4, size=3)      # labels at the end of the row
        if b % 3 == 0:
            x[1] = x[0]                                  # a repeat
        labs.append(x)
        u = np.unique(x)
        cols.append(np.concatenate([[blank], u]).astype(np.int64))
        rel.append((np.searchsorted(u, x) + 1).astype(np.int32))
    labels = np.concatenate(labs).astype(np.int32)
    # the reference: [B, T, 1 + max U] gathered log-probs (column 0 = the blank), labels renamed to 1..U
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(2031)
    x = torch.empty(B, T, V, device="cuda:0")
    for b0 in range(0, B, 8):
        x[b0:b0 + 8].normal_(0.0, 1.5, generator=gen)
        x[b0:b0 + 8] = torch.log_softmax(x[b0:b0 + 8], -1)
    U = max(len(c) for c in cols)
    sub = np.zeros((B, T, U), dtype=np.float32)
    for b in range(B):
        sub[b, :lx[b], :len(cols[b])] = x[b, :int(lx[b])].index_select(1, torch.tensor(cols[b], device="cuda:0")).cpu().numpy()
    g64, c64, valid = oracle.ctc(sub, np.concatenate(rel), lx, ly)
    assert valid.all() and np.isfinite(c64).all()
    del sub
    lab_t, lx_t, ly_t = torch.tensor(labels), torch.tensor(lx), torch.tensor(ly)
    core = crf._C
    costs = {}
    for tm in (False, True):
        if tm:
            x = x.transpose(0, 1).contiguous()
            torch.cuda.empty_cache()
        g = torch.full_like(x, NAN)
        _, g, ex = core.loss_fwd_bwd(x, lab_t, lx_t, ly_t, 0.0, -1.0, None, True, time_major=tm, blank=blank, grad_out=g)
        costs[tm] = ex["costs_ctc"].cpu().numpy().astype(np.float64)
        assert int(ex["invalid"].sum()) == 0
        assert np.allclose(costs[tm], c64, rtol=TOL, atol=0), float(np.abs(costs[tm] / c64 - 1).max())
        _gather_check(g, tm, cols, lx, g64, "time-major" if tm else "batch-major")
        del g, ex
        torch.cuda.empty_cache()
    assert np.array_equal(costs[True], costs[False])
    # the C API at this shape: get_workspace_size, compute_ctc_loss (workspace with its spare gradient buffer)
    st, c_api, g = _api(crf, x, labels, ly, lx, V, blank)
    assert st == 0
    assert np.array_equal(c_api, costs[True])
    _gather_check(g, True, cols, lx, g64, "compute_ctc_loss")
    del g, x
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the C API's output contract (include/ctc.h), on NaN-filled gradients and workspace
# ---------------------------------------------------------------------------------------------------------------------------------
def _tm(logits, T=None):
    """[B,T,V] numpy -> time-major CUDA tensor, the first T frames (default: max)."""
    return torch.tensor(np.ascontiguousarray(logits[:, :T].transpose(1, 0, 2)), device="cuda:0")


def _bm(g):
    return g.transpose(0, 1).cpu().numpy()


def _api_vs_oracle(crf, logits, labels, lx, ly, blank, valid_expected=None):
    B, T, V = logits.shape
    Tm = max(1, int(np.max(lx)))
    st, c, g = _api(crf, _tm(logits, Tm), labels, ly, lx, V, blank)
    assert st == 0
    g64, c64, valid = oracle_blank(logits, labels, lx, ly, blank)
    if valid_expected is not None:
        assert list(valid) == list(valid_expected)
    g = _bm(g)
    for b in range(B):
        n = int(lx[b])
        assert abs(c[b] - c64[b]) <= TOL * max(1.0, abs(c64[b])), (b, c[b], c64[b])
        assert np.all(g[b, n:] == 0.0), (b, "rows past input_lengths")
        if not valid[b]:
            assert c[b] == 0.0 and np.all(g[b] == 0.0), (b, "an unalignable utterance: cost 0, zero rows")
        elif n:
            assert rel_err(g[b, :n], g64[b, :n, ]) <= TOL, (b, rel_err(g[b, :n], g64[b, :n]))
    return c, g, c64


def test_api_unalignable_utterance(crf):
    V, blank = 30, 5
    logits, labels, lx, ly = ctc_batch(301, 4, 40, V, 12, blank)
    lab = np.split(labels, np.cumsum(ly)[:-1])
    lx[1], ly[1] = 10, 8
    lab[1] = np.array([1, 1, 2, 2, 3, 3, 4, 6])         # 8 labels + 4 repeats > 10 frames
    _api_vs_oracle(crf, logits, np.concatenate(lab).astype(np.int32), lx, ly, blank, valid_expected=[1, 0, 1, 1])


def test_api_zero_input_lengths(crf):
    """input_lengths[b] = 0 inside the batch, with and without labels (the latter has no alignment: cost 0)."""
    V, blank = 30, 11
    logits, labels, lx, ly = ctc_batch(302, 5, 30, V, 6, blank)
    lab = np.split(labels, np.cumsum(ly)[:-1])
    lx[1], ly[1], lab[1] = 0, 0, lab[1][:0]
    lx[3] = 0
    c, _, _ = _api_vs_oracle(crf, logits, np.concatenate(lab).astype(np.int32), lx, ly, blank, valid_expected=[1, 1, 1, 0, 1])
    assert c[1] == 0.0 and c[3] == 0.0


def test_api_empty_label_any_blank(crf):
    """L = 0 with blank != 0: the only path is the blank at every frame, cost = the sum of the blank column."""
    V, blank = 25, 17
    logits, labels, lx, ly = ctc_batch(303, 3, 50, V, 9, blank)
    lab = np.split(labels, np.cumsum(ly)[:-1])
    ly[0], lab[0] = 0, lab[0][:0]
    c, _, _ = _api_vs_oracle(crf, logits, np.concatenate(lab).astype(np.int32), lx, ly, blank)
    want = float(logits[0, :lx[0], blank].astype(np.float64).sum())
    assert abs(c[0] - want) <= TOL * abs(want)


def test_api_all_input_lengths_zero(crf):
    """No frames at all: the early return (nothing launched), every cost 0, the gradient buffer untouched."""
    V = 20
    act = torch.zeros(1, 3, V, device="cuda:0")
    st, c, g = _api(crf, act, np.array([3, 4], dtype=np.int32), np.array([0, 2, 0]), np.array([0, 0, 0]), V, 7)
    assert st == 0 and np.all(c == 0.0)
    assert torch.isnan(g).all()


@pytest.mark.parametrize("B", [1, 300])
def test_api_minibatch_sizes(crf, B):
    """One utterance, and 300 (2 B chain workgroups exceed the CU count) on short utterances."""
    V, blank = 20, 19
    logits, labels, lx, ly = ctc_batch(304 + B, B, 24 if B > 1 else 120, V, 6 if B > 1 else 40, blank, repeats=True)
    _api_vs_oracle(crf, logits, labels, lx, ly, blank)


def test_api_without_gradients_generic_grad_kernel(crf):
    """gradients = NULL at V = 2000 (the generic grad kernel writes the workspace's spare buffer): costs as with gradients."""
    V, blank = 2000, 1234
    logits, labels, lx, ly = ctc_batch(305, 3, 60, V, 15, blank, repeats=True)
    st, c, g = _api(crf, _tm(logits), labels, ly, lx, V, blank, grads=False)
    assert st == 0 and g is None
    _, c64, valid = oracle_blank(logits, labels, lx, ly, blank)
    assert valid.all()
    assert np.allclose(c, c64, rtol=TOL, atol=0)
    st, c2, _ = _api(crf, _tm(logits), labels, ly, lx, V, blank)
    assert st == 0 and np.array_equal(c, c2)


def test_gpu_ctc_padded_frames(crf):
    """_C.gpu_ctc with probs [T_pad, N, V], T_pad > max(sizes): the padded rows of grads come back 0 (grads starts as NaN)."""
    V, blank = 40, 9
    logits, labels, lx, ly = ctc_batch(306, 4, 80, V, 12, blank, repeats=True)
    lx = lx - 10                                         # every utterance ends at least 10 frames before the tensor
    probs = _tm(logits)
    grads = torch.full_like(probs, NAN)
    costs = torch.full((len(lx),), NAN)
    crf._C.gpu_ctc(probs, grads, torch.tensor(labels), torch.tensor(ly), torch.tensor(lx), len(lx), costs, blank)
    g64, c64, valid = oracle_blank(logits, labels, lx, ly, blank)
    assert valid.all()
    g = _bm(grads)
    assert np.allclose(costs.numpy(), c64, rtol=TOL, atol=0)
    for b in range(len(lx)):
        n = int(lx[b])
        assert np.all(g[b, n:] == 0.0), b
        assert rel_err(g[b, :n], g64[b, :n]) <= TOL


def test_api_on_a_side_stream(crf):
    """options.stream = a non-default stream that produced the activations (behind a busy wait) and made the buffers: the call works in
    that stream's order and its costs are ready when it returns (one sync), without any synchronisation by the caller."""
    V, blank = 50, 3
    logits, labels, lx, ly = ctc_batch(307, 4, 200, V, 40, blank, repeats=True)
    g64, c64, _ = oracle_blank(logits, labels, lx, ly, blank)
    src = _tm(logits)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(50_000_000)                       # (some ms of busy wait in front of the producer)
        act = src.clone()
        st, c, g = _api(crf, act, labels, ly, lx, V, blank, stream=s, sync=False)
        assert st == 0
        assert np.allclose(c, c64, rtol=TOL, atol=0), (c, c64)   # ready on return
        g = _bm(g)
    for b in range(len(lx)):
        n = int(lx[b])
        assert rel_err(g[b, :n], g64[b, :n]) <= TOL and np.all(g[b, n:] == 0.0)


def _ref_lib_path():
    return os.path.join(os.path.dirname(oracle.__file__), "_ref", "libctc_ref.so")


@pytest.mark.parametrize("Lmax", [300, 600])
def test_api_vs_reference_library_long_labels(crf, Lmax):
    """compute_ctc_loss against the reference's own library at label lengths beyond this suite's other cross-checks (its kernels stop at
    2 L + 1 <= 1280), blank inside, time-major; ours also against the fp64 oracle."""
    if not os.path.exists(_ref_lib_path()):
        pytest.skip("oracle/_ref/libctc_ref.so not built (needs the reference tree at build time)")
    V, blank = 60, 31
    logits, labels, lx, ly = ctc_batch(400 + Lmax, 3, 2 * Lmax + 60, V, Lmax, blank, repeats=True)
    st_r, c_ref, gr = _api(crf, _tm(logits), labels, ly, lx, V, blank, so=_ref_lib_path())
    assert st_r == 0
    c, g, c64 = _api_vs_oracle(crf, logits, labels, lx, ly, blank)
    gr = _bm(gr)
    for b in range(len(lx)):
        n = int(lx[b])
        assert abs(c[b] - c_ref[b]) <= TOL * abs(c_ref[b]), (b, c[b], c_ref[b])
        # (the reference's fp32 log-domain gradient drifts with T: test_gpu_parity.py::test_numerator_vs_reference_kernels' bounds; measured
        #  2.4e-3 at T = 660 and 6.6e-3 at T = 1 260 here, while ours is held to 1e-4 of the fp64 oracle above)
        tol_ref = 3e-2 if n >= 1000 else 6e-3 if n >= 300 else 2e-3
        assert rel_err(g[b, :n], gr[b, :n]) <= tol_ref, (b, rel_err(g[b, :n], gr[b, :n]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. -inf activations (a masked vocabulary)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "robust_ctc", "no_fast_grad"])
def test_masked_vocabulary(crf, poison, mode):
    """-inf in whole columns no label uses, and in the blank's column at some frames (the frames where a path must sit on a label:
    label-to-label transitions), both layouts, against the oracle."""
    V, blank = 40, 6
    rng = np.random.default_rng(501)
    B, T = 3, 150
    lx = np.array([150, 120, 90], dtype=np.int32)
    ly = np.array([30, 20, 12], dtype=np.int32)
    used = np.array([v for v in range(0, V, 2) if v != blank])     # the odd columns are masked
    labels = used[rng.integers(0, len(used), size=int(ly.sum()))].astype(np.int32)
    raw = rng.normal(0.0, 1.5, size=(B, T, V))
    raw[:, :, 1::2] = -np.inf
    raw[:, 0, blank] = -np.inf                                     # the first frame must be a label
    raw[:, 3::7, blank] = -np.inf
    logits = log_softmax_np(raw).astype(np.float32)
    assert np.isneginf(logits).any()
    g64, c64, valid = oracle_blank(logits, labels, lx, ly, blank)
    assert valid.all() and np.isfinite(c64).all()
    out = {}
    for tm in (False, True):
        costs, g, inv, _ = _run(crf._C, logits, labels, lx, ly, blank, tm, MODES[mode])
        assert np.isfinite(g).all()
        _check(costs, g, inv, c64, g64, lx, what=(mode, tm))
        assert np.all(g[:, :, 1::2] == 0.0)
        out[tm] = costs
    assert np.array_equal(out[True], out[False])


@pytest.mark.parametrize("time_major", [False, True])
def test_zero_probability_utterance(crf, poison, time_major):
    """An utterance whose only label column is -inf at every frame has probability 0: cost -inf (the fp64 oracle's value), zero gradient
    rows, not invalid; the utterances beside it are unaffected -- costs bit for bit those of the same batch without the -inf column (same
    Lmax: the same kernels), gradients to 1e-6 of the largest entry."""
    V, blank = 30, 29
    logits, labels, lx, ly = ctc_batch(502, 4, 90, V, 25, blank, repeats=True)
    lab = np.split(labels, np.cumsum(ly)[:-1])
    c = 4
    ly[1], lab[1] = 3, np.array([c, c, c])                 # (labels c c c: needs 5 frames)
    labels = np.concatenate(lab).astype(np.int32)
    masked = logits.copy()
    masked[1, :, c] = -np.inf
    g64, c64, valid = oracle_blank(masked, labels, lx, ly, blank)
    assert valid.all() and c64[1] == -np.inf and np.all(g64[1] == 0.0)
    costs, g, inv, _ = _run(crf._C, masked, labels, lx, ly, blank, time_major)
    costs0, g0, inv0, _ = _run(crf._C, logits, labels, lx, ly, blank, time_major)
    assert np.all(inv == 0) and np.all(inv0 == 0)
    assert costs[1] == -np.inf, costs[1]
    assert np.all(g[1] == 0.0)
    keep = [0, 2, 3]
    assert np.array_equal(costs[keep], costs0[keep])
    assert np.abs(g[keep] - g0[keep]).max() <= 1e-6 * np.abs(g0[keep]).max()
    for b in keep:
        assert abs(costs[b] - c64[b]) <= TOL * abs(c64[b])
        assert rel_err(g[b], g64[b]) <= TOL
    # the C API's cost for it as well
    st, c_api, g_api = _api(crf, _tm(masked), labels, ly, lx, V, blank)
    assert st == 0 and c_api[1] == -np.inf and bool((g_api[:, 1] == 0).all())
