"""GPU tests of the numerator's two warp-ctc options -- time-major activations and any blank column -- through every layer: the warp-ctc
C API of include/ctc.h (compute_ctc_loss) against the reference's own library (oracle/_ref/libctc_ref.so) driven by the same ctypes
prototypes, the costs and gradients against the fp64 oracle and torch's ctc_loss, time-major against batch-major bit for bit in every
numerator mode, and the Python surface (_C.gpu_ctc, WARP_CTC_LOSS(blank_label=...), CTC_CRF_LOSS's refusals)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import oracle
from tests.util import crf_env, ctc_batch as _batch, oracle_blank as _oracle_blank, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


class Opt(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("blank_label", ctypes.c_int)]


def _ref_lib_path():
    return os.path.join(os.path.dirname(oracle.__file__), "_ref", "libctc_ref.so")


def _warp_ctc(so, logits, labels, lx, ly, blank, with_grad=True):
    """compute_ctc_loss of the library `so` (ctc.h:76-109) on logits [B,T,V] handed over time-major, with a NaN-poisoned workspace
    (and, for this library, a NaN-filled gradient buffer) -> (status, costs [B] (+log p), grads [B,T,V] or None)."""
    lib = ctypes.CDLL(so)
    B, T, V = logits.shape
    ly_a, lx_a = np.ascontiguousarray(ly, dtype=np.int32), np.ascontiguousarray(lx, dtype=np.int32)
    lab_a = np.ascontiguousarray(labels, dtype=np.int32) if len(labels) else np.zeros(1, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    opt = Opt(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), int(blank))
    size = ctypes.c_size_t(0)
    lib.get_workspace_size.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, Opt, ctypes.POINTER(ctypes.c_size_t)]
    lib.get_workspace_size.restype = ctypes.c_int
    assert lib.get_workspace_size(ip(ly_a), ip(lx_a), V, B, opt, ctypes.byref(size)) == 0
    T_ = int(lx_a.max())
    act = torch.tensor(logits[:, :T_], device="cuda:0").transpose(0, 1).contiguous()      # [maxT, B, V]
    # this library promises zero rows t >= input_lengths[b] (ctc.h): its buffer starts as NaN so that the rows it skipped would show;
    # the reference's kernel leaves those rows alone (its callers zero the buffer)
    fill = 0.0 if os.path.realpath(so) == os.path.realpath(_ref_lib_path()) else float("nan")
    grads = torch.full_like(act, fill) if with_grad else None
    ws = torch.full(((size.value + 3) // 4,), float("nan"), device="cuda:0")
    costs = np.full(B, np.nan, dtype=np.float32)
    lib.compute_ctc_loss.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                     ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, Opt]
    lib.compute_ctc_loss.restype = ctypes.c_int
    torch.cuda.synchronize()
    status = lib.compute_ctc_loss(act.data_ptr(), grads.data_ptr() if with_grad else None, ip(lab_a), ip(ly_a), ip(lx_a), V, B,
                                  costs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ws.data_ptr(), opt)
    torch.cuda.synchronize()
    g = None
    if with_grad:
        g = np.zeros((B, T, V), dtype=np.float32)
        g[:, :T_] = grads.transpose(0, 1).cpu().numpy()
    return status, costs.astype(np.float64), g


def _blanks(V):
    return [0, 1, V - 1, V // 2 + 3]


@pytest.mark.parametrize("blank_i", range(4))
@pytest.mark.parametrize("case", ["ragged", "repeats", "empty_label", "no_grad"])
def test_compute_ctc_loss_vs_reference_library(crf, case, blank_i):
    """Our compute_ctc_loss against the reference's (gpu_ctc/ctc_entrypoint.cu, compiled in place by `make -C oracle ref`): both libraries in
    one process, identical prototypes and inputs, blank at 0, 1, V - 1 and in the middle."""
    if not os.path.exists(_ref_lib_path()):
        pytest.skip("oracle/_ref/libctc_ref.so not built (needs the reference tree at build time)")
    V = 40
    blank = _blanks(V)[blank_i]
    logits, labels, lx, ly = _batch(5 + blank_i, 4, 90, V, 20, blank, repeats=case == "repeats", empty=case == "empty_label")
    with_grad = case != "no_grad"
    st_r, c_r, g_r = _warp_ctc(_ref_lib_path(), logits, labels, lx, ly, blank, with_grad)
    st_o, c_o, g_o = _warp_ctc(crf._C.LIB_PATH, logits, labels, lx, ly, blank, with_grad)
    assert st_r == 0 and st_o == 0
    tol_ref = 2e-3   # (the reference cross-check's gradient tolerance below T = 300, tests/test_gpu_parity.py)
    for b in range(len(lx)):
        n = int(lx[b])
        assert abs(c_o[b] - c_r[b]) <= TOL * max(1.0, abs(c_r[b])), (b, c_o[b], c_r[b])
        if with_grad:
            assert rel_err(g_o[b, :n], g_r[b, :n]) <= tol_ref, (b, rel_err(g_o[b, :n], g_r[b, :n]))
            assert np.all(g_o[b, n:] == 0.0)


@pytest.mark.parametrize("blank_i", range(4))
def test_blank_vs_fp64_oracle_and_torch(crf, blank_i):
    """Independently of the reference library: blank k is the oracle's blank 0 with the columns k <-> 0 swapped, and torch's ctc_loss(blank=k)
    gives the same costs (its gradient has another convention: costs only)."""
    V = 40
    blank = _blanks(V)[blank_i]
    logits, labels, lx, ly = _batch(21 + blank_i, 5, 120, V, 30, blank, repeats=True, empty=True)
    g64, c64, valid = _oracle_blank(logits, labels, lx, ly, blank)
    assert all(valid)
    st, c, g = _warp_ctc(crf._C.LIB_PATH, logits, labels, lx, ly, blank)
    assert st == 0
    tl = torch.nn.functional.ctc_loss(torch.tensor(logits, dtype=torch.float64).transpose(0, 1), torch.tensor(labels, dtype=torch.long),
                                      torch.tensor(lx, dtype=torch.long), torch.tensor(ly, dtype=torch.long), blank=blank, reduction="none").numpy()
    for b in range(len(lx)):
        n = int(lx[b])
        assert abs(c[b] - c64[b]) <= TOL * max(1.0, abs(c64[b])), (b, c[b], c64[b])
        assert abs(c[b] + tl[b]) <= TOL * max(1.0, abs(tl[b])), (b, c[b], -tl[b])
        assert rel_err(g[b, :n], g64[b, :n]) <= TOL, (b, rel_err(g[b, :n], g64[b, :n]))


@pytest.mark.parametrize("mode", ["default", "robust_ctc", "no_tilt", "aux_stream"])
@pytest.mark.parametrize("blank", [0, 7])
def test_time_major_is_bitwise_batch_major(crf, mode, blank):
    """loss_fwd_bwd(time_major=True) on x.transpose(0, 1) = the batch-major call, bit for bit (costs, loss, transposed gradient), in the
    default mode, with the log-domain fallback for every utterance, with the plain (untilted) chains, and with the third stream.
    Bit for bit needs inputs whose gradient rows the grad pass sums in one order only: it adds a frame's posteriors into an LDS row with
    float atomics, and a label whose states lie in both waves that hold states (up to 63 labels: 2L + 1 <= 128) gets its addends in the
    order the waves arrive -- commutative for two addends onto 0, not for three.  So: labels of at most 60, none more than twice in an
    utterance (repeated pairs included).  A batch with labels three and more times is compared to 1e-6 of the largest entry."""
    core = crf._C
    V = 50
    logits, labels, lx, ly = _batch(31, 6, 160, V, 60, blank, empty=True, at_most_twice=True)
    x = torch.tensor(logits, device="cuda:0")
    kw = dict(default={}, robust_ctc=dict(robust_ctc=1), no_tilt=dict(ctc_tilt=0), aux_stream=dict(aux_stream=1))[mode]
    lab, lxt, lyt = torch.tensor(labels), torch.tensor(lx), torch.tensor(ly)
    with crf_env(**kw):
        l_b, g_b, e_b = core.loss_fwd_bwd(x, lab, lxt, lyt, 0.0, 0.25, None, True, blank=blank)
        l_t, g_t, e_t = core.loss_fwd_bwd(x.transpose(0, 1).contiguous(), lab, lxt, lyt, 0.0, 0.25, None, True, time_major=True, blank=blank)
        if mode == "robust_ctc":
            assert core.last_fallback_counts(torch.cuda.current_stream().cuda_stream)[1] == len(lx)
    assert g_t.shape == (x.shape[1], x.shape[0], V)
    assert torch.equal(g_t.transpose(0, 1), g_b), float((g_t.transpose(0, 1) - g_b).abs().max())
    assert torch.equal(e_t["costs_ctc"], e_b["costs_ctc"]) and torch.equal(l_t, l_b)
    g64, c64, _ = _oracle_blank(logits, labels, lx, ly, blank)
    assert np.allclose(e_b["costs_ctc"].cpu().numpy(), c64, rtol=TOL, atol=TOL)
    assert rel_err(g_b.cpu().numpy(), -0.25 * g64) <= TOL
    logits, labels, lx, ly = _batch(32, 6, 160, V // 5, 60, blank % (V // 5), repeats=True)   # (10 classes: every label many times)
    x = torch.tensor(logits, device="cuda:0")
    lab, lxt, lyt = torch.tensor(labels), torch.tensor(lx), torch.tensor(ly)
    with crf_env(**kw):
        l_b, g_b, e_b = core.loss_fwd_bwd(x, lab, lxt, lyt, 0.0, 0.25, None, True, blank=blank % (V // 5))
        l_t, g_t, e_t = core.loss_fwd_bwd(x.transpose(0, 1).contiguous(), lab, lxt, lyt, 0.0, 0.25, None, True, time_major=True, blank=blank % (V // 5))
    assert torch.equal(e_t["costs_ctc"], e_b["costs_ctc"])   # (the chains' sums have one order)
    assert float((g_t.transpose(0, 1) - g_b).abs().max()) <= 1e-6 * float(g_b.abs().max())


def test_gpu_ctc_mirror_any_blank(crf):
    """_C.gpu_ctc(probs [T,N,V], ..., blank_label) -- the pybind mirror of binding.cpp:86-117 -- with blank != 0 and in place: the same as
    compute_ctc_loss (and as the reference library's when it is built)."""
    V, blank = 40, 13
    logits, labels, lx, ly = _batch(41, 4, 100, V, 25, blank, repeats=True)
    probs = torch.tensor(logits, device="cuda:0").transpose(0, 1).contiguous()
    grads = torch.zeros_like(probs)
    costs = torch.zeros(len(lx))
    crf._C.gpu_ctc(probs, grads, torch.tensor(labels), torch.tensor(ly), torch.tensor(lx), len(lx), costs, blank)
    st, c_api, g_api = _warp_ctc(crf._C.LIB_PATH, logits, labels, lx, ly, blank)
    assert st == 0
    assert np.array_equal(costs.numpy().astype(np.float64), c_api)
    assert np.array_equal(grads.transpose(0, 1).cpu().numpy(), g_api)
    if os.path.exists(_ref_lib_path()):
        st_r, c_r, g_r = _warp_ctc(_ref_lib_path(), logits, labels, lx, ly, blank)
        assert st_r == 0
        for b in range(len(lx)):
            n = int(lx[b])
            assert abs(c_api[b] - c_r[b]) <= TOL * max(1.0, abs(c_r[b]))
            assert rel_err(g_api[b, :n], g_r[b, :n]) <= 2e-3
    with pytest.raises(AssertionError):   # minibatch_size must match probs.size(1), as before
        crf._C.gpu_ctc(probs, grads, torch.tensor(labels), torch.tensor(ly), torch.tensor(lx), len(lx) + 1, costs, blank)


@pytest.mark.parametrize("blank", [0, 1, 39])
def test_warp_ctc_loss_blank_label(crf, blank):
    """WARP_CTC_LOSS(blank_label=k): forward = -mean log p, backward = -gamma / N, against the fp64 oracle."""
    V = 40
    logits, labels, lx, ly = _batch(51, 3, 70, V, 15, blank, repeats=True)
    g64, c64, _ = _oracle_blank(logits, labels, lx, ly, blank)
    x = torch.tensor(logits, device="cuda:0", requires_grad=True)
    loss = crf.WARP_CTC_LOSS(blank_label=blank)(x, torch.tensor(labels), torch.tensor(lx), torch.tensor(ly))
    loss.backward()
    B = len(lx)
    assert abs(loss.item() + c64.sum() / B) <= TOL * abs(c64.sum() / B)
    assert rel_err(x.grad.cpu().numpy(), -g64 / B) <= TOL


def test_label_and_blank_checks(crf):
    core = crf._C
    V = 20
    logits, labels, lx, ly = _batch(61, 2, 30, V, 5, 4)
    x = torch.tensor(logits, device="cuda:0")
    lab, lxt, lyt = torch.tensor(labels), torch.tensor(lx), torch.tensor(ly)
    bad = lab.clone()
    bad[0] = 4
    with pytest.raises(RuntimeError, match="blank 4"):
        core.loss_fwd_bwd(x, bad, lxt, lyt, 0.0, 1.0, None, blank=4)
    with pytest.raises(RuntimeError, match="blank must lie"):
        core.loss_fwd_bwd(x, lab, lxt, lyt, 0.0, 1.0, None, blank=V)
    z = lab.clone()
    z[0] = 0
    with pytest.raises(RuntimeError, match=r"labels must lie in \[1, V-1=19\] \(0 is the blank\)"):   # the blank-0 message, as before
        core.loss_fwd_bwd(x, z, lxt, lyt, 0.0, 1.0, None)
    # the native entry point checks the blank itself (a caller of the C ABI has no Python in front of it)
    ws = torch.empty(core._lib.crf_workspace_bytes(None, 2, 30, V, 5), dtype=torch.uint8, device="cuda:0")
    out = torch.empty(8, device="cuda:0")
    meta = torch.zeros(16, dtype=torch.int32, device="cuda:0")
    for blank in (-1, V):
        rc = core._lib.crf_ctc_fwd_bwd(x.data_ptr(), 0, blank, meta.data_ptr(), meta.data_ptr(), meta.data_ptr(), meta.data_ptr(), 2, 30, V, 5, 1.0,
                                       torch.empty_like(x).data_ptr(), out.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 3 and "blank" in core._lib.crf_last_error().decode()


def test_ctc_crf_refuses_numerator_options(crf, golden_dir):
    """The den_lm fixes the blank at 0 and the CTC-CRF kernels read [N,T,V]: blank != 0 or time_major with a denominator is a clear error;
    CTC_CRF_LOSS itself is as before (the smoke fixture against the oracle)."""
    core = crf._C
    k = json.load(open(os.path.join(golden_dir, "kat_fixture.json")))
    fst = os.path.join(golden_dir, "den_lm_fixture.fst")
    ctx = crf.CRFContext(fst, 0)
    logits = np.log(np.array(k["probs"], dtype=np.float32))[None]
    x = torch.tensor(logits, device="cuda:0", requires_grad=True)
    lab, lx, ly = torch.tensor(k["labels"], dtype=torch.int32), torch.tensor([5], dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    loss = crf.CTC_CRF_LOSS(lamb=k["lamb"])(x, lab, lx, ly)
    loss.backward()
    ref = oracle.ctc_crf(oracle.fst_io.read_fst(fst), logits, np.array(k["labels"]), np.array([5]), np.array([3]), lamb=k["lamb"])
    assert abs(loss.item() - ref["loss"]) <= TOL * abs(ref["loss"])
    assert rel_err(x.grad.cpu().numpy(), ref["grad"]) <= TOL
    g = core.graph_for(x.device)
    for kw in (dict(blank=2), dict(time_major=True)):
        with pytest.raises(RuntimeError, match="numerator-only"):
            core.loss_fwd_bwd(x.detach(), lab, lx, ly, 1.0, 1.1, g, **kw)
    del ctx
