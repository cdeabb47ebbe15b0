"""GPU tests: plain CTC on the RAW network output (fp32 / bf16 / fp16) in either layout and with any blank -- crf_ctc_fwd_bwd_logits through
_C.loss_fwd_bwd(fused=True, c_den=0) and WARP_CTC_LOSS(fuse_log_softmax=True, time_major=..., blank_label=...) -- against the fp64 oracle on
log_softmax of the UPCAST ROUNDED input, and against torch's ctc_loss with autograd through log_softmax.

The kernels of the fused path are those of tests/test_gpu_ctc_variants.py (its header lists how the host picks them): crf_prep_kernel<16 / 64>,
crf_ctc_pair_kernel<NR> with its 16-bit branch, crf_grad_ctc_kernel<REGS>, the generic crf_grad_kernel and the crf_robust_ctc_* fallbacks.
Every call writes into a NaN-filled gradient buffer on a workspace of NaN bit patterns, in both layouts."""
import numpy as np
import pytest
import torch

from tests.util import crf_env, log_softmax_np, oracle_blank, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAN = float("nan")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
V_MATRIX = 72
MODES = {"default": {}, "robust_ctc": dict(robust_ctc=1), "no_fast_grad": dict(no_fast_grad=1)}
_CACHE = {}


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


@pytest.fixture
def poison(crf):
    crf._C.set_debug_poison(True)
    yield
    crf._C.set_debug_poison(False)


def softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.exp(x - m)
    return e / e.sum(-1, keepdims=True)


def reference(xr, labels, lx, ly, blank):
    """xr: [B,T,V] raw values already rounded to the dtype (a CPU tensor of that dtype).  -> (x^ float32 numpy, d/dx of +sum_b log p_b in
    fp64 = gamma - softmax(x^) for t < lx of the valid utterances and 0 elsewhere, +log p [B], valid [B])."""
    xh = xr.float().numpy()
    g64, c64, valid = oracle_blank(log_softmax_np(xh.astype(np.float64)), labels, lx, ly, blank)
    ref = np.zeros_like(g64)
    for b in range(len(lx)):
        n = int(lx[b])
        if valid[b] and np.isfinite(c64[b]):
            ref[b, :n] = g64[b, :n] - softmax64(xh[b, :n])
    return xh, ref, c64, valid


def make_batch(Lmax, V, blank, dtype, seed):
    """The batch of tests/test_gpu_ctc_variants.py::_variant_batch on N(0, 2^2) raw values rounded to `dtype`: a long utterance at Lmax over
    T = 2 Lmax + 60 frames, a short one with repeated labels, a short one without.  Cached with its reference."""
    key = (Lmax, V, blank, dtype)
    if key not in _CACHE:
        rng = np.random.default_rng(seed + Lmax + 7 * blank + 13 * V)
        T = 2 * Lmax + 60
        lx = np.array([T, T // 3, T // 5], dtype=np.int32)
        ly = np.array([Lmax, max(1, min(40, Lmax // 8)), min(7, Lmax)], dtype=np.int32)
        pool = np.array([v for v in range(V) if v != blank])
        lab = [pool[rng.integers(0, len(pool), size=int(ly[0]))],
               np.repeat(pool[rng.integers(0, len(pool), size=(int(ly[1]) + 2) // 3)], 3)[:int(ly[1])],
               pool[rng.integers(0, len(pool), size=int(ly[2]))]]
        labels = np.concatenate(lab).astype(np.int32)
        xr = torch.tensor(rng.normal(0.0, 2.0, size=(3, T, V)), dtype=torch.float32).to(DTYPES[dtype])
        xh, ref, c64, valid = reference(xr, labels, lx, ly, blank)
        assert valid.all() and np.isfinite(c64).all()
        _CACHE[key] = (xr, labels, lx, ly, ref, c64)
    return _CACHE[key]


def run(core, xr, labels, lx, ly, blank, time_major, switches=None):
    """_C.loss_fwd_bwd(fused=True, c_den=0, c_ctc=-1) into a NaN-filled fp32 grad_out -> (costs [B] f64, grad [B,T,V] f32, invalid [B],
    numerator fallback count).  xr [B,T,V] of its dtype on the CPU; handed over as [T,B,V] when time_major."""
    x = xr.to("cuda:0")
    if time_major:
        x = x.transpose(0, 1).contiguous()
    g_out = torch.full(x.shape, NAN, dtype=torch.float32, device="cuda:0")
    with crf_env(**(switches or {})):
        _, g, ex = core.loss_fwd_bwd(x, torch.tensor(labels), torch.tensor(lx), torch.tensor(ly), 0.0, -1.0, None, True, fused=True,
                                     time_major=time_major, blank=blank, grad_out=g_out)
        nfb = core.last_fallback_counts(torch.cuda.current_stream().cuda_stream)[1]
    assert g.data_ptr() == g_out.data_ptr() and g.dtype == torch.float32
    g = g.cpu().numpy()
    if time_major:
        g = np.ascontiguousarray(g.transpose(1, 0, 2))
    return ex["costs_ctc"].cpu().numpy().astype(np.float64), g, ex["invalid"].cpu().numpy(), nfb


def check(costs, g, ref, c64, lx, what, valid=None):
    """The bounds of tests/test_gpu_ctc_variants.py::_check on costs and on the gradient (TOL: the C-level gradient is fp32 in every input
    dtype), every frame's gradient sums to 0 within 1e-5 (tests/test_gpu_parity.py::test_fused_log_softmax's bound), rows past lx exactly 0."""
    assert not np.isnan(g).any(), (what, "a row was not written")
    for b in range(len(lx)):
        n = int(lx[b])
        if valid is not None and not valid[b]:
            assert np.all(g[b] == 0.0), (what, b, "gradient of an invalid utterance")
            continue
        err_c, err_g, err_s = abs(costs[b] - c64[b]), rel_err(g[b], ref[b]), float(np.abs(g[b].sum(-1)).max())
        print(what, "utterance", b, "cost err", err_c, "grad rel_err", err_g, "frame sum", err_s)
        assert err_c <= TOL * max(1.0, abs(c64[b])), (what, b, costs[b], c64[b])
        assert err_g <= TOL, (what, b, err_g)
        assert err_s <= 1e-5, (what, b, err_s)
        assert np.all(g[b, n:] == 0.0), (what, b, "rows past lx")


def both_layouts(crf, batch, blank, switches=None, what=(), fallback=False, valid=None):
    xr, labels, lx, ly, ref, c64 = batch
    out = {}
    for tm in (False, True):
        costs, g, inv, nfb = run(crf._C, xr, labels, lx, ly, blank, tm, switches)
        if fallback:
            assert nfb == len(lx), nfb            # every utterance through the log-domain chains and the fix kernel
        assert np.array_equal(inv, np.zeros(len(lx)) if valid is None else 1 - np.asarray(valid)), (what, tm, inv)
        check(costs, g, ref, c64, lx, what + ("time-major" if tm else "batch-major",), valid)
        out[tm] = costs
    assert np.array_equal(out[True], out[False]), (what, "costs differ between the layouts", out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. C level: dtype x layout x blank x chain instantiation x mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("blank", [0, V_MATRIX - 1, V_MATRIX // 2 + 3])
@pytest.mark.parametrize("Lmax", [255, 256, 512, 1024])
def test_fused_numerator_matrix(crf, poison, Lmax, blank, dtype, mode):
    """One label length per chain instantiation (NR = 1, 2, 4, 8; grad kernel REGS 2, 4, 16), the blank at 0, V - 1 and inside, both
    layouts, in the modes default, robust_ctc (every utterance through the fallback) and no_fast_grad (the generic grad kernel)."""
    both_layouts(crf, make_batch(Lmax, V_MATRIX, blank, dtype, 3000), blank, MODES[mode], (Lmax, blank, dtype, mode), fallback=mode == "robust_ctc")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("V", [37, 257, 1025])
def test_fused_vocabulary_paths(crf, poison, V, dtype):
    """Lmax = 7: rows of 16-bit elements on odd offsets (odd V), crf_prep_kernel<16>, <64> with its register path and with its two passes,
    the generic grad kernel for V > 1024; blank at 0, V - 1 and inside."""
    for blank in (0, V - 1, V // 2):
        both_layouts(crf, make_batch(7, V, blank, dtype, 4000), blank, None, (V, blank, dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_fused_invalid_and_empty(crf, poison, dtype):
    """An utterance with L + repeats > lx (invalid: cost 0, gradient exactly 0, flagged) and an empty transcript in one batch."""
    V, blank, T = 23, 5, 40
    rng = np.random.default_rng(61)
    lab = [np.array([1, 1, 2, 2, 3]), np.array([], dtype=np.int64), np.array([7, 8, 8, 9]), np.array([4, 0, 6])]
    lx = np.array([6, 33, T, 17], dtype=np.int32)                 # 0: needs 7 frames
    ly = np.array([len(a) for a in lab], dtype=np.int32)
    labels = np.concatenate(lab).astype(np.int32)
    xr = torch.tensor(rng.normal(0.0, 2.0, size=(4, T, V)), dtype=torch.float32).to(DTYPES[dtype])
    xh, ref, c64, valid = reference(xr, labels, lx, ly, blank)
    assert valid.tolist() == [0, 1, 1, 1]
    c64 = np.where(valid.astype(bool), c64, 0.0)
    both_layouts(crf, (xr, labels, lx, ly, ref, c64), blank, None, ("invalid+empty", dtype), valid=valid)
    costs, _, _, _ = run(crf._C, xr, labels, lx, ly, blank, False)
    assert costs[0] == 0.0


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_fused_masked_class(crf, poison, dtype):
    """A column of -inf raw values that no label uses: its softmax and its gradient are 0, everything else as without it."""
    V, blank, masked = 37, 36, 11
    xr0, labels, lx, ly, _, _ = make_batch(7, V, blank, dtype, 4000)
    labels = np.where(labels == masked, masked + 1, labels).astype(np.int32)
    xr = xr0.clone()
    xr[:, :, masked] = -float("inf")
    xh, ref, c64, valid = reference(xr, labels, lx, ly, blank)
    assert valid.all() and np.isfinite(c64).all()
    both_layouts(crf, (xr, labels, lx, ly, ref, c64), blank, None, ("masked", dtype))
    _, g, _, _ = run(crf._C, xr, labels, lx, ly, blank, True)
    assert np.all(g[:, :, masked] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. Python level: WARP_CTC_LOSS against torch's ctc_loss with autograd through log_softmax
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("tm", [False, True])
@pytest.mark.parametrize("bl", [0, 36, 17])
def test_warp_ctc_loss_fused_against_torch(crf, poison, dtype, tm, bl):
    V = 37
    xr, labels, lx, ly, _, _ = make_batch(7, V, bl, dtype, 4000)
    targs = [torch.tensor(a, dtype=torch.int32) for a in (labels, lx, ly)]
    xt = xr.float().clone().requires_grad_(True)                       # torch's reference on the upcast input (CPU)
    lp = torch.log_softmax(xt, -1).transpose(0, 1)
    ref = torch.nn.functional.ctc_loss(lp, targs[0].long(), targs[1].long(), targs[2].long(), blank=bl, reduction="sum")
    ref.backward()
    x = (xr.transpose(0, 1).contiguous() if tm else xr).to("cuda:0").requires_grad_(True)
    loss = crf.WARP_CTC_LOSS(size_average=False, blank_label=bl, fuse_log_softmax=True, time_major=tm)(x, *targs)
    loss.backward()
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    g = x.grad.float().cpu()
    if tm:
        g = g.transpose(0, 1)
    err_l, err_g = abs(loss.item() - ref.item()) / abs(ref.item()), rel_err(g.numpy(), xt.grad.numpy())
    print(dtype, tm, bl, "loss", loss.item(), ref.item(), "rel", err_l, "grad rel_err", err_g)
    assert err_l <= 1e-4
    assert err_g <= (1e-4 if dtype == "fp32" else 1e-2)                # (16 bits: the result is rounded to the input's dtype)
    avg = crf.WARP_CTC_LOSS(blank_label=bl, fuse_log_softmax=True, time_major=tm)(x.detach(), *targs)
    assert abs(avg.item() * 3 - loss.item()) <= 1e-5 * abs(loss.item())   # size_average divides by N = size(1) when time-major


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the unfused module, time-major
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bl", [0, 17])
def test_warp_ctc_loss_time_major_unfused(crf, poison, bl):
    """WARP_CTC_LOSS(time_major=True) on (T, N, V) log-probs = the batch-major call on the transposed tensor: the loss bit for bit, the
    gradient within 1e-6 of its largest entry (float atomics in the grad pass)."""
    V = 37
    xr, labels, lx, ly, _, _ = make_batch(7, V, bl, "fp32", 4000)
    targs = [torch.tensor(a, dtype=torch.int32) for a in (labels, lx, ly)]
    xb = torch.log_softmax(xr.to("cuda:0"), -1).requires_grad_(True)
    xt = xb.detach().transpose(0, 1).contiguous().requires_grad_(True)
    lb = crf.WARP_CTC_LOSS(blank_label=bl)(xb, *targs)
    lt = crf.WARP_CTC_LOSS(blank_label=bl, time_major=True)(xt, *targs)
    lb.backward()
    lt.backward()
    assert torch.equal(lb, lt), (lb.item(), lt.item())
    assert xt.grad.shape == xt.shape
    gb, gt = xb.grad.cpu().numpy(), xt.grad.transpose(0, 1).cpu().numpy()
    assert np.abs(gb - gt).max() <= 1e-6 * np.abs(gb).max()
