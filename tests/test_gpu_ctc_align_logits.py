"""GPU tests of the forced alignment on RAW network output (ctc_crf.ctc_align(fuse_log_softmax=True) / crf_ctc_align_logits,
cat_amd/csrc/k_align.hip) in fp32, bf16 and fp16 against the fp64 NumPy Viterbi of tests/align_ref.py.

Harness of tests/test_gpu_ctc_align.py: every call writes into `pos` / `scores` tensors prefilled with a sentinel, on a workspace filled with
0xFF bytes (the lse values of frames at or past lx would read as NaN), and runs batch-major AND time-major; the two must agree bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import align_ref
from tests.test_gpu_ctc_align import SENT_POS, SENT_SCORE, bound, random_alignment, tokens_of

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def lse_lanes(V):
    """Lanes that share a row in crf_align_lse_kernel (include/ctc_crf_hip.h)."""
    return 16 if V <= 256 else 64


def lse64(xh):
    """fp64 lse of every row of the upcast input [..., V]."""
    x = np.asarray(xh, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]


def tolerance(lx, V, raw_sum, lse_row):
    """bound(lx, max(|raw path sum|, sum_t |lse_t|)) + lx 2^-24 (V / g + 8): the recursion's fp32 sums (tests/test_gpu_ctc_align.py), and
    per frame the longest chain of fp32 additions in the lse kernel (V / g entries per lane, then the butterfly) plus a few ulp for exp, log."""
    return bound(lx, max(abs(raw_sum), float(np.abs(lse_row[:lx]).sum()))) + lx * 2.0 ** -24 * (V / lse_lanes(V) + 8)


def run(crf, x, labels, lx, ly, blank, layouts=(False, True), fused=True):
    """x: [B,T,V] CUDA tensor of any of the three dtypes, batch-major.  -> (pos [B,T], tokens [B,T], scores [B], invalid [B]) as numpy,
    after checking that the layouts agree bit for bit, that no sentinel is left and that tokens belong to pos."""
    B, T, V = x.shape
    lab_t, lx_t, ly_t = (torch.tensor(np.asarray(a), dtype=torch.int32) for a in (labels, lx, ly))
    out = {}
    for tm in layouts:
        xx = x.transpose(0, 1).contiguous() if tm else x
        pos0 = torch.full((B, T), SENT_POS, dtype=torch.int32, device=x.device)
        sc0 = torch.full((B,), SENT_SCORE, dtype=torch.float32, device=x.device)
        pos, tok, sc, inv = crf._C.ctc_align(xx, lab_t, lx_t, ly_t, blank, tm, pos_out=pos0, scores_out=sc0, fused=fused)
        assert pos.data_ptr() == pos0.data_ptr() and sc.data_ptr() == sc0.data_ptr()
        assert tok.dtype == torch.int32 and tok.shape == (B, T)
        out[tm] = tuple(a.cpu().numpy() for a in (pos, tok, sc, inv))
        del xx
    first = out[layouts[0]]
    for tm in layouts[1:]:
        for a, c in zip(first, out[tm]):
            assert np.array_equal(a.view(np.int32), c.view(np.int32)), ("layouts differ", tm)
    pos, tok, sc, inv = first
    assert not np.any(pos == SENT_POS) and not np.any(sc == SENT_SCORE)
    assert np.all((inv == 0) | (inv == 1))
    assert np.array_equal(tok, tokens_of(pos, labels, ly, blank)), "tokens do not belong to pos"
    return pos, tok, sc, inv


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. an exact grid: the path and the tie rule, bit for bit, in every dtype
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [8, 37])
@pytest.mark.parametrize("L", [0, 1, 7, 255, 256, 512, 1024, 2047])
def test_exact_grid_paths(crf, L, V):
    """Raw values are multiples of 0.25 in [-8, 8]: exact in fp32, bf16 and fp16, and every partial sum is exact in fp32 as in fp64, so
    the kernel's recursion and the oracle's compare the same numbers -- with many exact ties on so coarse a grid.  pos must equal
    align_ref.viterbi on the raw values and be the same in the three dtypes and the two layouts.  L covers every NR; lx = L + repeats (one
    alignment) and about 1.5 L + 20; blank at 0, V - 1 and inside."""
    rng = np.random.default_rng(7000 + 3 * L + V)
    for blank in (0, V - 1, V // 2):
        pool = np.array([v for v in range(V) if v != blank])
        labs = [pool[rng.integers(0, len(pool), size=L)], pool[rng.integers(0, len(pool), size=L)]]
        need = [max(1, len(a) + int((a[1:] == a[:-1]).sum())) for a in labs]
        lx = np.array([need[0], max(need[1], int(1.5 * L) + 20)])
        T = int(lx.max()) + 1
        xn = (rng.integers(-32, 33, size=(2, T, V)) * 0.25).astype(np.float32)
        labels, ly = np.concatenate(labs), np.array([L, L])
        want = [align_ref.viterbi(xn[b, :int(lx[b])], labs[b], blank) for b in range(2)]
        lse = lse64(xn)
        seen = {}
        for name, dt in DTYPES.items():
            x = torch.tensor(xn).to(dt).to("cuda:0")
            assert torch.equal(x.float().cpu(), torch.tensor(xn))          # the grid is exact in this dtype
            pos, tok, sc, inv = run(crf, x, labels, lx, ly, blank)
            assert np.all(inv == 0)
            for b in range(2):
                n = int(lx[b])
                raw, rpos = want[b]
                bad = np.nonzero(pos[b, :n] != rpos)[0]
                assert bad.size == 0, (name, L, V, blank, b, bad[:5], pos[b][bad[:5]], rpos[bad[:5]])
                assert np.all(pos[b, n:] == -2)
                ref = raw - lse[b, :n].sum()
                assert abs(sc[b] - ref) <= tolerance(n, V, raw, lse[b]), (name, L, V, blank, b, sc[b], ref)
            seen[name] = (pos, sc)
        for name in ("bf16", "fp16"):
            assert np.array_equal(seen[name][0], seen["fp32"][0])
            assert np.array_equal(seen[name][1].view(np.int32), seen["fp32"][1].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. dense random raw values: a valid path with the best score under log_softmax
# ---------------------------------------------------------------------------------------------------------------------------------
_DENSE = {}


def dense_raw(T, V, sigma):
    """Six ragged utterances (tests/test_gpu_ctc_align.py::dense_batch's lengths and transcripts) on N(0, 1) sigma raw values, fp32 on the CPU."""
    key = (T, V, sigma)
    if key not in _DENSE:
        _DENSE.clear()                                                   # (one batch at a time: V = 8192 is 65 MB)
        seed = 100 * T + V + sigma
        blank = (0, V - 1, V // 3)[(T + V) % 3]
        rng = np.random.default_rng(seed)
        x = torch.tensor(rng.standard_normal((6, T, V), dtype=np.float32) * np.float32(sigma))
        lx = np.array([T, T, max(1, T - 1), max(1, T // 2), max(1, T // 3), T])
        pool = np.array([v for v in range(V) if v != blank])
        labs = []
        for b in range(6):
            n = int(rng.integers(0, lx[b] // 2 + 2)) if b else int(lx[b] + 1) // 2
            a = pool[rng.integers(0, min(len(pool), 6 if b % 2 else len(pool)), size=n)]
            while not align_ref.fits(a, int(lx[b])):
                a = a[:-1]
            labs.append(a)
        _DENSE[key] = (x, blank, lx, labs)
    return _DENSE[key]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("sigma", [1, 5])
@pytest.mark.parametrize("V", [37, 72, 8192])
@pytest.mark.parametrize("T", [1, 2, 50, 333])
def test_dense_random_scores(crf, T, V, sigma, dtype):
    """ref = the fp64 Viterbi optimum on log_softmax64(x^), returned = the fp64 score of the returned path there: |score - ref| <= tol and
    |returned - ref| <= tol.  For fp32 also: the scores of today's path, ctc_align(log_softmax(x)), lie within the same tol."""
    x32, blank, lx, labs = dense_raw(T, V, sigma)
    xr = x32.to(DTYPES[dtype])
    xh = xr.float().numpy()
    labels, ly = np.concatenate(labs).astype(np.int64), np.array([len(a) for a in labs])
    xd = xr.to("cuda:0")
    pos, tok, sc, inv = run(crf, xd, labels, lx, ly, blank)
    assert np.all(inv == 0)
    if dtype == "fp32":
        _, _, sc_old, _ = run(crf, torch.log_softmax(xd, -1), labels, lx, ly, blank, fused=False)
    for b, a in enumerate(labs):
        n = int(lx[b])
        lse = lse64(xh[b, :n])
        lsm = xh[b, :n].astype(np.float64) - lse[:, None]
        ref, rpos = align_ref.viterbi(lsm, a, blank)
        assert rpos is not None
        align_ref.check_path(pos[b], a, n, blank)
        returned = align_ref.path_score(lsm, pos[b], a, n, blank)
        raw = align_ref.path_score(xh[b], pos[b], a, n, blank)
        tol = tolerance(n, V, raw, lse)
        print(dtype, T, V, sigma, "utterance", b, "score", sc[b], "ref", ref, "returned", returned, "tol", tol)
        assert abs(sc[b] - ref) <= tol, (b, sc[b], ref, tol)
        assert abs(returned - ref) <= tol, (b, returned, ref, tol)
        if dtype == "fp32":
            assert abs(sc_old[b] - sc[b]) <= tol, (b, sc_old[b], sc[b], tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. invalid, dead and empty utterances
# ---------------------------------------------------------------------------------------------------------------------------------
def c_level(core, x, time_major, blank, labels, off, lx, ly, max_l, fused):
    """crf_ctc_align_logits / crf_ctc_align with device metadata that the Python layer would refuse (a label outside [0, V))."""
    B, T, V = x.shape if not time_major else (x.shape[1], x.shape[0], x.shape[2])
    dev = x.device
    d = [torch.tensor(np.asarray(a), dtype=torch.int32, device=dev) for a in (labels, off, lx, ly)]
    pos = torch.full((B, T), SENT_POS, dtype=torch.int32, device=dev)
    sc = torch.full((B,), SENT_SCORE, dtype=torch.float32, device=dev)
    inv = torch.full((B,), -5, dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    nb = (core._lib.crf_ctc_align_logits_workspace_bytes if fused else core._lib.crf_ctc_align_workspace_bytes)(B, T, V, max_l)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    st = vp(torch.cuda.current_stream().cuda_stream)
    tail = (vp(d[0].data_ptr()), vp(d[1].data_ptr()), vp(d[2].data_ptr()), vp(d[3].data_ptr()), B, T, V, max_l, vp(pos.data_ptr()),
            vp(sc.data_ptr()), vp(inv.data_ptr()), vp(ws.data_ptr()), nb, st)
    if fused:
        rc = core._lib.crf_ctc_align_logits(vp(x.data_ptr()), {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[x.dtype],
                                            1 if time_major else 0, blank, *tail)
    else:
        rc = core._lib.crf_ctc_align(vp(x.data_ptr()), 1 if time_major else 0, blank, *tail)
    assert rc == 0, core._lib.crf_last_error()
    torch.cuda.synchronize()
    return pos.cpu().numpy(), sc.cpu().numpy(), inv.cpu().numpy()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_invalid_dead_and_empty_utterances(crf, dtype):
    """L + repeats > lx and lx = 0: score -inf, row -2, invalid 1.  -inf entries that leave exactly one alignment: that path.  A frame of
    -inf and a label whose column is -inf: every alignment dead, score -inf, row -2, invalid 0.  ly = 0: all blank.  A label outside [0, V)
    (C level): invalid 1 -- the flags are those of crf_ctc_align on the upcast input."""
    V, blank, T = 5, 0, 40
    rng = np.random.default_rng(5)
    xn = rng.normal(0.0, 2.0, size=(7, T, V)).astype(np.float32)
    labs = [np.array([1, 1, 2]), np.array([3, 4]), np.array([1, 2, 2, 3]), np.array([1, 2, 2, 3]), np.array([], dtype=np.int64),
            np.array([2, 3, 4]), np.array([2, 3, 4])]
    lx = np.array([3, 0, 30, 30, 17, 40, 40])         # 0: needs 4 frames; 1: no frames; 2: one alignment left; 3: none; 4: empty; 5: ordinary
    cls, want2 = random_alignment(rng, labs[2], 30, blank)
    keep = xn[2, np.arange(30), cls].copy()
    xn[2, :30] = -np.inf
    xn[2, np.arange(30), cls] = keep
    xn[3, :30] = xn[2, :30]
    xn[3, 11, :] = -np.inf                             # a frame nothing can pass
    xn[6, :, 3] = -np.inf                              # 6: a label's column is -inf in every frame
    xr = torch.tensor(xn).to(DTYPES[dtype])
    xh = xr.float().numpy()
    labels, ly = np.concatenate(labs), np.array([len(a) for a in labs])
    pos, tok, sc, inv = run(crf, xr.to("cuda:0"), labels, lx, ly, blank)
    assert inv.tolist() == [1, 1, 0, 0, 0, 0, 0]
    for b in (0, 1, 3, 6):
        assert sc[b] == -np.inf and np.all(pos[b] == -2) and np.all(tok[b] == -1), b
    assert np.array_equal(pos[2, :30], want2) and np.all(pos[2, 30:] == -2)
    for b, n in ((2, 30), (4, 17), (5, 40)):
        lse = lse64(xh[b, :n])
        raw = align_ref.path_score(xh[b], pos[b], labs[b], n, blank)
        ref, _ = align_ref.viterbi(xh[b, :n].astype(np.float64) - lse[:, None], labs[b], blank)
        assert abs(sc[b] - ref) <= tolerance(n, V, raw, lse), (b, sc[b], ref)
    assert np.all(pos[4, :17] == -1) and np.all(pos[4, 17:] == -2) and np.all(tok[4, :17] == blank)
    # the C level, with a label outside [0, V) in utterance 5; the same flags and rows from crf_ctc_align on the upcast values
    off = np.concatenate([[0], np.cumsum(ly)[:-1]])
    bad = labels.copy()
    bad[off[5] + 1] = V
    xd = xr.to("cuda:0")
    for tm in (False, True):
        xx = xd.transpose(0, 1).contiguous() if tm else xd
        p1, s1, i1 = c_level(crf._C, xx, tm, blank, bad, off, lx, ly, 4, True)
        p0, s0, i0 = c_level(crf._C, xx.float(), tm, blank, bad, off, lx, ly, 4, False)
        assert i1.tolist() == [1, 1, 0, 0, 0, 1, 0] and np.array_equal(i1, i0)
        assert np.array_equal(p1, p0)
        assert s1[5] == -np.inf and np.all(p1[5] == -2)
        assert np.array_equal(np.isneginf(s1), np.isneginf(s0))
        assert np.array_equal(p1[[0, 1, 2, 3, 4, 6]], pos[[0, 1, 2, 3, 4, 6]])


def test_public_surface(crf):
    """ctc_crf.ctc_align(fuse_log_softmax=True): three device tensors, no autograd, on bf16 in both layouts."""
    x32, blank, lx, labs = dense_raw(50, 37, 1)
    x = x32.to(torch.bfloat16).to("cuda:0").requires_grad_(True)
    args = [torch.tensor(a, dtype=torch.int32) for a in (np.concatenate(labs), lx, [len(a) for a in labs])]
    pos, tok, sc = crf.ctc_align(x, *args, blank=blank, fuse_log_softmax=True)
    assert pos.is_cuda and tok.is_cuda and sc.is_cuda and not sc.requires_grad and sc.dtype == torch.float32
    pos_t, tok_t, sc_t = crf.ctc_align(x.detach().transpose(0, 1).contiguous(), *args, blank=blank, time_major=True, fuse_log_softmax=True)
    assert torch.equal(pos, pos_t) and torch.equal(tok, tok_t) and torch.equal(sc, sc_t)
    with pytest.raises(RuntimeError, match="labels must lie"):
        bad = args[0].clone(); bad[0] = 37
        crf.ctc_align(x.detach(), bad, args[1], args[2], blank=blank, fuse_log_softmax=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. beyond 2^31 elements
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bf16_activations_beyond_2_31_elements(crf):
    """bf16 rows past 2^31 elements (64-bit row addresses in both kernels), both layouts: B x T x V just above 2^31 constant activations,
    a planted path in the LAST utterance only; the others have empty transcripts."""
    B, T, V, blank = 96, 2800, 8000, 3
    assert 2 ** 31 < B * T * V < 2 ** 31 + 2 ** 24
    if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
        pytest.skip("needs 12 GB of free device memory")
    rng = np.random.default_rng(31)
    pool = np.array([v for v in range(V) if v != blank])
    labs = [pool[rng.integers(0, len(pool), size=300)] if b == B - 1 else pool[:0] for b in range(B)]
    lx = np.array([T - (b % 7) for b in range(B)])
    n = int(lx[B - 1])
    cls, want = random_alignment(rng, labs[B - 1], n, blank)
    labels, ly = np.concatenate(labs), np.array([len(a) for a in labs])
    lo, hi = -2.0, 3.0                                                   # (exact in bf16)
    res = {}
    for tm in (False, True):
        x = torch.full((T, B, V) if tm else (B, T, V), lo, dtype=torch.bfloat16, device="cuda:0")
        row = x[:n, B - 1] if tm else x[B - 1, :n]
        row[torch.arange(n, device="cuda:0"), torch.tensor(cls, device="cuda:0")] = hi
        pos0 = torch.full((B, T), SENT_POS, dtype=torch.int32, device="cuda:0")
        sc0 = torch.full((B,), SENT_SCORE, dtype=torch.float32, device="cuda:0")
        pos, tok, sc, inv = crf._C.ctc_align(x, *[torch.tensor(a, dtype=torch.int32) for a in (labels, lx, ly)], blank, tm, pos_out=pos0,
                                             scores_out=sc0, fused=True)
        res[tm] = tuple(a.cpu().numpy() for a in (pos, tok, sc, inv))
        del x, row, pos, tok, sc, inv
        torch.cuda.empty_cache()
    for a, c in zip(res[False], res[True]):
        assert np.array_equal(a.view(np.int32), c.view(np.int32))
    pos, tok, sc, inv = res[False]
    assert np.all(inv == 0) and not np.any(pos == SENT_POS) and not np.any(sc == SENT_SCORE)
    for b in range(B):
        m = int(lx[b])
        assert np.array_equal(pos[b, :m], want if b == B - 1 else np.full(m, -1)) and np.all(pos[b, m:] == -2), b
    lse_hi, lse_lo = np.log(np.exp(hi) + (V - 1) * np.exp(lo)), lo + np.log(V)
    ref = n * (hi - lse_hi)
    assert abs(sc[B - 1] - ref) <= bound(n, max(n * hi, n * lse_hi)) + n * 2.0 ** -24 * (V / 64 + 8), (sc[B - 1], ref)
    assert abs(sc[0] - int(lx[0]) * (lo - lse_lo)) <= bound(int(lx[0]), int(lx[0]) * max(abs(lo), lse_lo)) + int(lx[0]) * 2.0 ** -24 * (V / 64 + 8)
