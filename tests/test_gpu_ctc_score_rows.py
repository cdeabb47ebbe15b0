"""GPU tests of the hypothesis scores on DEVICE ROWS (ctc_crf.ctc_score / ctc_logp with CUDA hyps, crf_ctc_score_rows;
cat_amd/csrc/k_rows.hip): the padded rows ctc_sample and ctc_beam_search leave on the device, scored where they lie.  The yardstick is the
CPU-hypotheses call of tests/test_gpu_ctc_score.py, bit for bit -- each hypothesis against the call that takes the kernel of ITS length
class -- and through it the fp64 oracle (`check`, rtol 1e-4)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_ctc_score import DTYPES, KERNEL_OF_L, LX1, N1, T1, V1, _i32, check, reference, run, small_batch
from tests.util import log_softmax_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MIN = -2 ** 31
bits = lambda a: np.asarray(a).view(np.int32)


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def rows(hyps, W, fill):
    """(hyps [H,W] int32 with `fill` behind every length, hyp_lengths [H] int32), both on the device."""
    lab = torch.full((len(hyps), W), fill, dtype=torch.int32)
    for h, a in enumerate(hyps):
        lab[h, :len(a)] = _i32(a)
    return lab.to(DEV), _i32([len(h) for h in hyps]).to(DEV)


def score_rows(crf, x, lab_d, hl_d, utt, lx, blank, layouts=(False, True), fused=False, max_hyp_len=None):
    """x: [N,T,V] CUDA tensor, batch-major; utt / lx: numpy (lx staged from the CPU).  -> (scores, invalid) as numpy after checking that
    the layouts agree bit for bit."""
    out = []
    utt_d = None if utt is None else _i32(utt).to(DEV)
    for tm in layouts:
        xx = x.transpose(0, 1).contiguous() if tm else x
        sc, inv = crf._C.ctc_score(xx, lab_d, hl_d, _i32(lx), utt_d, blank, tm, fused=fused, max_hyp_len=max_hyp_len)
        assert sc.shape == hl_d.shape and sc.dtype == torch.float32 and inv.dtype == torch.int32 and sc.is_cuda and inv.is_cuda
        out.append((sc.cpu().numpy(), inv.cpu().numpy()))
    for sc, inv in out[1:]:
        assert np.array_equal(bits(sc), bits(out[0][0])) and np.array_equal(inv, out[0][1]), ("layouts differ", sc, out[0][0])
    return out[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. one class: the small batch, against the CPU-hypotheses call and the oracle; garbage behind the lengths
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, 2, V1 - 1])
def test_one_class_is_the_cpu_call_bit_for_bit(crf, blank):
    c = small_batch(blank)
    x = torch.tensor(c["logp"]).to(DEV)
    sc, inv = run(crf, x, c["hyps"], c["utt"], LX1, blank)                      # CPU hypotheses, both layouts
    lab_d, hl_d = rows(c["hyps"], 14, blank)
    sc_d, inv_d = score_rows(crf, x, lab_d, hl_d, c["utt"], LX1, blank)
    assert crf._C.last_score_kernel() == "crf_ctc_score_wave_kernel<1>"
    assert np.array_equal(bits(sc_d), bits(sc)) and np.array_equal(inv_d, inv), (sc_d, sc)
    check(sc_d, inv_d, c["cost"], c["valid"], blank)
    for fill in (123456, INT32_MIN):
        lab_g, _ = rows(c["hyps"], 14, fill)
        sc_g, inv_g = score_rows(crf, x, lab_g, hl_d, c["utt"], LX1, blank)
        assert np.array_equal(bits(sc_g), bits(sc)) and np.array_equal(inv_g, inv), ("words behind the length were read", fill)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. every class in one list: each hypothesis takes the kernel of its own length
# ---------------------------------------------------------------------------------------------------------------------------------
def _alone(crf, x, hyp, lx, blank):
    """The CPU-hypotheses call on ONE hypothesis: (score bits, invalid, the kernel it took)."""
    sc, inv = crf._C.ctc_score(x, _i32(hyp) if len(hyp) else torch.zeros(0, dtype=torch.int32), _i32([len(hyp)]), _i32(lx), _i32([0]), blank)
    return bits(sc.cpu().numpy())[0], int(inv.cpu()[0]), crf._C.last_score_kernel()


def test_every_class_in_one_list(crf):
    N, V, T, W, blank = 1, 5, 1212, 600, 0
    lengths = [0, 1, 31, 32, 63, 64, 127, 128, 255, 256, 600]
    rng = np.random.default_rng(7100)
    order = rng.permutation(len(lengths))
    hyps = [rng.integers(1, V, size=lengths[i]).astype(np.int32) for i in order]
    x = torch.tensor(log_softmax_np(rng.normal(0.0, 2.0, size=(N, T, V))).astype(np.float32)).to(DEV)
    lx, utt = np.array([T]), np.zeros(len(hyps), dtype=np.int64)
    want = []
    for h in hyps:
        b, inv, kernel = _alone(crf, x, h, lx, blank)
        assert inv == 0 and kernel == KERNEL_OF_L.get(len(h), "crf_ctc_score_wave_kernel<1>"), (len(h), kernel)
        want.append(b)
    want = np.array(want, dtype=np.int32)
    assert np.all(np.isfinite(want.view(np.float32)))
    lab_d, hl_d = rows(hyps, W, INT32_MIN)
    sc, inv = score_rows(crf, x, lab_d, hl_d, utt, lx, blank)                  # the default bound: min(W, 2047) = 600
    assert crf._C.last_score_kernel() == "crf_ctc_score_wg_kernel<4>"
    assert np.array_equal(bits(sc), want) and not np.any(inv), (sc, want.view(np.float32))
    for cap in (600, 2047):
        sc_c, inv_c = score_rows(crf, x, lab_d, hl_d, utt, lx, blank, layouts=(False,), max_hyp_len=cap)
        assert np.array_equal(bits(sc_c), want) and not np.any(inv_c), cap
    assert crf._C.last_score_kernel() == "crf_ctc_score_wg_kernel<8>"
    perm = rng.permutation(len(hyps))
    idx = torch.tensor(perm).to(DEV)
    sc_p, inv_p = score_rows(crf, x, lab_d[idx].contiguous(), hl_d[idx].contiguous(), utt, lx, blank, layouts=(False,))
    assert np.array_equal(bits(sc_p), want[perm]) and not np.any(inv_p)


def test_longest_hypothesis_beside_a_short_one(crf):
    V, T, blank = 5, 4106, 0
    rng = np.random.default_rng(7200)
    hyps = [rng.integers(1, V, size=2047).astype(np.int32), rng.integers(1, V, size=3).astype(np.int32)]
    x = torch.tensor(log_softmax_np(rng.normal(0.0, 2.0, size=(1, T, V))).astype(np.float32)).to(DEV)
    lx = np.array([T])
    want = [_alone(crf, x, h, lx, blank) for h in hyps]
    assert [w[2] for w in want] == ["crf_ctc_score_wg_kernel<8>", "crf_ctc_score_wave_kernel<1>"] and [w[1] for w in want] == [0, 0]
    lab_d, hl_d = rows(hyps, 2047, INT32_MIN)
    sc, inv = score_rows(crf, x, lab_d, hl_d, [0, 0], lx, blank)
    assert crf._C.last_score_kernel() == "crf_ctc_score_wg_kernel<8>"
    assert np.array_equal(bits(sc), np.array([w[0] for w in want], dtype=np.int32)) and not np.any(inv) and np.all(np.isfinite(sc))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the bound and bad rows: results the contract defines, not exceptions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bound_and_bad_rows(crf):
    blank, W = 2, 34
    c = small_batch(blank)
    x = torch.tensor(c["logp"]).to(DEV)
    sc0, inv0 = run(crf, x, c["hyps"], c["utt"], LX1, blank, layouts=(False,))
    H0 = len(c["hyps"])
    rng = np.random.default_rng(7300)
    pool = np.array([v for v in range(V1) if v != blank])
    draw = lambda n: pool[rng.integers(0, len(pool), size=n)].astype(np.int32)
    long32 = pool[np.arange(32) % len(pool)].astype(np.int32)                     # no repeats: fits lx = 48, only the bound refuses it
    _, ok32 = reference(c["logp"], [long32], [0], LX1, blank)
    assert ok32[0] == 1
    bad_v, bad_neg = draw(3), draw(3)
    bad_v[1], bad_neg[2] = V1, -7
    extra = [long32, draw(3), draw(3), draw(3), draw(3), bad_v, bad_neg]
    lab_d, hl_d = rows(list(c["hyps"]) + extra, W, INT32_MIN)
    hl = hl_d.cpu()
    hl[H0 + 1], hl[H0 + 2] = -1, W + 1
    utt = np.concatenate([c["utt"], [0, 0, 0, -1, N1, 0, 0]])
    sc, inv = score_rows(crf, x, lab_d, hl.to(DEV), utt, LX1, blank, max_hyp_len=31)
    assert crf._C.last_score_kernel() == "crf_ctc_score_wave_kernel<1>"
    assert not np.any(np.isnan(sc))
    assert np.all(sc[H0:] == -np.inf) and np.all(inv[H0:] == 1), (sc[H0:], inv[H0:])
    assert np.array_equal(bits(sc[:H0]), bits(sc0)) and np.array_equal(inv[:H0], inv0)
    # the same rows under a bound that admits the 32 labels: only that hypothesis changes, into the CPU call's bits for it
    sc2, inv2 = score_rows(crf, x, lab_d, hl.to(DEV), utt, LX1, blank, max_hyp_len=32)
    s32, i32_ = crf._C.ctc_score(x, _i32(long32), _i32([32]), _i32(LX1), _i32([0]), blank)
    assert inv2[H0] == 0 and bits(sc2)[H0] == bits(s32.cpu().numpy())[0] and int(i32_.cpu()[0]) == 0
    assert np.array_equal(bits(sc2[:H0]), bits(sc0)) and np.all(sc2[H0 + 1:] == -np.inf) and np.all(inv2[H0 + 1:] == 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. raw network output
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [V1, 300])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_raw_output_is_the_fused_cpu_call(crf, dtype, V):
    blank = 2
    c = small_batch(blank)
    rng = np.random.default_rng(7400 + V)
    x = torch.tensor(rng.normal(0.0, 2.0, size=(N1, T1, V)).astype(np.float32)).to(DTYPES[dtype]).to(DEV)
    sc, inv = run(crf, x, c["hyps"], c["utt"], LX1, blank, fused=True)
    lab_d, hl_d = rows(c["hyps"], 13, INT32_MIN)
    sc_d, inv_d = score_rows(crf, x, lab_d, hl_d, c["utt"], LX1, blank, fused=True)
    assert np.array_equal(bits(sc_d), bits(sc)) and np.array_equal(inv_d, inv), (dtype, V, sc_d, sc)
    assert np.array_equal(inv_d, 1 - c["valid"]) and not np.any(np.isnan(sc_d))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the chain: sample / beam search -> score, nothing leaves the device
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lx_on_device", [False, True])
def test_chain_sample_and_beam_to_score(crf, lx_on_device):
    N, T, V = 4, 40, 8
    rng = np.random.default_rng(7500)
    x = torch.tensor(log_softmax_np(rng.normal(0.0, 2.0, size=(N, T, V))).astype(np.float32)).to(DEV)
    lx = torch.tensor([40, 33, 17, 5], dtype=torch.int32)
    lx_in = lx.to(DEV) if lx_on_device else lx
    hyps, hl, hu = crf.ctc_sample(x, lx, 5, seed=75)
    got = crf.ctc_score(x, hyps, hl, lx_in, hu)
    want = crf.ctc_score(x, hyps.cpu(), hl.cpu(), lx, hu.cpu())
    assert got.shape == (N * 5,) and np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
    assert bool(torch.isfinite(want).all())
    hyps, hl, hu, _ = crf.ctc_beam_search(x, lx, beam_size=8, nbest=4)
    got = crf.ctc_score(x, hyps, hl, lx_in, hu)
    want = crf.ctc_score(x, hyps.cpu(), hl.cpu(), lx, hu.cpu())
    assert got.shape == (N * 4,) and np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))


def test_mixed_placement_is_refused_by_name(crf):
    x = torch.zeros(2, 10, 8, device=DEV)
    hyps, hl, hu = torch.ones(2, 3, dtype=torch.int32), torch.tensor([2, 3], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    lx = torch.tensor([10, 10], dtype=torch.int32)
    for f in (crf.ctc_score, crf.ctc_logp):
        with pytest.raises(RuntimeError, match="hyp_lengths is a CPU tensor"):
            f(x, hyps.to(DEV), hl, lx, hu.to(DEV))
        with pytest.raises(RuntimeError, match="hyp_utt is a CPU tensor"):
            f(x, hyps.to(DEV), hl.to(DEV), lx, hu)
        with pytest.raises(RuntimeError, match="hyp_lengths is a CUDA tensor"):
            f(x, hyps, hl.to(DEV), lx, hu)
        with pytest.raises(RuntimeError, match="padded rows"):
            f(x, hyps.to(DEV).reshape(-1), hl.to(DEV), lx, hu.to(DEV))
        with pytest.raises(RuntimeError, match="int32"):
            f(x, hyps.to(DEV).long(), hl.to(DEV), lx, hu.to(DEV))
        with pytest.raises(RuntimeError, match="max_hyp_len=2048 exceeds 2047"):
            f(x, hyps.to(DEV), hl.to(DEV), lx, hu.to(DEV), max_hyp_len=2048)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. no synchronisation: torch's sync debug mode raises on anything that waits for the device
# ---------------------------------------------------------------------------------------------------------------------------------
def test_device_rows_never_synchronise(crf):
    N, T, V, K = 4, 40, 8, 5
    rng = np.random.default_rng(7600)
    x = torch.tensor(log_softmax_np(rng.normal(0.0, 2.0, size=(N, T, V))).astype(np.float32)).to(DEV)
    lx = torch.tensor([40, 33, 17, 5], dtype=torch.int32)
    hyps, hl, hu = crf.ctc_sample(x, lx, K, seed=76)
    risk = torch.arange(N * K, dtype=torch.float32, device=DEV)
    leaf = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):      # the positive control: this build enforces the mode
            torch.ones(1, device=DEV).item()
        scores = crf.ctc_score(x, hyps, hl, lx, hu)
        lp, inv = crf.ctc_logp(leaf, hyps, hl, lx, hu, max_hyp_len=T)
        (torch.softmax(lp.view(N, K), -1) * risk.view(N, K)).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(leaf.grad).all()) and np.array_equal(bits(scores.cpu().numpy()), bits(lp.detach().cpu().numpy()))
