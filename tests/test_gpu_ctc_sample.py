"""GPU tests of the sampler and the best-path decoder (ctc_crf.ctc_sample / ctc_greedy, crf_ctc_sample; cat_amd/csrc/k_sample.hip) against
the NumPy yardstick tests/sample_ref.py: every uniform is recomputed on the host (Philox4x32-10 is counter-based), every draw is held to
the fp64 CDF of softmax of the upcast row, every collapsed sequence to the frame path the call reports -- no statistics.

Draw tolerance: class c is admissible for u iff w_c > 0 and P[c-1] - eps <= u < P[c] + eps with eps = (V + 64) 2^-23: the worst case of an
fp32 sum of V terms in any order (V 2^-24 relative on both the partial sum and the total) plus 64 2^-23 for the hardware's exp.  Every
call runs on a poisoned workspace and writes into outputs prefilled with a sentinel."""
import numpy as np
import pytest
import torch

from tests import sample_ref

pytestmark = pytest.mark.gpu
SENT = -77
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def _i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int64).reshape(-1), dtype=torch.int32)


def eps_of(V):
    return (V + 64) * 2.0 ** -23


def make_x(N, T, V, dtype, seed, neg_col=True):
    """[N,T,V] on the GPU: 2 * normal, one column at -inf (V >= 2), rounded to `dtype`."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((N, T, V))).astype(np.float32)
    if neg_col and V >= 2:
        x[:, :, int(rng.integers(V))] = -np.inf
    return torch.tensor(x).to(dtype).to("cuda:0")


def ragged(N, T):
    return [T] if N == 1 else [T, 0, max(1, T // 2)][:N] + [T] * (N - 3)


def run(crf, x, lx, K, seed, offset=0, blank=0, time_major=False, greedy=False):
    """x: [N,T,V] CUDA tensor, batch-major (transposed here for time_major).  -> (hyps [N K,T], hyp_len [N K], paths [N K,T]) as numpy,
    after checking that no sentinel is left in any output."""
    N, T, V = x.shape
    xin = x.transpose(0, 1).contiguous() if time_major else x
    H = N * K
    hyps = torch.full((H, T), SENT, dtype=torch.int32, device=x.device)
    paths = torch.full((H, T), SENT, dtype=torch.int32, device=x.device)
    h2, hl, p2 = crf._C.ctc_sample(xin, _i32(lx), K, seed, offset, blank, time_major, greedy=greedy, hyps_out=hyps, paths_out=paths)
    assert h2 is hyps and p2 is paths and hl.shape == (H,) and hl.dtype == torch.int32
    want = "crf_sample_row_kernel<%d%s>" % (16 if V <= 256 else 64, ", greedy" if greedy else "")
    assert crf._C.last_sample_kernel() == want
    hyps, hl, paths = hyps.cpu().numpy(), hl.cpu().numpy(), paths.cpu().numpy()
    assert not np.any(hyps == SENT) and not np.any(paths == SENT)
    return hyps, hl, paths


def check_draws(x, lx, K, seed, offset, blank, paths):
    """Every class of every frame t < lx[n] of every path is admissible for its uniform; -> the share of draws with exactly one
    admissible class."""
    N, T, V = x.shape
    x64 = x.float().double().cpu().numpy()
    single = total = 0
    for n in range(N):
        L = int(lx[n])
        if L == 0:
            continue
        u = sample_ref.uniforms(seed, offset, n, L, K)                       # [L][K]
        adm = sample_ref.admissible(x64[n, :L], u, eps_of(V))               # [L][K][V]
        got = paths[n * K:(n + 1) * K, :L].T                                # [L][K]
        assert got.min() >= 0 and got.max() < V
        ok = np.take_along_axis(adm, got[..., None], axis=-1)[..., 0]
        assert ok.all(), ("draw outside the admissible set", n, np.argwhere(~ok)[:5], got[~ok][:5], u[~ok][:5])
        single += int((adm.sum(-1) == 1).sum())
        total += L * K
    return single / max(total, 1)


def check_collapse(paths, hyps, hl, lx, K, blank):
    want_h, want_l, want_p = sample_ref.expected_outputs(paths, lx, K, blank)
    assert np.array_equal(paths, want_p), "paths must be -1 exactly from lx on"
    assert np.array_equal(hl, want_l), (hl, want_l)
    assert np.array_equal(hyps, want_h)


# (V, T, K, N, blank, dtype): every value of each axis at least once, both row kernels (V <= 256: 16 lanes per row), every dtype with an odd V
CASES = [(1, 1, 1, 1, 0, "fp32"), (2, 63, 3, 3, 1, "fp32"), (63, 64, 4, 1, 0, "bf16"), (64, 65, 5, 3, 63, "fp32"),
         (65, 130, 64, 1, 17, "fp16"), (72, 130, 65, 3, 0, "fp32"), (73, 64, 4, 3, 72, "bf16"), (300, 65, 3, 3, 5, "fp32"),
         (301, 63, 5, 3, 300, "fp16"), (600, 63, 5, 1, 599, "bf16"), (5000, 5, 4, 3, 2500, "fp32")]


@pytest.mark.parametrize("V,T,K,N,blank,dtype", CASES)
def test_draws_and_collapse(crf, V, T, K, N, blank, dtype):
    """1. the draw check, 2. the collapse check."""
    x = make_x(N, T, V, DTYPES[dtype], seed=V * 1000 + T)
    lx = ragged(N, T)
    seed, offset = 0x9E3779B97F4A7C15 ^ V, T
    hyps, hl, paths = run(crf, x, lx, K, seed, offset, blank)
    check_draws(x, lx, K, seed, offset, blank, paths)
    check_collapse(paths, hyps, hl, lx, K, blank)


def test_the_draw_check_bites(crf):
    """V = 72, 2 * normal with one -inf column: at least 99 % of the draws have exactly ONE admissible class (99.75 % in a CPU simulation
    of the yardstick alone) -- asserted on the yardstick, whatever the kernel drew; and the kernel's draws pass."""
    N, T, V, K = 3, 130, 72, 65
    x = make_x(N, T, V, torch.float32, seed=72)
    lx = [T, T, T]
    hyps, hl, paths = run(crf, x, lx, K, 12345, 6)
    share = check_draws(x, lx, K, 12345, 6, 0, paths)
    x64 = x.double().cpu().numpy()
    adm = np.concatenate([sample_ref.admissible(x64[n], sample_ref.uniforms(12345, 6, n, T, K), eps_of(V)) for n in range(N)])
    yard = float((adm.sum(-1) == 1).mean())
    assert yard >= 0.99 and abs(share - yard) < 1e-12, (yard, share)
    assert not adm[..., np.isneginf(x64[0, 0])].any()                     # the -inf column is admissible for no draw
    # the draws are spread: every class of positive weight of a 72-class row appears among the 3 * 130 * 65 draws
    assert len(np.unique(paths)) == V - 1


def test_rows_of_minus_inf_and_zero_weights(crf):
    """A row of -inf only emits the blank; a class at -inf is never drawn, even next to tiny weights; lx = 0 and lx = T side by side."""
    N, T, V, K, blank = 2, 9, 7, 6, 4
    x = make_x(N, T, V, torch.float32, seed=5, neg_col=False)
    x[0, 3, :] = -np.inf
    x[1, 0, :] = -np.inf
    x[0, 5, [0, 2, 6]] = -np.inf
    x[0, 6, :] = torch.tensor([-np.inf, -90.0, -np.inf, 0.0, -np.inf, -100.0, -np.inf])   # weights that underflow next to weight 1
    hyps, hl, paths = run(crf, x, [T, T], K, 3, 0, blank)
    assert np.all(paths[:K, 3] == blank) and np.all(paths[K:, 0] == blank)
    assert not np.isin(paths[:K, 5], [0, 2, 6]).any()
    assert np.all(paths[:K, 6] == 3)
    g_h, g_l, g_p = run(crf, x, [T, T], 1, 0, 0, blank, greedy=True)
    assert g_p[0, 3] == 0 and g_p[1, 0] == 0                             # torch.argmax's rule for the arg-max of a row of -inf only
    check_collapse(g_p, g_h, g_l, [T, T], 1, blank)


def forced_paths(T, V, blank):
    """Frame paths with the collapse's corner cases around the 64-frame steps (frames 63/64 and 127/128), as [5][T] classes."""
    a, b, c = [v for v in range(V) if v != blank][:3]
    alt = np.array([a, b] * T)[:T]                                         # no blank, no repeat
    p0 = alt.copy()                                                        # a repeat straddling 63/64 and 127/128
    p0[64], p0[128] = p0[63], p0[127]
    p1 = alt.copy()                                                        # a blank between two equal labels there
    p1[62:65] = [a, blank, a]
    p1[126:129] = [b, blank, b]
    p1[61], p1[65], p1[125], p1[129] = c, c, c, c
    p2 = np.full(T, blank)                                                 # all blanks
    p3 = alt.copy()                                                        # length = T
    last = V - 1 if blank != V - 1 else V - 2                              # the largest label, also across the step
    p4 = np.where(np.arange(T) % 3 == 0, last, np.where(np.arange(T) % 3 == 1, blank, a))
    return np.stack([p0, p1, p2, p3, p4])


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("blank,V", [(0, 5), (4, 5), (2, 301)])
def test_forced_paths(crf, dtype, blank, V):
    """3. one-hot rows (0 at the chosen class, -inf elsewhere): the path is the same for any seed, in sample and greedy mode."""
    T, K = 130, 3
    fp = forced_paths(T, V, blank)
    N = len(fp)
    x = torch.full((N, T, V), -np.inf)
    x.scatter_(2, torch.tensor(fp)[..., None], 0.0)
    x = x.to(DTYPES[dtype]).to("cuda:0")
    lx = [T, T, T, T, T - 1]
    want_h, want_l, want_p = sample_ref.expected_outputs(np.repeat(fp, K, axis=0), lx, K, blank)
    assert want_l[3 * K] == T and want_l[2 * K] == 0
    for tm in (False, True):
        hyps, hl, paths = run(crf, x, lx, K, 99 + blank, 1, blank, time_major=tm)
        assert np.array_equal(paths, want_p) and np.array_equal(hl, want_l) and np.array_equal(hyps, want_h)
        g_h, g_l, g_p = run(crf, x, lx, 1, 0, 0, blank, time_major=tm, greedy=True)
        assert np.array_equal(g_p, want_p[::K]) and np.array_equal(g_l, want_l[::K]) and np.array_equal(g_h, want_h[::K])


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("V", [7, 73, 300])
def test_greedy(crf, dtype, V):
    """4. torch.argmax of the upcast rows + collapse, on random rows and on rows with exact ties (the lowest index wins), both layouts,
    through the public call."""
    N, T, blank = 3, 70, V // 2
    rng = np.random.default_rng(V)
    x = make_x(N, T, V, DTYPES[dtype], seed=V + 1)
    ties = torch.tensor(rng.integers(0, 3, size=(N, T // 2, V)).astype(np.float32)).to(DTYPES[dtype]).to("cuda:0")   # many equal maxima
    x[:, ::2][:, :T // 2] = ties
    lx = [T, 0, 33]
    am = torch.argmax(x.float(), -1).cpu().numpy()
    assert (x.float() == x.float().max(-1, keepdim=True).values).sum(-1).max() > 1       # ties exist
    want_h, want_l, want_p = sample_ref.expected_outputs(am, lx, 1, blank)
    for tm in (False, True):
        g_h, g_l, g_p = run(crf, x, lx, 1, 0, 0, blank, time_major=tm, greedy=True)
        assert np.array_equal(g_p, want_p) and np.array_equal(g_l, want_l) and np.array_equal(g_h, want_h)
        xin = x.transpose(0, 1).contiguous().requires_grad_(True) if tm else x.clone().requires_grad_(True)
        h, l = crf.ctc_greedy(xin, _i32(lx), blank=blank, time_major=tm)
        assert h.is_cuda and l.is_cuda and not h.requires_grad and h.dtype == torch.int32 and l.dtype == torch.int32
        assert np.array_equal(h.cpu().numpy(), want_h) and np.array_equal(l.cpu().numpy(), want_l)


@pytest.mark.parametrize("dtype,V", [("fp32", 72), ("bf16", 73), ("fp16", 301)])
def test_reproducible_bit_for_bit(crf, dtype, V):
    """5. the same bits in both layouts, whatever the other utterances hold, for any K above k, across calls; other seeds and offsets
    give other paths."""
    N, T, K, blank = 3, 130, 5, 1
    x = make_x(N, T, V, DTYPES[dtype], seed=11)
    lx = [T, 100, 64]
    seed, offset = (1 << 64) - 3, (1 << 32) - 1
    base = run(crf, x, lx, K, seed, offset, blank)
    again = run(crf, x, lx, K, seed, offset, blank)
    tm = run(crf, x, lx, K, seed, offset, blank, time_major=True)
    for a, b, c in zip(base, again, tm):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # utterance 1 keeps its bits when the OTHER utterances' rows and lengths change (n enters the counter: same place in the call)
    x2 = make_x(N, T, V, DTYPES[dtype], seed=12)
    x2[1] = x[1]
    other = run(crf, x2, [7, 100, T], K, seed, offset, blank)
    for a, b in zip(base, other):
        assert np.array_equal(a[K:2 * K], b[K:2 * K])
    assert not np.array_equal(base[2][:K, :7], other[2][:K, :7])
    # K = 5 against the first five of K = 65
    big = run(crf, x, lx, 65, seed, offset, blank)
    for a, b in zip(base, big):
        assert np.array_equal(a, b.reshape((N, 65) + b.shape[1:])[:, :K].reshape(a.shape))
    for s2, o2 in ((seed - 1, offset), (seed, offset - 1), (seed ^ (1 << 40), offset)):
        assert not np.array_equal(base[2], run(crf, x, lx, K, s2, o2, blank)[2])
    check_draws(x, lx, K, seed, offset, blank, base[2])


def test_round_trip_through_ctc_score(crf):
    """6. the sampled hypotheses, moved to the CPU, are valid input of ctc_score: finite scores and invalid == 0 wherever lx > 0 (a
    collapsed path always fits its frames); the public call's outputs and hyp_utt."""
    N, T, V, K, blank = 4, 50, 20, 7, 3
    x = make_x(N, T, V, torch.float32, seed=3, neg_col=False).requires_grad_(True)
    lp = torch.log_softmax(x, -1)
    lx = _i32([T, 0, 17, 1])
    hyps, hl, utt, paths = crf.ctc_sample(lp, lx, K, 2024, offset=5, blank=blank, return_paths=True)
    for o in (hyps, hl, utt, paths):
        assert o.is_cuda and o.dtype == torch.int32 and not o.requires_grad
    assert hyps.shape == (N * K, T) and hl.shape == (N * K,) and paths.shape == (N * K, T)
    assert utt.cpu().tolist() == [h // K for h in range(N * K)]
    three = crf.ctc_sample(lp, lx, K, 2024, offset=5, blank=blank)
    assert len(three) == 3 and torch.equal(three[0], hyps) and torch.equal(three[1], hl)
    check_draws(lp.detach(), lx.tolist(), K, 2024, 5, blank, paths.cpu().numpy())
    check_collapse(paths.cpu().numpy(), hyps.cpu().numpy(), hl.cpu().numpy(), lx.tolist(), K, blank)
    scores, invalid = crf._C.ctc_score(lp.detach(), hyps.cpu(), hl.cpu(), lx, utt.cpu(), blank)
    scores, invalid = scores.cpu().numpy(), invalid.cpu().numpy()
    live = np.repeat(lx.numpy() > 0, K)
    assert np.all(invalid[live] == 0) and np.all(np.isfinite(scores[live])) and np.all(scores[live] < 0)
    assert np.all(invalid[~live] == 1)
    # the state of torch's generator is not touched
    st = torch.cuda.get_rng_state()
    crf.ctc_sample(lp, lx, K, 1)
    assert torch.equal(st, torch.cuda.get_rng_state())
