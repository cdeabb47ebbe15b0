"""GPU tests of the forward-only hypothesis scores (ctc_crf.ctc_score / crf_ctc_score, crf_ctc_score_logits; cat_amd/csrc/k_score.hip)
against the fp64 oracle (tests.util.oracle_blank) on the activations REPEATED per hypothesis on the host -- what the callers did before.

Tolerance on finite scores: rtol 1e-4, atol 0 (the project's TOL for numerator costs, tests/test_gpu_ctc_variants.py; the oracle's own fp32
arithmetic stays within 5.1e-6 of its fp64).  Inputs are log_softmax(normal * 2), so no score lies near 0.  Everywhere: -inf matches -inf
exactly, `invalid` is the complement of the oracle's `valid`, an invalid hypothesis scores -inf, and there is no NaN.  Every call writes
into a `scores` tensor prefilled with a sentinel and runs batch-major AND time-major; the two must agree bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests.guard import Arena
from tests.util import crf_env, log_softmax_np, oracle_blank

pytestmark = pytest.mark.gpu
RTOL = 1e-4
SENT = 12345.0
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# the instantiation a call takes, from its longest hypothesis (include/ctc_crf_hip.h): 64 NR states per wave, 512 NR per workgroup
KERNEL_OF_L = {31: "crf_ctc_score_wave_kernel<1>", 32: "crf_ctc_score_wave_kernel<2>", 63: "crf_ctc_score_wave_kernel<2>",
               64: "crf_ctc_score_wave_kernel<4>", 127: "crf_ctc_score_wave_kernel<4>", 128: "crf_ctc_score_wave_kernel<8>",
               255: "crf_ctc_score_wave_kernel<8>", 256: "crf_ctc_score_wg_kernel<2>", 600: "crf_ctc_score_wg_kernel<4>",
               2047: "crf_ctc_score_wg_kernel<8>"}
ALL_KERNELS = {f"crf_ctc_score_wave_kernel<{n}>" for n in (1, 2, 4, 8)} | {f"crf_ctc_score_wg_kernel<{n}>" for n in (2, 4, 8)}


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


def flat(hyps):
    return np.concatenate([np.asarray(h, dtype=np.int32) for h in hyps] + [np.zeros(0, dtype=np.int32)])


def reference(logp, hyps, hyp_utt, lx, blank):
    """(+log p [H] fp64, valid [H]) of the fp64 oracle on the rows of each hypothesis's utterance, repeated on the host.  logp: [N,T,V]
    log-probs (fp32 or fp64; the oracle reads fp32)."""
    hyp_utt = np.asarray(hyp_utt)
    rep = np.ascontiguousarray(np.asarray(logp)[hyp_utt])
    ly = np.array([len(h) for h in hyps], dtype=np.int32)
    _, cost, valid = oracle_blank(rep, flat(hyps), np.asarray(lx, dtype=np.int32)[hyp_utt], ly, blank)
    return cost, valid


def check(sc, inv, cost, valid, what=""):
    assert not np.any(np.isnan(sc)), (what, sc)
    assert np.array_equal(inv, 1 - valid), (what, inv, valid)
    for h in range(len(sc)):
        if not valid[h]:
            assert sc[h] == -np.inf, (what, h, sc[h])
        elif np.isinf(cost[h]):
            assert sc[h] == cost[h], (what, h, sc[h], cost[h])
        else:
            assert np.isfinite(sc[h]) and abs(sc[h] - cost[h]) <= RTOL * abs(cost[h]), (what, h, sc[h], cost[h])


def run(crf, x, hyps, hyp_utt, lx, blank, layouts=(False, True), fused=False, padded=False):
    """x: [N,T,V] CUDA tensor, batch-major.  -> (scores [H], invalid [H]) as numpy, after checking that the layouts agree bit for bit
    and that no sentinel is left."""
    H = len(hyps)
    hl = _i32([len(h) for h in hyps])
    if padded:
        lab = torch.full((H, max(1, int(hl.max())) + 2), blank, dtype=torch.int32)
        for h, a in enumerate(hyps):
            lab[h, :len(a)] = _i32(a)
    else:
        lab = _i32(flat(hyps))
    out = {}
    for tm in layouts:
        xx = x.transpose(0, 1).contiguous() if tm else x
        sc0 = torch.full((H,), SENT, dtype=torch.float32, device=x.device)
        sc, inv = crf._C.ctc_score(xx, lab, hl, _i32(lx), None if hyp_utt is None else _i32(hyp_utt), blank, tm, fused=fused, scores_out=sc0)
        assert sc.data_ptr() == sc0.data_ptr() and inv.dtype == torch.int32 and inv.shape == (H,)
        out[tm] = (sc.cpu().numpy(), inv.cpu().numpy())
        del xx
    sc, inv = out[layouts[0]]
    for tm in layouts[1:]:
        assert np.array_equal(sc.view(np.int32), out[tm][0].view(np.int32)) and np.array_equal(inv, out[tm][1]), ("layouts differ", sc, out[tm][0])
    assert not np.any(sc == SENT) and np.all((inv == 0) | (inv == 1))
    return sc, inv


# ---------------------------------------------------------------------------------------------------------------------------------
# the small batch of cases 1, 3 and 6
# ---------------------------------------------------------------------------------------------------------------------------------
N1, T1, V1 = 3, 48, 6
LX1 = np.array([48, 31, 9], dtype=np.int32)
_SMALL = {}


def small_batch(blank):
    """N = 3, ragged lx, (7, 0, 4) hypotheses per utterance in shuffled order: lengths 0, 1, 2, 5, 12, one with repeated labels, one
    with L <= lx < L + repeats, one longer than lx = 9.  Computed once per blank, shared and left unchanged."""
    if blank not in _SMALL:
        rng = np.random.default_rng(4100 + blank)
        pool = np.array([v for v in range(V1) if v != blank])
        draw = lambda n: pool[rng.integers(0, len(pool), size=n)].astype(np.int32)
        a, b, c, d = pool[:4]
        u0 = [draw(0), draw(1), draw(2), draw(5), draw(12), np.array([a, a, b, b, a], dtype=np.int32), draw(12)]
        u2 = [draw(2), draw(1),
              np.array([a, a, b, b, c, c, d, d], dtype=np.int32),     # 8 <= 9 < 8 + 4: invalid
              draw(12)]                                               # longer than lx = 9: invalid
        hyps, utt = u0 + u2, [0] * 7 + [2] * 4
        order = rng.permutation(len(hyps))
        hyps, utt = [hyps[i] for i in order], np.array([utt[i] for i in order])
        logp = log_softmax_np(rng.normal(0.0, 2.0, size=(N1, T1, V1))).astype(np.float32)
        cost, valid = reference(logp, hyps, utt, LX1, blank)
        assert valid.sum() == len(hyps) - 2 and np.all(np.isfinite(cost[valid == 1]))
        for v in (logp, cost, valid, utt):
            v.setflags(write=False)
        _SMALL[blank] = dict(logp=logp, hyps=hyps, utt=utt, cost=cost, valid=valid)
    return _SMALL[blank]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. parity, small
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, V1 - 1, 2])
def test_parity_small(crf, blank):
    c = small_batch(blank)
    x = torch.tensor(c["logp"]).to("cuda:0")
    sc, inv = run(crf, x, c["hyps"], c["utt"], LX1, blank)
    check(sc, inv, c["cost"], c["valid"], blank)
    assert crf._C.last_score_kernel() == "crf_ctc_score_wave_kernel<1>"
    sc2, inv2 = run(crf, x, c["hyps"], c["utt"], LX1, blank, padded=True)       # the padded (H, Lmax) form
    assert np.array_equal(sc.view(np.int32), sc2.view(np.int32)) and np.array_equal(inv, inv2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. geometry boundaries: every NR of both geometries
# ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_table_covers_every_instantiation():
    assert set(KERNEL_OF_L.values()) == ALL_KERNELS


@pytest.mark.parametrize("L", sorted(KERNEL_OF_L))
def test_geometry_boundaries(crf, L):
    rng = np.random.default_rng(4200 + L)
    T, V, blank = 2 * L + 12, 5, 0
    pool = np.arange(1, V)
    hyps = [pool[rng.integers(0, len(pool), size=n)].astype(np.int32) for n in (L, 1, 0)]
    logp = log_softmax_np(rng.normal(0.0, 2.0, size=(1, T, V))).astype(np.float32)
    lx, utt = np.array([T]), np.zeros(3, dtype=np.int64)
    cost, valid = reference(logp, hyps, utt, lx, blank)
    assert np.all(valid == 1)
    sc, inv = run(crf, torch.tensor(logp).to("cuda:0"), hyps, utt, lx, blank)
    assert crf._C.last_score_kernel() == KERNEL_OF_L[L]
    check(sc, inv, cost, valid, L)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. bits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bits(crf):
    blank = 2
    c = small_batch(blank)
    hyps, utt = c["hyps"], c["utt"]
    x = torch.tensor(c["logp"]).to("cuda:0")
    bits = lambda a: a.view(np.int32)
    sc, inv = run(crf, x, hyps, utt, LX1, blank)                     # (batch-major against time-major: inside run)
    check(sc, inv, c["cost"], c["valid"])
    sc_b, inv_b = run(crf, x, hyps, utt, LX1, blank)                 # the same call twice
    assert np.array_equal(bits(sc), bits(sc_b)) and np.array_equal(inv, inv_b)
    perm = np.random.default_rng(43).permutation(len(hyps))          # the list permuted
    sc_p, inv_p = run(crf, x, [hyps[i] for i in perm], utt[perm], LX1, blank)
    assert np.array_equal(bits(sc_p), bits(sc[perm])) and np.array_equal(inv_p, inv[perm])
    first = np.nonzero(utt == 0)[0]                                  # the first utterance's hypotheses alone: same tensor, then its rows only
    assert max(len(hyps[i]) for i in first) == max(len(h) for h in hyps)
    sc_f, inv_f = run(crf, x, [hyps[i] for i in first], utt[first], LX1, blank)
    assert np.array_equal(bits(sc_f), bits(sc[first])) and np.array_equal(inv_f, inv[first])
    sc_1, inv_1 = run(crf, x[:1].contiguous(), [hyps[i] for i in first], utt[first], LX1[:1], blank)
    assert np.array_equal(bits(sc_1), bits(sc[first])) and np.array_equal(inv_1, inv[first])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. dead and sharp inputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [0, 3])
def test_dead_columns(crf, blank):
    """Every frame admits ONE class: exactly one alignment is left (the score is the sum of its entries), and with one more -inf none
    (score -inf, invalid 0)."""
    V = 5
    a, b = [v for v in range(V) if v != blank][:2]
    path = [a, blank, a, b, blank, b, blank]            # collapses to (a, a, b, b)
    hyp = np.array([a, a, b, b], dtype=np.int32)
    T = len(path)
    rng = np.random.default_rng(44)
    one = np.full((1, T, V), -np.inf, dtype=np.float32)
    one[0, np.arange(T), path] = np.log(rng.uniform(0.2, 0.9, size=T)).astype(np.float32)
    none = one.copy()
    none[0, 3, b] = -np.inf
    logp = np.concatenate([one, none])
    hyps, utt, lx = [hyp, hyp, np.array([a], dtype=np.int32)], np.array([0, 1, 0]), np.array([T, T])
    cost, valid = reference(logp, hyps, utt, lx, blank)
    assert np.all(valid == 1) and np.isfinite(cost[0]) and cost[1] == -np.inf and cost[2] == -np.inf
    assert abs(cost[0] - one[0, np.arange(T), path].astype(np.float64).sum()) < 1e-9
    sc, inv = run(crf, torch.tensor(logp).to("cuda:0"), hyps, utt, lx, blank)
    check(sc, inv, cost, valid)
    assert sc[1] == -np.inf and sc[2] == -np.inf and np.all(inv == 0)


def test_sharp_inputs(crf):
    rng = np.random.default_rng(45)
    N, T, V, blank = 2, 120, 8, 0
    logp = log_softmax_np(rng.normal(0.0, 40.0, size=(N, T, V))).astype(np.float32)
    lx = np.array([120, 97])
    hyps = [rng.integers(1, V, size=n).astype(np.int32) for n in (0, 3, 17, 30, 40, 9, 31)]
    hyps.append(np.array([int(np.argmax(logp[1, t])) for t in range(0, 97, 2)], dtype=np.int32))    # follows the peaks (blanks dropped below)
    hyps[-1] = hyps[-1][hyps[-1] != blank]
    utt = np.array([0, 1, 0, 1, 0, 1, 0, 1])
    cost, valid = reference(logp, hyps, utt, lx, blank)
    assert np.all(valid == 1)
    sc, inv = run(crf, torch.tensor(logp).to("cuda:0"), hyps, utt, lx, blank)
    check(sc, inv, cost, valid)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. raw network output
# ---------------------------------------------------------------------------------------------------------------------------------
def raw_reference(x, hyps, utt, lx, blank):
    """The oracle on the fp64 log_softmax of the exact upcast of x ([N,T,V] tensor of any of the three dtypes)."""
    return reference(log_softmax_np(x.float().cpu().numpy().astype(np.float64)), hyps, utt, lx, blank)


@pytest.mark.parametrize("V", [7, 300])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_raw_output(crf, dtype, V):
    """V = 7: rows of 16-bit elements start on 2-byte boundaries only; V = 300: the wide lse kernel.  The workspace is filled with 0xFF
    (set_debug_poison): the lse values of frames at or past lx would read as NaN."""
    rng = np.random.default_rng(4500 + V)
    N, T, blank = 3, 40, 4
    lx = np.array([40, 23, 31])
    pool = np.array([v for v in range(V) if v != blank])
    hyps = [pool[rng.integers(0, len(pool), size=n)].astype(np.int32) for n in (12, 0, 5, 1, 30, 8)]
    utt = np.array([2, 0, 0, 2, 2, 0])                             # (utterance 1 owns none; L = 30 fits lx = 31 only without repeats)
    x = torch.tensor(rng.normal(0.0, 2.0, size=(N, T, V)).astype(np.float32)).to(DTYPES[dtype]).to("cuda:0")
    cost, valid = raw_reference(x, hyps, utt, lx, blank)
    sc, inv = run(crf, x, hyps, utt, lx, blank, fused=True)
    check(sc, inv, cost, valid, (dtype, V))
    assert valid.sum() >= 5


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. guard bands
# ---------------------------------------------------------------------------------------------------------------------------------
def run_guarded(core, x, hyps, utt, lx, blank, fused, time_major, null_invalid, misalign=0):
    """One call of the C ABI with every buffer carved from a 0xFF arena (64 KiB bands), the workspace exactly as large as the library
    asks.  -> (scores, invalid or None) as numpy after the bands were checked."""
    dev = torch.device("cuda", 0)
    B, T, V = (x.shape[1], x.shape[0], x.shape[2]) if time_major else x.shape
    H = len(hyps)
    hl = _i32([len(h) for h in hyps])
    off = torch.cumsum(hl, 0, dtype=torch.int32) - hl
    lab = _i32(flat(hyps))
    nws = core._lib.crf_ctc_score_logits_workspace_bytes(B, T, V) if fused else 0
    assert nws >= 0
    meta = (("labels", lab), ("hyp_off", off), ("hyp_len", hl), ("hyp_utt", _i32(utt)), ("lx", _i32(lx)))
    nbytes = x.numel() * x.element_size()
    arena = Arena(dev, Arena.room([nbytes] + [4 * t.numel() for _, t in meta] + [4 * H, 4 * H, nws]))
    arena.carve("act", nbytes, misalign=misalign)
    arena.put("act", x)
    for name, t in meta:
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    arena.carve("score", 4 * H)
    arena.put("score", torch.full((H,), SENT, dtype=torch.float32))
    if not null_invalid:
        arena.carve("invalid", 4 * H)
    sections = None
    if fused:
        arena.carve("ws", nws)
        sections = [("lse", 0, 4 * B * T)]
    P, vp = arena.ptr, ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    tail = (1 if time_major else 0, blank, P("labels"), P("hyp_off"), P("hyp_len"), P("hyp_utt"), P("lx"), B, H, T, V, int(hl.max()), P("score"),
            vp(0) if null_invalid else P("invalid"))
    with torch.cuda.device(dev):
        if fused:
            rc = core._lib.crf_ctc_score_logits(P("act"), DTYPES_ID[x.dtype], *tail, P("ws"), nws, stream)
        else:
            rc = core._lib.crf_ctc_score(P("act"), *tail, stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check(sections)
    if fused:
        assert bool((arena.view("ws")[:4 * B * T] != 0xFF).any()), "the call did not use the carved workspace"
    assert torch.equal(arena.get("act", torch.uint8), x.contiguous().reshape(-1).view(torch.uint8)), "the call wrote to its input"
    sc = arena.get("score", torch.float32).numpy()
    inv = None if null_invalid else arena.get("invalid", torch.int32).numpy()
    assert not np.any(sc == SENT)
    return sc, inv


DTYPES_ID = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def test_guard_bands_log_probs(crf):
    """crf_ctc_score, time-major, invalid_dev = NULL; one hypothesis more with a label outside [0, V) (the binding would refuse it)."""
    blank = 2
    c = small_batch(blank)
    hyps = list(c["hyps"]) + [np.array([0, V1, 1], dtype=np.int32)]
    utt = np.concatenate([c["utt"], [1]])
    x = torch.tensor(c["logp"]).transpose(0, 1).contiguous()
    sc, inv = run_guarded(crf._C, x, hyps, utt, LX1, blank, fused=False, time_major=True, null_invalid=True)
    assert inv is None and sc[-1] == -np.inf
    check(sc[:-1], 1 - c["valid"], c["cost"], c["valid"])           # (no invalid vector in this call: -inf where the oracle says invalid)
    assert np.array_equal(np.isinf(sc[:-1]), c["valid"] == 0)


def test_guard_bands_raw_bf16_misaligned(crf):
    """crf_ctc_score_logits on bf16 rows that start 2 bytes past a multiple of 256, with a gap of 256 bytes behind the lse section."""
    blank = 2
    c = small_batch(blank)
    rng = np.random.default_rng(46)
    x = torch.tensor(rng.normal(0.0, 2.0, size=(N1, T1, V1)).astype(np.float32)).to(torch.bfloat16)
    cost, valid = raw_reference(x, c["hyps"], c["utt"], LX1, blank)
    with crf_env(CRF_WS_GAP=1):
        need = crf._C._lib.crf_ctc_score_logits_workspace_bytes(N1, T1, V1)
        assert need >= 4 * N1 * T1 + 256
        sc, inv = run_guarded(crf._C, x, c["hyps"], c["utt"], LX1, blank, fused=True, time_major=False, null_invalid=False, misalign=2)
    check(sc, inv, cost, valid)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. one long case
# ---------------------------------------------------------------------------------------------------------------------------------
def test_long_case(crf):
    rng = np.random.default_rng(47)
    T, V, blank = 1500, 72, 0
    logp = log_softmax_np(rng.normal(0.0, 2.0, size=(1, T, V))).astype(np.float32)
    hyps = [rng.integers(1, V, size=n).astype(np.int32) for n in (250, 250, 20, 0)]
    utt, lx = np.zeros(4, dtype=np.int64), np.array([T])
    cost, valid = reference(logp, hyps, utt, lx, blank)
    assert np.all(valid == 1)
    sc, inv = run(crf, torch.tensor(logp).to("cuda:0"), hyps, utt, lx, blank)
    assert crf._C.last_score_kernel() == "crf_ctc_score_wave_kernel<8>"
    check(sc, inv, cost, valid)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_surface(crf):
    rng = np.random.default_rng(48)
    N, T, V, blank = 4, 50, 9, 3
    logp = log_softmax_np(rng.normal(0.0, 2.0, size=(N, T, V))).astype(np.float32)
    lx = torch.tensor([50, 41, 33, 50], dtype=torch.int32)
    hl = torch.tensor([7, 0, 12, 20], dtype=torch.int32)
    pool = np.array([v for v in range(V) if v != blank])
    padded = torch.tensor(pool[rng.integers(0, len(pool), size=(N, 20))], dtype=torch.int32)      # (N, Lmax), as nn.CTCLoss takes targets
    want = -torch.nn.functional.ctc_loss(torch.tensor(logp).double().transpose(0, 1), padded.long(), lx.long(), hl.long(), blank=blank,
                                         reduction="none").numpy()
    assert np.all(np.isfinite(want))
    x = torch.tensor(logp).to("cuda:0")
    # hyp_utt=None: hypothesis h on utterance h = -F.ctc_loss(reduction='none')
    got = crf.ctc_score(x, padded, hl, lx, blank=blank)
    assert got.device == x.device and got.dtype == torch.float32 and got.shape == (N,)
    g = got.cpu().numpy()
    assert not np.any(np.isnan(g)) and np.all(np.abs(g - want) <= RTOL * np.abs(want)), (g, want)
    # time-major, as nn.CTCLoss takes the activations: the same bits
    got_tm = crf.ctc_score(x.transpose(0, 1).contiguous(), padded, hl, lx, blank=blank, time_major=True)
    assert torch.equal(got_tm, got)
    # no autograd history, even for an input that requires grad
    xg = x.clone().requires_grad_(True)
    r = crf.ctc_score(xg, padded, hl, lx, blank=blank)
    assert r.requires_grad is False and r.grad_fn is None and torch.equal(r, got)
    # a non-default stream: enqueued there, right after that stream's synchronise
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x2 = torch.tensor(logp).to("cuda:0", non_blocking=False)
        r2 = crf.ctc_score(x2, padded, hl, lx, blank=blank)
    s.synchronize()
    assert torch.equal(r2.cpu(), got.cpu())
    # raw output through the public name
    raw = torch.tensor(rng.normal(0.0, 2.0, size=(N, T, V)).astype(np.float32)).to(torch.float16).to("cuda:0")
    w16 = -torch.nn.functional.ctc_loss(torch.log_softmax(raw.cpu().double(), -1).transpose(0, 1), padded.long(), lx.long(), hl.long(),
                                        blank=blank, reduction="none").numpy()
    g16 = crf.ctc_score(raw, padded, hl, lx, blank=blank, fuse_log_softmax=True).cpu().numpy()
    assert np.all(np.abs(g16 - w16) <= RTOL * np.abs(w16)), (g16, w16)
