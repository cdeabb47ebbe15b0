"""GPU tests of the prefix beam search (ctc_crf.ctc_beam_search / crf_ctc_beam; cat_amd/csrc/k_beam.hip) against the fp64 yardstick
tests/beam_ref.py.

Tolerance on finite scores: rtol 1e-4, atol 0, as for the hypothesis scores (tests/test_gpu_ctc_score.py); inputs are log_softmax(normal
* 2), so no score lies near 0.  The search itself is held to the contract through `beam_ref.replay`: the GPU's own trace is followed
frame by frame in fp64, and no candidate it left out may beat one it took by more than RTOL |score| -- a near-tie decided the other way
in fp32 / fp64 passes, anything else does not, and an error in one frame does not excuse the next.  Every call runs batch-major AND
time-major with a poisoned workspace (0xFF); the two layouts must agree bit for bit."""
import numpy as np
import pytest
import torch

from tests import beam_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-4
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


def run(crf, x, lx, W, nbest, C, blank, fused=False):
    """x: [N,T,V] CUDA tensor, batch-major.  -> (hyps [N,nbest,T], lens [N,nbest], scores [N,nbest], trace [N,T,W]) as numpy, after checking
    that the two layouts agree bit for bit and that hyp_utt is h // nbest."""
    N, T, V = x.shape
    out = []
    for tm in (False, True):
        xin = x.transpose(0, 1).contiguous() if tm else x
        hyps, hl, hu, sc, tr = crf.ctc_beam_search(xin, _i32(lx), W, nbest, C, blank, tm, fused, return_trace=True)
        assert hyps.shape == (N * nbest, T) and hl.shape == (N * nbest,) and sc.shape == (N * nbest,) and tr.shape == (N, T, W)
        assert hyps.dtype == torch.int32 and hl.dtype == torch.int32 and sc.dtype == torch.float32 and tr.dtype == torch.int32
        assert torch.equal(hu.cpu(), torch.arange(N * nbest, dtype=torch.int32) // nbest)
        out.append((hyps.cpu().numpy().reshape(N, nbest, T), hl.cpu().numpy().reshape(N, nbest), sc.cpu().numpy().reshape(N, nbest),
                    tr.cpu().numpy()))
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the layouts differ"
    return out[0]


def close(got, want):
    if not np.isfinite(want):
        return got == want
    return np.isfinite(got) and abs(got - want) <= RTOL * abs(want)


def check_against_replay(x64, lx, W, C, blank, hyps, lens, scores, trace, normalize=False, what=""):
    """One utterance: x64 [T,V] the upcast activations; the outputs of its ranks (nbest of them) and its trace [T,W]."""
    T = x64.shape[0]
    lxc = max(0, min(int(lx), T))
    nbest = len(lens)
    assert (trace[lxc:] == -1).all(), (what, "trace rows past lx")
    rp = beam_ref.replay(x64, lx, trace, W, C, blank, normalize)
    print(f"{what} lx={lx}: replay excess {rp['excess']:.3e} {rp['why'] or ''}")
    assert rp["why"] is None and rp["excess"] <= RTOL, (what, lx, rp["excess"], rp["why"])
    assert not np.any(np.isnan(scores))
    for r in range(nbest):
        pre, want = rp["prefixes"][r], rp["scores"][r]
        assert close(scores[r], want), (what, lx, r, scores[r], want)
        if pre is None:
            assert lens[r] == 0 and scores[r] == -np.inf
            pre = ()
        assert lens[r] == len(pre) and tuple(hyps[r, :lens[r]]) == pre, (what, lx, r, hyps[r], pre)
        assert (hyps[r, lens[r]:] == blank).all(), (what, lx, r, "the tail is not the blank")
    assert all(scores[r] >= scores[r + 1] for r in range(nbest - 1)), (what, lx, scores)
    return rp


def count_prefixes(V, lx):
    """Label sequences over V - 1 labels that fit lx frames (length + repeats <= lx), the empty one included."""
    n = 0
    for L in range(lx + 1):
        for seq in np.ndindex(*([V - 1] * L)):
            n += L + sum(a == b for a, b in zip(seq, seq[1:])) <= lx
    return n


@pytest.mark.parametrize("V", [3, 4])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_exact_width(crf, V, dtype):
    """V = 3 and 4, T = 4 .. 6 (three utterances of one call), W = 64, C = V - 1, every blank, both layouts, both normalize values.  Where
    the beam holds every prefix -- at most 41 at V = 3, 61 at V = 4 and four frames -- the search is exact: the returned set of (label
    sequence, score) IS brute force over all V^T labellings, within RTOL.  At V = 4 and five or six frames there are more than 64 prefixes
    (105 and more): there the trace is held to the contract by replay and every score is bounded by brute force from above."""
    T, lx = 6, [4, 5, 6]
    exact = [count_prefixes(V, n) <= 64 for n in lx]
    assert exact == ([True] * 3 if V == 3 else [True, False, False])
    rng = np.random.default_rng(40 + V)
    raw = torch.tensor((2.0 * rng.standard_normal((3, T, V))).astype(np.float32))
    for normalize in (False, True):
        xc = (raw if normalize else torch.log_softmax(raw, -1)).to(DTYPES[dtype])
        x64 = xc.double().numpy()
        xg = xc.to("cuda:0")
        for blank in range(V):
            hyps, lens, scores, trace = run(crf, xg, lx, 64, 64, V - 1, blank, fused=normalize)
            for b in range(3):
                what = f"V={V} {dtype} normalize={normalize} blank={blank}"
                want = {k: v for k, v in beam_ref.brute(x64[b], lx[b], blank, normalize).items() if v > -np.inf}
                n = int((scores[b] > -np.inf).sum())
                got = {tuple(hyps[b, r, :lens[b, r]]): scores[b, r] for r in range(n)}
                assert len(got) == n, (what, "a label sequence twice")
                assert (scores[b, n:] == -np.inf).all() and (lens[b, n:] == 0).all() and (hyps[b, n:] == blank).all()
                assert all((hyps[b, r, lens[b, r]:] == blank).all() for r in range(n))
                if exact[b]:
                    assert set(got) == set(want), (what, lx[b], len(got), len(want))
                    for k, v in got.items():
                        assert close(v, want[k]), (what, lx[b], k, v, want[k])
                    assert all(scores[b, r] >= scores[b, r + 1] for r in range(63))
                else:
                    assert n == 64
                    check_against_replay(x64[b], lx[b], 64, V - 1, blank, hyps[b], lens[b], scores[b], trace[b], normalize, what)
                    for k, v in got.items():
                        assert v <= want[k] + RTOL * abs(want[k]), (what, lx[b], k, v, want[k])


@pytest.fixture(scope="module")
def case_outputs(crf):
    """Every seeded case once: (x fp32 numpy, outputs of run with nbest = W)."""
    out = {}
    for case in beam_ref.REPLAY_CASES:
        seed, V, W, C, T, lxs, blank = case
        x = beam_ref.make_inputs(seed, len(lxs), T, V)
        out[case] = (x, run(crf, torch.tensor(x, device="cuda:0"), lxs, W, W, C, blank))
    return out


@pytest.mark.parametrize("case", beam_ref.REPLAY_CASES, ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5])
def test_replay(case_outputs, case):
    """The seeded cases (tests/beam_ref.py REPLAY_CASES: V in {2, 3, 5, 65, 72, 300}, W in {1, 2, 4, 16, 64}, C in {1, 8, 40, 64}, T in
    {1, 17, 64, 150} and the narrow beams at V = 3, T = 30; ragged lx with 0 and 1): replay of the GPU's trace shows no unchosen candidate
    beating a chosen one by more than RTOL |score|, the GPU scores match replay's fp64 scores, hyps / hyp_lengths are the sequences the
    trace spells, ranks are in non-increasing score, trace rows past lx and empty slots hold -1."""
    seed, V, W, C, T, lxs, blank = case
    x, (hyps, lens, scores, trace) = case_outputs[case]
    assert crf_kernel_name() == "crf_beam_row_kernel<f32>"
    for b, lx in enumerate(lxs):
        rp = check_against_replay(x[b].astype(np.float64), lx, W, C, blank, hyps[b], lens[b], scores[b], trace[b], what=str(case[:5]))
        assert [p for p in beam_ref.spell(trace[b], lx, W)] == rp["prefixes"]
        if lx == 0:
            assert lens[b, 0] == 0 and scores[b, 0] == 0.0 and (scores[b, 1:] == -np.inf).all()


def crf_kernel_name():
    import ctc_crf
    return ctc_crf._C.last_beam_kernel()


@pytest.mark.parametrize("case", [c for c in beam_ref.REPLAY_CASES if c[1:5] in ((5, 16, 8, 64), (72, 16, 40, 150), (3, 4, 64, 30))],
                         ids=lambda c: "V%d-W%d-C%d-T%d" % c[1:5])
def test_scores_are_lower_bounds_of_ctc_score(crf, case_outputs, case):
    """A prefix's mass within the search is part of its full CTC likelihood: every finite returned score is <= ctc_score of that
    hypothesis, up to RTOL -- and the rows go into ctc_score as they are returned."""
    seed, V, W, C, T, lxs, blank = case
    x, (hyps, lens, scores, _) = case_outputs[case]
    N = len(lxs)
    hu = torch.arange(N * W, dtype=torch.int32) // W
    full = crf.ctc_score(torch.tensor(x, device="cuda:0"), torch.tensor(hyps.reshape(N * W, T)), torch.tensor(lens.reshape(-1)), _i32(lxs),
                         hu, blank=blank).cpu().numpy().reshape(N, W)
    seen = 0
    for b in range(N):
        for r in range(W):
            if np.isfinite(scores[b, r]) and lxs[b] > 0:
                assert np.isfinite(full[b, r]) and scores[b, r] <= full[b, r] + RTOL * abs(full[b, r]), (b, r, scores[b, r], full[b, r])
                seen += 1
    assert seen >= W


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_same_bits_across_calls_batches_widths_and_poison(crf, dtype):
    """The outputs of an utterance are the same bits in a second call, in a permuted batch, with fewer ranks asked for, and whatever the
    workspace held on entry (0xFF poison on and off) -- raw network output with normalize, all three dtypes, ties of 16-bit values included."""
    N, T, V, W, C, blank = 5, 70, 41, 16, 40, 3
    rng = np.random.default_rng(7)
    xg = torch.tensor((2.0 * rng.standard_normal((N, T, V))).astype(np.float32)).to(DTYPES[dtype]).to("cuda:0")
    lx = [70, 1, 33, 0, 69]
    first = run(crf, xg, lx, W, W, C, blank, fused=True)
    again = run(crf, xg, lx, W, W, C, blank, fused=True)
    crf._C.set_debug_poison(False)
    try:
        plain = run(crf, xg, lx, W, W, C, blank, fused=True)
    finally:
        crf._C.set_debug_poison(True)
    perm = [3, 0, 4, 2, 1]
    moved = run(crf, xg[perm].contiguous(), [lx[i] for i in perm], W, W, C, blank, fused=True)
    best = run(crf, xg, lx, W, 1, C, blank, fused=True)
    three = run(crf, xg, lx, W, 3, C, blank, fused=True)
    for k in range(4):
        assert np.array_equal(first[k].view(np.int32), again[k].view(np.int32))
        assert np.array_equal(first[k].view(np.int32), plain[k].view(np.int32))
        assert np.array_equal(first[k][perm].view(np.int32), moved[k].view(np.int32))
    for k in range(3):
        assert np.array_equal(first[k][:, :1].view(np.int32), best[k].view(np.int32))
        assert np.array_equal(first[k][:, :3].view(np.int32), three[k].view(np.int32))
    assert np.array_equal(first[3], best[3]) and np.array_equal(first[3], three[3])
    x64 = xg.cpu().double().numpy()
    for b in range(N):
        check_against_replay(x64[b], lx[b], W, C, blank, first[0][b], first[1][b], first[2][b], first[3][b], True, f"{dtype} fused")
    # eight classes of 40 per frame: which of several equal 16-bit values take part is the lower index's
    cut = run(crf, xg, lx, W, W, 8, blank, fused=True)
    for b in range(N):
        check_against_replay(x64[b], lx[b], W, 8, blank, cut[0][b], cut[1][b], cut[2][b], cut[3][b], True, f"{dtype} fused C=8")
