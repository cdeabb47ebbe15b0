"""GPU tests of the prefix beam search (ctc_crf.ctc_beam_search / crf_ctc_beam; cat_amd/csrc/k_beam.hip) against the fp64 yardstick
tests/beam_ref.py.

Tolerance on finite scores: rtol 1e-4, atol 0, as for the hypothesis scores (tests/test_gpu_ctc_score.py); inputs are log_softmax(normal
* 2), so no score lies near 0.  The search itself is held to the contract through `beam_ref.replay`: the GPU's own trace is followed
frame by frame in fp64, and no candidate it left out may beat one it took by more than RTOL |score| -- a near-tie decided the other way
in fp32 / fp64 passes, anything else does not, and an error in one frame does not excuse the next.  Every call runs batch-major AND
time-major with a poisoned workspace (0xFF); the two layouts must agree bit for bit.

Where replay cannot tell -- an exact tie counts as no excess whichever way it went -- the trace must EQUAL the reference's: one frame on
rows whose E_t is planted (beam_ref.planted_rows: the row stage's tie rules at V up to 8192) and inputs built to tie at every level of
the total order (beam_ref.TIE_CASES).  There the scores may lie anywhere, 0 included: they are single input values, or sums held to rtol."""
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
    """The seeded cases (tests/beam_ref.py REPLAY_CASES: V in {2, 3, 5, 9, 65, 72, 300}, W in {1, 2, 4, 16, 64}, C in {1, 8, 40, 64}, T in
    {1, 17, 64, 130, 150} and the narrow beams at V = 3, T = 30; ragged lx with 0 and 1; at W = 64 and T = 130 the back-trace takes three
    chunks of the 64-frame LDS buffer at its full width, lx = 128 ends on a chunk boundary, 65 is one frame past it): replay of the GPU's trace shows no unchosen candidate
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


KERNEL = {"fp32": "crf_beam_row_kernel<f32>", "bf16": "crf_beam_row_kernel<bf16>", "fp16": "crf_beam_row_kernel<f16>"}


def check_equals_search(ref, W, T, blank, hyps, lens, scores, trace, what):
    """One utterance whose trace must EQUAL the reference's (`ref` = beam_ref.search with nbest = W): trace words, label sequences, lengths
    word for word; the scores within RTOL, a missing rank at -inf."""
    assert np.array_equal(trace, ref["trace"]), (what, "trace", trace.tolist(), ref["trace"].tolist())
    for r in range(len(lens)):
        pre, want = ref["nbest"][r] if r < len(ref["nbest"]) else ((), -np.inf)
        assert lens[r] == len(pre) and tuple(hyps[r, :lens[r]]) == pre and (hyps[r, lens[r]:] == blank).all(), (what, r, hyps[r], pre)
        assert close(scores[r], want), (what, r, scores[r], want)
    assert not np.any(np.isnan(scores))


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("V", [64, 129, 4096, 4097, 8191, 8192])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_one_frame_trace_is_E_t(crf, dtype, V, C):
    """T = 1, W = 64: the trace of the one frame IS the row stage's E_t -- the stay of () and () + c for c in E_t, merged by value.  Rows:
    beam_ref.planted_rows (all of E_t in one column, equal values at v, v + 64 and v, v + 4096, a tie across the cut at place C, rows that
    are -inf but for a few classes, +0.0 / -0.0, the blank below everything so that all the places show, or on top) and three rows of
    2 normal through the dtype; the blank first and last.  V = 4096 is the last launch with four rows per workgroup (64 KiB of LDS), 4097
    the first with one, 8192 the widest row.  normalize = False: every score is ONE input value (pb = 0 and 0 (+) -inf = 0 exactly), so
    the trace row equals beam_ref.search's word for word, with its label sequences, and the scores are the values.  normalize = True:
    x^ - lse is rounded to fp32, so the classes of the extension words, in trace order, are the head of the reference's top_classes
    (exact), and the row is held to the contract by replay."""
    W, T = 64, 1
    rng = np.random.default_rng(V + C)
    noise = beam_ref.through(2.0 * rng.standard_normal((3, V)), dtype)
    for blank in (0, V - 1):
        planted = beam_ref.planted_rows(V, dtype, blank, C)
        for normalize in (False, True):
            named = [(n, r) for n, r in planted if not (normalize and n in beam_ref.PLANTED_LOGPROB_ONLY)] + [(f"normal{i}", r) for i, r in enumerate(noise)]
            x = np.stack([r for _, r in named])[:, None, :]
            xg = torch.tensor(x).to(DTYPES[dtype])
            assert np.array_equal(xg.float().numpy().view(np.int32), x.view(np.int32))
            hyps, lens, scores, trace = run(crf, xg.to("cuda:0"), [1] * len(named), W, W, C, blank, fused=normalize)
            assert crf_kernel_name() == KERNEL[dtype]
            for b, (name, row) in enumerate(named):
                what = f"V={V} C={C} {dtype} blank={blank} normalize={normalize} row={name}"
                x64 = x[b].astype(np.float64)
                if not normalize:
                    ref = beam_ref.search(x[b], 1, W, W, C, blank)
                    check_equals_search(ref, W, T, blank, hyps[b], lens[b], scores[b], trace[b], what)
                    for r, (pre, want) in enumerate(ref["nbest"]):
                        assert scores[b, r] == np.float32(want), (what, r)          # (one input value: the bits)
                else:
                    words = [int(w) for w in trace[b, 0] if w >= 0]
                    assert all(w & 63 == 0 for w in words), (what, words)
                    got = [(w >> 6) - 1 for w in words if w >> 6]
                    assert got == beam_ref.top_classes(x64[0], blank, min(C, V - 1))[:len(got)], (what, got)
                check_against_replay(x64, 1, W, C, blank, hyps[b], lens[b], scores[b], trace[b], normalize, what)


WIDE_LX9 = (6, 3, 0, 5, 1, 6, 2, 4, 6)


@pytest.mark.parametrize("fused", [False, True], ids=["logp", "fused"])
@pytest.mark.parametrize("blank_last", [False, True], ids=["blank0", "blankV-1"])
@pytest.mark.parametrize("W,C", [(16, 40), (64, 64)])
@pytest.mark.parametrize("V", [4096, 4097, 8192])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_wide_rows_replay(crf, dtype, V, W, C, blank_last, fused):
    """Rows of the widths the call was written for: V = 4096 (four rows per workgroup, 64 KiB of LDS), 4097 (one row per workgroup) and
    8192 (the widest), N = 3, T = 6, lx = (6, 3, 0), 2 normal through the dtype (log_softmax before the rounding where the call does not
    normalise): replay of the GPU's trace per utterance as in test_replay, both layouts bit for bit.  With W = 16 and the blank first the
    call is repeated with six more utterances (54 frames: the last workgroup of four rows has idle waves, as the one of 18 frames has):
    the first three utterances keep their bits."""
    T, lx, blank = 6, WIDE_LX9[:3], (V - 1 if blank_last else 0)
    rng = np.random.default_rng(V + W)
    raw = torch.tensor(2.0 * rng.standard_normal((9, T, V)), dtype=torch.float32)
    xc = (raw if fused else torch.log_softmax(raw, -1)).to(DTYPES[dtype])
    xg = xc.to("cuda:0")
    out = run(crf, xg[:3].contiguous(), lx, W, W, C, blank, fused=fused)
    assert crf_kernel_name() == KERNEL[dtype]
    x64 = xc[:3].double().numpy()
    worst = 0.0
    for b in range(3):
        what = f"V={V} W={W} C={C} {dtype} blank={blank} fused={fused}"
        rp = check_against_replay(x64[b], lx[b], W, C, blank, out[0][b], out[1][b], out[2][b], out[3][b], fused, what)
        assert [p for p in beam_ref.spell(out[3][b], lx[b], W)] == rp["prefixes"]
        worst = max(worst, rp["excess"])
    assert out[1][2, 0] == 0 and out[2][2, 0] == 0.0 and (out[2][2, 1:] == -np.inf).all()
    print(f"wide rows V={V} W={W} C={C} {dtype} blank={blank} fused={fused}: largest replay excess {worst:.3e}")
    if W == 16 and blank == 0:
        nine = run(crf, xg, WIDE_LX9, W, W, C, blank, fused=fused)
        for k in range(4):
            assert np.array_equal(nine[k][:3].view(np.int32), out[k].view(np.int32)), (V, dtype, fused, k)
        if V == 4096:
            x9 = xc.double().numpy()
            for b in (3, 8):
                check_against_replay(x9[b], WIDE_LX9[b], W, C, blank, nine[0][b], nine[1][b], nine[2][b], nine[3][b], fused, "nine")


@pytest.mark.parametrize("case", beam_ref.TIE_CASES, ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5])
def test_exact_ties_follow_the_total_order(crf, case):
    """beam_ref.TIE_CASES: inputs whose classes share one value per group and frame, so candidates tie EXACTLY, in fp64 and in the
    kernel's arithmetic alike, at every level of the contract's order and across the beam's edge, while no two candidates that do not
    tie come nearer than 1e-3 relative (tests/test_ctc_beam_api.py holds the cases to that).  replay counts a tie as no excess whichever
    way it went; here the GPU's trace, label sequences and lengths must EQUAL the reference's, at lx = T, T - 1 and 1: a stay that loses a
    tie to an extension, a higher slot that wins over a lower one, or class order in place of the place in E_t changes a trace word."""
    seed, V, W, C, T, blank, groups = case
    x = beam_ref.grouped_inputs(seed, T, V, blank, groups)
    lxs = (T, T - 1, 1)
    hyps, lens, scores, trace = run(crf, torch.tensor(np.stack([x] * 3), device="cuda:0"), lxs, W, W, C, blank)
    assert crf_kernel_name() == KERNEL["fp32"]
    for b, lx in enumerate(lxs):
        ref = beam_ref.search(x, lx, W, W, C, blank)
        check_equals_search(ref, W, T, blank, hyps[b], lens[b], scores[b], trace[b], f"{case} lx={lx}")
        assert (trace[b, lx:] == -1).all()


def minus_inf_inputs(V, dtype, normalize):
    """[N, 5, V] through the dtype with classes at -inf (log_softmax of the rows AFTER the -inf went in where the call does not normalise):
    utterance 0: a third of the classes at -inf in every frame, the blank at -inf in frame 2; 1: frame 1 with two classes and the blank
    above -inf (fewer than C), frame 3 with one class only, the blank at -inf; 2: frame 0 with the blank alone, frame 2 with fewer than C
    classes and the blank at -inf; 3 (normalize = False only): frame 2 entirely at -inf -- the beam dies there.  blank = 1."""
    T, blank = 5, 1
    rng = np.random.default_rng(V)
    raw = 2.0 * rng.standard_normal((4, T, V))
    raw[0][rng.random((T, V)) < 1 / 3] = -np.inf
    raw[0, :, 0] = 0.5                                           # (no frame of utterance 0 is empty)
    raw[0, 2, blank] = -np.inf
    keep = raw[1, 1, [0, blank, V - 1]].copy()
    raw[1, 1] = -np.inf
    raw[1, 1, [0, blank, V - 1]] = keep
    keep = raw[1, 3, V - 2]
    raw[1, 3] = -np.inf
    raw[1, 3, V - 2] = keep
    keep = raw[2, 0, blank]
    raw[2, 0] = -np.inf
    raw[2, 0, blank] = keep
    raw[2, 2, 3:] = -np.inf
    raw[2, 2, blank] = -np.inf
    x = torch.tensor(raw, dtype=torch.float32)
    if not normalize:
        x = torch.log_softmax(x, -1)
        x[3, 2] = -np.inf
    x = x[:4 if not normalize else 3].to(DTYPES[dtype])
    assert not torch.isnan(x).any()
    return x, blank


@pytest.mark.parametrize("normalize", [False, True], ids=["logp", "fused"])
@pytest.mark.parametrize("W", [4, 16])
@pytest.mark.parametrize("V", [6, 130])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_minus_inf_classes_and_dying_beams(crf, dtype, V, W, normalize):
    """A class at -inf never yields a candidate, in E_t or not, and the beam may hold fewer than W (include/ctc_crf_hip.h): rows with
    classes at -inf, with the blank at -inf, with fewer classes above -inf than C = min(40, V - 1) -- the row stage's filler pairs
    (class -1, -inf) -- and, with log-probs, a frame entirely at -inf, after which the beam is empty: every later trace row is -1 and
    every rank is missing (length 0, score -inf, a row of blanks).  Held to the contract by replay, the label sequences are the ones the
    trace spells, no score is NaN."""
    C, T = 40, 5
    xc, blank = minus_inf_inputs(V, dtype, normalize)
    N = xc.shape[0]
    lx = [5, 5, 4, 5][:N]
    hyps, lens, scores, trace = run(crf, xc.to("cuda:0"), lx, W, W, C, blank, fused=normalize)
    assert crf_kernel_name() == KERNEL[dtype] and not np.isnan(scores).any()
    x64 = xc.double().numpy()
    for b in range(N):
        what = f"V={V} W={W} {dtype} normalize={normalize} utterance {b}"
        rp = check_against_replay(x64[b], lx[b], W, C, blank, hyps[b], lens[b], scores[b], trace[b], normalize, what)
        assert [p for p in beam_ref.spell(trace[b], lx[b], W)] == rp["prefixes"], what
    # utterance 2, frame 0: the blank alone -- one slot, the stay of (); utterance 1, frame 3: one class and no blank -- every extension is
    # by that class, and a stay survives only on its repeat
    assert trace[2, 0].tolist() == [0] + [-1] * (W - 1)
    live = [int(w) for w in trace[1, 3] if w >= 0]
    assert live and all((w >> 6) - 1 in (-1, V - 2) for w in live) and any(w >> 6 for w in live)
    if not normalize:
        assert (trace[3, :2, 0] >= 0).all() and (trace[3, 2:] == -1).all()
        assert (lens[3] == 0).all() and (scores[3] == -np.inf).all() and (hyps[3] == blank).all()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_single_class_vocabulary(crf, dtype):
    """V = 1: the blank is the only class, C = min(top_classes, V - 1) = 0 -- no extension exists.  Rank 0 is the empty prefix with the
    sum of the blank's values, ranks 1 .. 3 are missing, the trace is [0, -1, -1, -1] in every live frame."""
    T, W = 3, 4
    x = beam_ref.through(-0.25 - np.random.default_rng(1).random((3, T, 1)), dtype)
    lx = (3, 1, 0)
    hyps, lens, scores, trace = run(crf, torch.tensor(x).to(DTYPES[dtype]).to("cuda:0"), lx, W, 4, 8, 0)
    assert crf_kernel_name() == KERNEL[dtype]
    for b, n in enumerate(lx):
        assert trace[b, :n].tolist() == [[0, -1, -1, -1]] * n and (trace[b, n:] == -1).all()
        assert (lens[b] == 0).all() and (hyps[b] == 0).all()
        assert close(scores[b, 0], x[b, :n, 0].astype(np.float64).sum()) and (scores[b, 1:] == -np.inf).all(), (b, scores[b])
        check_against_replay(x[b].astype(np.float64), n, W, 8, 0, hyps[b], lens[b], scores[b], trace[b], False, f"V=1 {dtype}")
