"""GPU tests of ctc_edit_distance (cat_amd/csrc/k_edit.hip, include/ctc_crf_hip.h crf_ctc_edit_distance): distance AND the three operation
counts equal the yardstick (tests/edit_ref.py: the contract's recursion with its tie rule, anti-diagonal NumPy form) exactly -- these are
integers -- over the reference lengths at which the kernel changes its rows per lane or goes over to strips, hypotheses shorter and longer
than the reference, alphabets of 2 and 3 symbols (ties and repeats everywhere) and of thousands, permuted hyp_utt, utterances without a
hypothesis, padding of any content, invalid rows, and the rows of ctc_beam_search / ctc_sample / ctc_greedy as they come."""
import numpy as np
import pytest
import torch

from tests import edit_ref

pytestmark = pytest.mark.gpu

REF_LENS = (0, 1, 63, 64, 65, 127, 128, 255, 256, 511, 512, 513, 1024, 2047)
HYP_LENS = (0, 1, 63, 64, 65, 300, 320)        # the last one is W itself
W_MATRIX = 320
STRIPS = "crf_ctc_edit_kernel<8, strips>"


@pytest.fixture(scope="module")
def mod():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


def yardstick(refs, hyps, utt):
    """[H][4] (dist, nsub, ndel, nins): one batch of the anti-diagonal form per utterance; -1 for rows given as None."""
    out = np.full((len(hyps), 4), -1, dtype=np.int64)
    for u in sorted({u for u, y in zip(utt, hyps) if y is not None}):
        rows = [h for h in range(len(hyps)) if utt[h] == u and hyps[h] is not None]
        out[rows] = edit_ref.antidiag_batch([refs[u]] * len(rows), [hyps[h] for h in rows])
    return out


def rows_of(hyps, W, fill):
    """(H, W) int32 CPU tensor: hypothesis h in front of row h, `fill(h, n)` -> n ints behind it; and the lengths."""
    t = torch.zeros((len(hyps), W), dtype=torch.int32)
    for h, y in enumerate(hyps):
        t[h, :len(y)] = torch.tensor(y, dtype=torch.int32)
        t[h, len(y):] = torch.as_tensor(np.asarray(fill(h, W - len(y)), dtype=np.int64).astype(np.int32))
    return t, torch.tensor([len(y) for y in hyps], dtype=torch.int32)


def call(mod, refs, rows, lens, utt, none_utt=False):
    """ctc_edit_distance with the counts -> [H][4] int64 numpy."""
    lab = torch.tensor([t for r in refs for t in r], dtype=torch.int32)
    ly = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    hu = None if none_utt else torch.tensor(utt, dtype=torch.int32).cuda()
    d, s, de, i = mod.ctc_edit_distance(rows.cuda(), lens.cuda(), lab, ly, hu, return_ops=True)
    for t in (d, s, de, i):
        assert t.is_cuda and t.dtype == torch.int32 and t.shape == (rows.size(0),) and not t.requires_grad
    only = mod.ctc_edit_distance(rows.cuda(), lens.cuda(), lab, ly, hu)
    assert torch.equal(only, d)                                                     # ops_dev NULL: the same distances
    return torch.stack([d, s, de, i], 1).cpu().numpy().astype(np.int64)


def related(rng, r, n, A):
    """A hypothesis of n tokens that follows the reference r with errors of all three kinds (a random one where r is empty)."""
    if len(r) == 0 or n == 0:
        return rng.integers(0, A, n).tolist()
    out, i = [], 0
    while len(out) < n:
        k = rng.random()
        if k < 0.7:
            out.append(int(r[i % len(r)])); i += 1
        elif k < 0.8:
            out.append(int(rng.integers(0, A))); i += 1
        elif k < 0.9:
            out.append(int(rng.integers(0, A)))
        else:
            i += 1
    return out


@pytest.fixture(scope="module")
def matrix():
    """Every reference length against every hypothesis length, per alphabet: (refs, hyps, utt, want), the yardstick computed once."""
    out = {}
    for A in (2, 3, 5000):
        rng = np.random.default_rng(A)
        refs = [rng.integers(0, A, R).tolist() for R in REF_LENS]
        pairs = [(u, Y) for u in range(len(refs)) for Y in HYP_LENS]
        utt = [u for u, _ in pairs]
        hyps = [related(rng, refs[u], Y, A) if k % 2 else rng.integers(0, A, Y).tolist() for k, (u, Y) in enumerate(pairs)]
        out[A] = (refs, hyps, utt, yardstick(refs, hyps, utt))
    return out


@pytest.mark.parametrize("A", [2, 3, 5000])
def test_every_length_pair(mod, matrix, A):
    refs, hyps, utt, want = matrix[A]
    assert len(hyps) == 98 and len(hyps) % 4 != 0
    rows, lens = rows_of(hyps, W_MATRIX, lambda h, n: np.full(n, -5))
    got = call(mod, refs, rows, lens, utt)
    assert mod._C.last_edit_kernel() == STRIPS
    assert np.array_equal(got, want), np.nonzero((got != want).any(1))[0]
    assert (got[:, 0] == got[:, 1:].sum(1)).all()
    R = np.array([len(refs[u]) for u in utt])
    assert ((R - got[:, 1] - got[:, 2]) == (lens.numpy() - got[:, 1] - got[:, 3])).all()          # the hits, counted on either side
    if A == 5000:                                                                    # tokens are int32 words, whatever their sign
        shift = lambda seqs: [[t - 2 ** 31 if t % 2 else t + 2 ** 30 for t in s] for s in seqs]
        rows2, _ = rows_of(shift(hyps), W_MATRIX, lambda h, n: np.full(n, 7))
        assert np.array_equal(call(mod, shift(refs), rows2, lens, utt), want)


def test_same_bits_in_any_order_batch_and_call(mod, matrix):
    """The list permuted, a second call, and the short references alone in another batch (other kernels): the same words per pair."""
    refs, hyps, utt, want = matrix[3]
    rows, lens = rows_of(hyps, W_MATRIX, lambda h, n: np.zeros(n))
    perm = np.random.default_rng(1).permutation(len(hyps))
    got = call(mod, refs, rows[perm], lens[perm], [utt[h] for h in perm])
    assert np.array_equal(got, want[perm])
    assert np.array_equal(call(mod, refs, rows[perm], lens[perm], [utt[h] for h in perm]), got)
    for nref, kernel in ((4, "crf_ctc_edit_kernel<1>"), (7, "crf_ctc_edit_kernel<2>"), (9, "crf_ctc_edit_kernel<4>"), (11, "crf_ctc_edit_kernel<8>")):
        keep = [h for h in range(len(hyps)) if utt[h] < nref]
        got = call(mod, refs[:nref], rows[keep], lens[keep], [utt[h] for h in keep])
        assert mod._C.last_edit_kernel() == kernel and len(refs[nref - 1]) == REF_LENS[nref - 1]
        assert np.array_equal(got, want[keep]), kernel


@pytest.mark.parametrize("max_ref,kernel", [(1, "<1>"), (64, "<1>"), (65, "<2>"), (128, "<2>"), (129, "<4>"), (256, "<4>"), (257, "<8>"),
                                            (512, "<8>"), (513, "<8, strips>"), (1025, "<8, strips>")])
def test_kernel_by_longest_reference(mod, max_ref, kernel):
    """The longest reference of the batch selects the rows per lane; hyp_utt permuted, utterance 2 owns no hypothesis, H = 7."""
    rng = np.random.default_rng(max_ref)
    A = 2 + max_ref % 2
    refs = [rng.integers(0, A, n).tolist() for n in (max_ref // 2, max_ref, min(9, max_ref), 0)]
    utt = [1, 3, 0, 1, 0, 3, 1]
    W = max_ref + 70
    lens = [max_ref + 70, 5, max_ref // 2, max(max_ref - 1, 0), 0, 66, max_ref]
    hyps = [related(rng, refs[u], n, A) for u, n in zip(utt, lens)]
    rows, hl = rows_of(hyps, W, lambda h, n: rng.integers(0, A, n))
    got = call(mod, refs, rows, hl, utt)
    assert mod._C.last_edit_kernel() == "crf_ctc_edit_kernel" + kernel
    assert np.array_equal(got, yardstick(refs, hyps, utt))


def test_long_hypotheses(mod):
    """Hypothesis rows of thousands of tokens: many blocks of 64 columns, against one strip, three strips and the register kernels."""
    rng = np.random.default_rng(8)
    refs = [rng.integers(0, 3, n).tolist() for n in (2047, 513, 40)]
    utt, lens = [0, 1, 2, 1, 2], [2047, 1500, 2047, 0, 129]
    hyps = [related(rng, refs[u], n, 3) for u, n in zip(utt, lens)]
    rows, hl = rows_of(hyps, 2047, lambda h, n: np.full(n, 1))
    want = yardstick(refs, hyps, utt)
    assert np.array_equal(call(mod, refs, rows, hl, utt), want) and mod._C.last_edit_kernel() == STRIPS
    got = call(mod, refs[2:], rows[[2, 4]], hl[[2, 4]], [0, 0])
    assert np.array_equal(got, want[[2, 4]]) and mod._C.last_edit_kernel() == "crf_ctc_edit_kernel<1>"


def test_padding_is_never_read(mod, matrix):
    """Behind hyp_len: the reference's own tokens (a kernel that read on would find matches), garbage, zeros -- one result."""
    refs, hyps, utt, want = matrix[2]
    big = np.random.default_rng(4).integers(-2 ** 31, 2 ** 31, (len(hyps), W_MATRIX))
    fills = (lambda h, n: np.resize(np.asarray(refs[utt[h]]), len(hyps[h]) + n)[len(hyps[h]):] if refs[utt[h]] else np.zeros(n),
             lambda h, n: big[h, :n], lambda h, n: np.zeros(n))
    for fill in fills:
        rows, lens = rows_of(hyps, W_MATRIX, fill)
        assert np.array_equal(call(mod, refs, rows, lens, utt), want)


def test_invalid_rows_take_minus_one_and_leave_their_neighbours(mod):
    rng = np.random.default_rng(6)
    for max_ref in (50, 600):
        refs = [rng.integers(0, 3, n).tolist() for n in (max_ref, 17, 0)]
        W = 90
        utt = [0, -1, 1, 3, 2, 0, 1, -2 ** 31, 2, 0, 2 ** 31 - 1]
        hyps = [related(rng, refs[u] if 0 <= u < 3 else [], n, 3) for u, n in zip(utt, (90, 10, 20, 20, 5, 0, 17, 3, 0, 64, 9))]
        rows, lens = rows_of(hyps, W, lambda h, n: np.full(n, 2))
        lens[6], lens[9] = -1, W + 1                                                  # lengths outside [0, W]
        bad = [1, 3, 6, 7, 9, 10]
        got = call(mod, refs, rows, lens, utt)
        want = yardstick(refs, [None if h in bad else y for h, y in enumerate(hyps)], [u if 0 <= u < 3 else 0 for u in utt])
        assert (want[bad] == -1).all() and (want[[0, 2, 4, 5, 8]] >= 0).all()
        assert np.array_equal(got, want)


def test_hyp_utt_none_empty_rows_and_no_hypotheses(mod):
    refs = [[1, 2, 3], [], [4, 4]]
    hyps = [[1, 3], [7], [4, 4]]
    rows, lens = rows_of(hyps, 4, lambda h, n: np.full(n, 9))
    assert call(mod, refs, rows, lens, [0, 1, 2], none_utt=True).tolist() == [[1, 0, 1, 0], [1, 0, 0, 1], [0, 0, 0, 0]]
    lab, ly = torch.tensor([1, 2, 3, 4, 4], dtype=torch.int32), torch.tensor([3, 0, 2], dtype=torch.int32)
    z = torch.zeros(3, dtype=torch.int32).cuda()
    d, s, de, i = mod.ctc_edit_distance(torch.zeros((3, 0), dtype=torch.int32).cuda(), z, lab, ly, return_ops=True)   # rows of width 0
    assert d.tolist() == [3, 0, 2] and de.tolist() == [3, 0, 2] and s.tolist() == i.tolist() == [0, 0, 0]
    d = mod.ctc_edit_distance(torch.zeros((0, 5), dtype=torch.int32).cuda(), z[:0], lab, ly, z[:0])
    assert d.shape == (0,) and d.is_cuda
    d = mod.ctc_edit_distance(rows.cuda(), lens.cuda(), lab.long(), ly.long())         # int64 labels, as the loss calls take them
    assert d.tolist() == [1, 1, 0]


def test_rows_of_the_decoders_go_straight_in(mod):
    """ctc_beam_search, ctc_sample and ctc_greedy on a small random input -> ctc_edit_distance, nothing copied to the host in between;
    the result equals the yardstick on the .cpu() lists, and summed errors over summed lengths is cal_wer's figure."""
    N, T, V, K = 5, 40, 7, 4
    gen = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(2.0 * torch.randn((N, T, V), generator=gen), -1).cuda()
    lx = torch.tensor([40, 33, 1, 17, 40], dtype=torch.int32)
    rng = np.random.default_rng(5)
    refs = [rng.integers(1, V, n).tolist() for n in (12, 0, 3, 9, 30)]
    lab = torch.tensor([t for r in refs for t in r], dtype=torch.int32)
    ly = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    for name, out in (("beam", mod.ctc_beam_search(lp, lx, beam_size=8, nbest=K)[:3]), ("sample", mod.ctc_sample(lp, lx, K, seed=11)),
                      ("greedy", mod.ctc_greedy(lp, lx) + (None,))):
        hyps, hl, hu = out
        d, s, de, i = mod.ctc_edit_distance(hyps, hl, lab, ly, hu, return_ops=True)
        H = hyps.size(0)
        utt = list(range(N)) if hu is None else hu.cpu().tolist()
        lists = [hyps[h, :int(hl[h])].cpu().tolist() for h in range(H)]
        want = yardstick(refs, lists, utt)
        got = torch.stack([d, s, de, i], 1).cpu().numpy()
        assert np.array_equal(got, want), name
        assert H == (N if name == "greedy" else N * K) and sum(len(y) for y in lists) > 0
        for h in (0, H - 1):
            assert tuple(want[h]) == edit_ref.loop(refs[utt[h]], lists[h])
        errors, ref_len = d.sum(), ly[torch.tensor(utt)].sum()                       # the two sums of get_wer
        assert int(errors) / int(ref_len) == edit_ref.wer(want[:, 0], [len(refs[u]) for u in utt])
    assert mod._C.last_edit_kernel() == "crf_ctc_edit_kernel<1>"
