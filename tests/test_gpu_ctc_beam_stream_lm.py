"""GPU tests of the streaming beam search with an n-gram LM (ctc_beam_search_chunk(lm=...), include/ctc_crf_hip.h crf_ctc_beam_chunk with
tables).  The yardstick is the whole-utterance call ctc_beam_search(lm=...), held to tests/beam_lm_ref.py by tests/test_gpu_ctc_beam_lm.py;
every comparison is bit for bit: hyps[:len], hyp_lengths, fused scores, lm_scores and the chunks' traces one after the other.  Both calls
run the one frame step of cat_amd/csrc/k_beam_lm_body.h; the state's load and store, st_lds / na_lds rebuilt from it and the back-trace differ."""
import numpy as np
import pytest
import torch

from tests import beam_lm_ref, beam_ref, ngram_ref
from tests import beam_stream_ref as S
from tests.beam_stream_ref import DTYPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def check_splits(crf, x_cpu, lx, W, C, blank, dtype, splits, lm, alpha, beta, fused_modes=(False, True), what=""):
    """every split, both layouts, fuse_log_softmax on and off -> the whole call's dict (batch-major, the first fused mode)"""
    x = torch.tensor(x_cpu).to(DTYPES[dtype]).to(DEV)
    first = None
    for fused in fused_modes:
        for tm in (False, True):
            xin = x.transpose(0, 1).contiguous() if tm else x
            want = S.whole(crf, xin, lx, W, W, C, blank, tm, fused, lm=lm, alpha=alpha, beta=beta)
            first = first or want
            for split in splits:
                _, got = S.stream(crf, xin, lx, split, W, W, C, blank, tm, fused=fused, lm=lm, alpha=alpha, beta=beta)
                S.assert_same(got, want, blank, (what, dtype, tm, fused, split))
    return first


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("case", beam_lm_ref.LM_TIE_CASES, ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5])
def test_any_split_equals_whole_on_exact_ties_under_a_live_lm(crf, case, dtype):
    """beam_lm_ref.LM_TIE_CASES (values that bf16 holds, so one set for the three dtypes): exact ties of the fused scores at every level
    of the order; without fuse_log_softmax the result also equals beam_lm_ref.search."""
    seed, V, W, C, T, blank, G, order, alpha, beta, zero_group = case
    x, ng = beam_lm_ref.lm_tie_inputs(case)
    lm, ref = crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
    lxs = (T, T - 1, 1)
    want = check_splits(crf, np.stack([x] * 3), lxs, W, C, blank, dtype, S.splits_of(T, seed), lm, alpha, beta, what=str(case[:5]))
    for b, lx in enumerate(lxs):
        r = beam_lm_ref.search(x, lx, W, W, C, blank, ref, alpha, beta)
        assert np.array_equal(want["trace"][b], r["trace"]), (case, lx)
        for k in range(W):
            pre = r["nbest"][k][0] if k < len(r["nbest"]) else ()
            h = b * W + k
            assert want["len"][h] == len(pre) and tuple(want["hyps"][h, :len(pre)]) == pre, (case, lx, k)


def test_back_off_order_8_split_at_every_frame(crf):
    """beam_lm_ref.back_off_case(order=8): the LM state of the chain (0 .. 6) and its seven back-offs, carried across a chunk end at
    every frame: T chunks of 1 and every split into two."""
    for closed in (False, True):
        ng, x, (V, W, C, T, blank, alpha, beta) = beam_lm_ref.back_off_case(closed, 8)
        lm = crf.NgramLM.from_ngrams(ng, V)
        splits = [(1,) * T] + [(k, T - k) for k in range(1, T)]
        want = check_splits(crf, x, [T], W, C, blank, "fp32", splits, lm, alpha, beta, (False,), what=f"order 8 closed={closed}")
        assert want["len"][0] >= 7 and np.isfinite(want["lm"][0]) and want["lm"][0] != 0


@pytest.mark.parametrize("case", [beam_ref.REPLAY_CASES[1], beam_ref.REPLAY_CASES[5], beam_ref.TIE_CASES[2]], ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5])
def test_zero_weights_equal_the_lm_free_chunk_call(crf, case):
    """alpha = beta = 0: every output of every chunk call equals the LM-free chunk call's bit for bit, lm_scores are 0."""
    if len(case) == 7 and isinstance(case[5], tuple):
        seed, V, W, C, T, lxs, blank = case
        x = beam_ref.make_inputs(seed, len(lxs), T, V)
    else:
        seed, V, W, C, T, blank, groups = case
        x, lxs = np.stack([beam_ref.grouped_inputs(seed, T, V, blank, groups)] * 2), (T, T - 1)
    lm = crf.NgramLM.from_ngrams(ngram_ref.random_model(seed, V, 3), V)
    xd = torch.tensor(x, device=DEV)
    for split in S.splits_of(T, seed)[:4]:
        plain = []
        S.stream(crf, xd, lxs, split, W, W, C, blank, on_chunk=lambda j, seen, st, res: plain.append(res))

        def on_chunk(j, seen, st, res):
            for k in ("hyps", "len", "score", "trace"):
                assert np.array_equal(S.bits(res[k]), S.bits(plain[j][k])), (k, split, j)
            assert (res["lm"] == 0).all()
        S.stream(crf, xd, lxs, split, W, W, C, blank, lm=lm, alpha=0.0, beta=0.0, on_chunk=on_chunk)


def test_a_state_made_with_an_lm_continues_only_with_it(crf):
    V, W, C, blank = 6, 4, 5, 0
    x = torch.tensor(beam_ref.make_inputs(1, 2, 8, V), device=DEV)
    lm = crf.NgramLM.from_ngrams(ngram_ref.random_model(1, V, 2), V)
    other = crf.NgramLM.from_ngrams(ngram_ref.random_model(2, V, 2), V)
    state, _ = S.step(crf, x[:, :4].contiguous(), [4, 4], None, W, 1, C, blank, lm=lm, alpha=0.5, beta=0.25)
    with pytest.raises(RuntimeError, match="lm="):
        S.step(crf, x[:, 4:].contiguous(), [4, 4], state, W, 1, C, blank, lm=None)
    with pytest.raises(RuntimeError, match="lm="):
        S.step(crf, x[:, 4:].contiguous(), [4, 4], state, W, 1, C, blank, lm=other, alpha=0.5, beta=0.25)
    with pytest.raises(RuntimeError, match="alpha="):
        S.step(crf, x[:, 4:].contiguous(), [4, 4], state, W, 1, C, blank, lm=lm, alpha=0.75, beta=0.25)
    plain, _ = S.step(crf, x[:, :4].contiguous(), [4, 4], None, W, 1, C, blank)
    with pytest.raises(RuntimeError, match="lm="):
        S.step(crf, x[:, 4:].contiguous(), [4, 4], plain, W, 1, C, blank, lm=lm, alpha=0.5, beta=0.25)
    S.step(crf, x[:, 4:].contiguous(), [4, 4], state, W, 1, C, blank, lm=lm, alpha=0.5, beta=0.25)
