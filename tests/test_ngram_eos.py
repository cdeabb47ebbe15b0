"""CPU tests of the end-of-sentence values and the per-token values of cat_amd/ngram_lm.py: eos_logp against the textbook of
tests/ngram_score_ref.py (which reads the n-gram dict only), the tables untouched by </s> entries, score(eos=True), token_scores, and
every new error."""
import numpy as np
import pytest

from tests import ngram_ref
from tests.ngram_score_ref import ScoreRef

RTOL = 1e-6          # tests/test_ngram_lm.py's bound, relative to the sum of the magnitudes of the terms; eos_logp is an fp64 result
                     # rounded to fp32 once, so 2^-24 of that mass would do -- 1e-6 for uniformity
CASES = [(order, bos, unk) for order in (1, 2, 3, 4, 5) for bos in (True, False) for unk in (True, False)]


@pytest.fixture(scope="module")
def NgramLM():
    import ctc_crf
    return ctc_crf.NgramLM


def to_key(history):
    return tuple(history)


@pytest.mark.parametrize("order,bos,unk", CASES)
def test_eos_logp_against_the_textbook(NgramLM, order, bos, unk):
    V = 9
    ng = ngram_ref.random_model(11, V, order, bos=bos, unk=unk, eos=True)
    lm, ref = NgramLM.from_ngrams(ng, V), ScoreRef(ng, V)
    assert ref.has_eos() and lm.eos_logp is not None
    assert lm.eos_logp.dtype == np.float32 and lm.eos_logp.shape == (lm.num_states,) and np.isfinite(lm.eos_logp).all()
    assert order == 1 or len(ref.eos) > 1                         # (beyond the unigram: the longest match is exercised)
    for s in range(lm.num_states):
        h = to_key(lm.state_history[s])
        want = ref.cond_eos(h)
        assert abs(float(lm.eos_logp[s]) - want) <= RTOL * ref.mass_eos(h), (h, lm.eos_logp[s], want)


@pytest.mark.parametrize("order,bos,unk", CASES)
def test_eos_entries_leave_the_tables_alone(NgramLM, order, bos, unk):
    V = 9
    ng = ngram_ref.random_model(12, V, order, bos=bos, unk=unk, eos=True)
    bare = {k: v for k, v in ng.items() if ngram_ref.EOS not in k}
    assert len(bare) < len(ng)
    a, b = NgramLM.from_ngrams(ng, V), NgramLM.from_ngrams(bare, V)
    assert b.eos_logp is None and a.eos_logp is not None
    assert (a.order, a.num_states, a.num_arcs, a.start) == (b.order, b.num_states, b.num_arcs, b.start) and a.state_history == b.state_history
    for name in a.host_tables():
        x, y = a.host_tables()[name], b.host_tables()[name]
        assert x.dtype == y.dtype and np.array_equal(x.view(np.int32), y.view(np.int32)), name


@pytest.mark.parametrize("order,bos,unk", [(1, False, False), (3, True, True), (5, True, False)])
def test_arpa_round_trip_keeps_eos(NgramLM, tmp_path, order, bos, unk):
    V = 7
    ng = ngram_ref.random_model(13, V, order, bos=bos, unk=unk, eos=True)
    path = ngram_ref.write_arpa(ng, str(tmp_path / "lm.arpa"))
    a, b = NgramLM.from_arpa(path, V), NgramLM.from_ngrams(ng, V)
    assert np.array_equal(a.eos_logp.view(np.int32), b.eos_logp.view(np.int32))
    for name, t in a.host_tables().items():
        assert np.array_equal(t.view(np.int32), b.host_tables()[name].view(np.int32)), name


@pytest.mark.parametrize("order,bos,unk", CASES)
def test_score_with_eos_and_token_scores(NgramLM, order, bos, unk):
    V = 9
    ng = ngram_ref.random_model(14, V, order, bos=bos, unk=unk, eos=True)
    lm, ref = NgramLM.from_ngrams(ng, V), ScoreRef(ng, V)
    rng = np.random.default_rng(order)
    seqs = [[]] + [[int(c) for c in rng.integers(0, V, size=int(rng.integers(1, 14)))] for _ in range(40)]
    for seq in seqs:
        for eos in (False, True):
            got, want = lm.score(seq, eos=eos), ref.score(seq, True, eos)
            assert abs(got - want) <= RTOL * ref.mass_score(seq, True, eos) + 1e-30, (seq, eos, got, want)
        assert lm.score(seq) == lm.score(seq, eos=False)
        for with_bos in (True, False):
            lps, orders = lm.token_scores(seq, bos=with_bos) if not with_bos else lm.token_scores(seq)
            s, chain = lm.start if with_bos else 0, []
            for c in seq:                                         # lookup chained by hand
                lp, s = lm.lookup(s, c)
                chain.append(lp)
            assert lps == chain and orders == ref.orders(seq, with_bos), (seq, with_bos)
            assert all(1 <= m <= order for m in orders)
        if not seq:
            assert lm.score(seq, eos=True) == float(lm.eos_logp[lm.start]) and lm.token_scores(seq) == ([], [])
    assert sum(lm.token_scores(seqs[1])[0]) == lm.score(seqs[1])


def test_new_errors(NgramLM):
    base = {(0,): (-1.0, -0.5), (1,): (-0.5, -0.25), (0, 1): (-0.25, 0.0)}
    E = ngram_ref.EOS
    for bad, msg in (({**base, (E, 1): (-1.0, 0.0)}, r"</s> anywhere but last"),
                     ({**base, (0, E, E): (-1.0, 0.0)}, r"</s> anywhere but last"),
                     ({**base, (E,): (-1.0, 0.0), (0, E, 1): (-1.0, 0.0)}, r"inside a context"),
                     ({**base, (E,): (float("inf"), 0.0)}, r"non-finite"),
                     ({**base, (0, E): (float("nan"), 0.0)}, r"non-finite"),
                     ({**base, (E,): (-1.0, 0.0), (1, 1, E): (-1.0, 0.0)}, r"prefix of n-gram \(1, 1, '</s>'\) is absent")):
        with pytest.raises(ValueError, match=msg):
            NgramLM.from_ngrams(bad, 2)
    lm = NgramLM.from_ngrams(base, 2)
    assert lm.eos_logp is None
    with pytest.raises(ValueError, match=r"eos=True needs a model with a </s> unigram"):
        lm.score([0, 1], eos=True)
    assert lm.score([0, 1], eos=False) == lm.score([0, 1])
    # a </s> n-gram without the </s> unigram: no chain ends, no values
    assert NgramLM.from_ngrams({**base, (0, E): (-1.0, 0.0)}, 2).eos_logp is None


def test_eos_through_one_back_off_by_hand(NgramLM):
    """Three lines: after "0" the model has no "0 </s>", so log P(</s> | 0) = bow(0) + log P(</s>)."""
    ng = {(0,): (-1.0, -0.5), (ngram_ref.EOS,): (-2.0, 0.0), (0, 0): (-0.25, 0.0)}
    lm = NgramLM.from_ngrams(ng, 1)
    assert lm.order == 2 and lm.num_states == 2 and lm.state_history == [(), (0,)]
    want = np.array([-2.0 * ngram_ref.LN10, (-0.5 - 2.0) * ngram_ref.LN10]).astype(np.float32)
    assert np.array_equal(lm.eos_logp, want)
    assert lm.score([0], eos=True) == lm.lookup(0, 0)[0] + float(want[1])
    assert lm.token_scores([0, 0]) == ([lm.lookup(0, 0)[0], lm.lookup(1, 0)[0]], [1, 2])
