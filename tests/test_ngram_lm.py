"""CPU tests of cat_amd/ngram_lm.py: the compiled tables against the textbook back-off lookup of tests/ngram_ref.py (which reads the n-gram
dict only), the ARPA reader on files written by ngram_ref.write_arpa, and every malformed-file error with its line number."""
import numpy as np
import pytest

from tests import ngram_ref

RTOL = 1e-6          # the tables hold fp32 values and the walk adds them in fp32: 2^-24 relative per term, at most order + 1 terms --
                     # of a look-up relative to the sum of the terms' magnitudes (ngram_ref.Ref.mass): a back-off weight above 0 cancels
                     # against the values below 0 (order 8, history (7 0 7 5 0 2), class 3: the terms sum to -0.017), and one rounding of
                     # every value plus at most 8 rounded sums are 9 * 2^-24 = 5.4e-7 of that mass


@pytest.fixture(scope="module")
def NgramLM():
    import ctc_crf
    return ctc_crf.NgramLM


def history_of(lm, s):
    return tuple(lm.state_history[s])


@pytest.mark.parametrize("bos,unk", [(True, False), (False, True), (True, True), (False, False)])
@pytest.mark.parametrize("order", [1, 2, 3, 5, 8])
def test_tables_against_the_textbook(NgramLM, order, bos, unk):
    """For every state and every token lm.lookup equals the textbook value from that state's history within 1e-6 relative, and the next
    state is the longest kept suffix of history + token; the tables have the promised shape; score() of random sequences matches."""
    V = 9
    ng = ngram_ref.random_model(4, V, order, bos=bos, unk=unk, eos=True)
    lm, ref = NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
    assert lm.order == ref.order == order and lm.vocab_size == V
    S, A = lm.num_states, lm.num_arcs
    assert lm.row_off.shape == (S + 1,) and lm.row_off[0] == 0 and lm.row_off[1] == 0 and lm.row_off[-1] == A
    assert lm.arc_label.shape == lm.arc_logp.shape == lm.arc_next.shape == (A,) and lm.bo_state.shape == lm.bo_weight.shape == (S,)
    assert lm.uni_logp.shape == lm.uni_next.shape == (V,)
    assert all(np.isfinite(getattr(lm, n)).all() for n in ("arc_logp", "bo_weight", "uni_logp"))
    assert lm.state_history[0] == () and all(lm.bo_state[s] < s for s in range(1, S)) and lm.bo_state[0] == 0
    assert [len(h) for h in lm.state_history] == sorted(len(h) for h in lm.state_history) and max(len(h) for h in lm.state_history) <= max(order - 1, 0)
    assert set(lm.state_history[1:]) == {k for k in ref.ng if len(k) < order and k != (ngram_ref.UNK,)}
    assert history_of(lm, lm.start) == ref.known_suffix(ref.start)       # (the state of <s>; the root where the model has none, or order 1)
    for s in range(S):
        row = lm.arc_label[lm.row_off[s]:lm.row_off[s + 1]]
        assert (np.diff(row) > 0).all()
        h = history_of(lm, s)
        assert history_of(lm, lm.bo_state[s]) == ref.known_suffix(h[1:]) if s else True
        for c in range(V):
            lp, nx = lm.lookup(s, c)
            want = ref.cond(h, c)
            assert abs(lp - want) <= RTOL * ref.mass(h, c), (h, c, lp, want)
            assert order > 5 or abs(lp - want) <= RTOL * abs(want), (h, c, lp, want)     # (the narrower bound the models up to order 5 also meet)
            assert history_of(lm, nx) == ref.known_suffix(h + (c,)), (h, c, history_of(lm, nx))
    rng = np.random.default_rng(order)
    for _ in range(50):
        seq = [int(c) for c in rng.integers(0, V, size=int(rng.integers(0, 12)))]
        want = ref.score(seq)
        assert abs(lm.score(seq) - want) <= RTOL * sum(abs(ref.cond(ref.start + tuple(seq[:i]), c)) for i, c in enumerate(seq)) + 1e-30, seq


def test_dict_forms_and_missing_unigrams(NgramLM):
    """Numeric strings are classes; a class without a unigram takes <unk>'s value, else unk_logp, else construction fails and names it."""
    ng = {("0",): (-1.0, -0.5), (1,): (-0.5, 0.0), ("0", "1"): (-0.25, 0.0)}
    with pytest.raises(ValueError, match=r"class 2 has no unigram"):
        NgramLM.from_ngrams(ng, 3)
    lm = NgramLM.from_ngrams(ng, 3, unk_logp=-3.0)
    assert abs(lm.lookup(0, 2)[0] + 3.0 * ngram_ref.LN10) < 1e-6 and lm.start == 0 and lm.order == 2
    assert abs(lm.score([0, 1]) - (-1.25 * ngram_ref.LN10)) < 1e-6
    lm = NgramLM.from_ngrams({**ng, ("<unk>",): (-2.0, 0.0)}, 3, unk_logp=-3.0)      # the model's own <unk> wins
    assert abs(lm.lookup(0, 2)[0] + 2.0 * ngram_ref.LN10) < 1e-6
    for bad, msg in (({(0,): (float("nan"), 0.0)}, "non-finite"), ({(0,): (-1.0, 0.0), (0, 0, 0): (-1.0, 0.0)}, "prefix"),
                     ({(5,): (-1.0, 0.0)}, r"token 5 outside \[0, vocab_size=1\)"), ({tuple(range(1)) * 9: (-1.0, 0.0)}, "order 9")):
        with pytest.raises(ValueError, match=msg):
            NgramLM.from_ngrams(bad, 1)
    with pytest.raises(TypeError):
        NgramLM()


@pytest.mark.parametrize("order,bos,unk", [(1, False, False), (3, True, True), (5, True, False), (8, True, True)])
def test_arpa_round_trip(NgramLM, tmp_path, order, bos, unk):
    """The model read back from a written file has the tables of the model built from the dict, bit for bit; </s> entries are dropped."""
    V = 7
    ng = ngram_ref.random_model(6, V, order, bos=bos, unk=unk, eos=True)
    path = ngram_ref.write_arpa(ng, str(tmp_path / "lm.arpa"))
    a, b = NgramLM.from_arpa(path, V), NgramLM.from_ngrams(ng, V)
    assert (a.order, a.num_states, a.num_arcs, a.start) == (b.order, b.num_states, b.num_arcs, b.start) and a.state_history == b.state_history
    for name, t in a.host_tables().items():
        assert np.array_equal(t.view(np.int32), b.host_tables()[name].view(np.int32)), name
    ref = ngram_ref.Ref(ng, V)
    assert abs(a.score([1, 2, 3, 1]) - ref.score([1, 2, 3, 1])) <= 1e-5 * abs(ref.score([1, 2, 3, 1]))


def test_order_nine_is_refused(NgramLM, tmp_path):
    """MAX_ORDER = 8 is the largest order (the kernel's walk is bounded by it): a chain of 8 tokens with its prefixes builds and walks
    seven sparse rows, the same chain with its 9-gram raises in from_ngrams, and a file with a 9-gram section raises at that section's
    line, whatever the section holds."""
    import cat_amd.ngram_lm
    assert cat_amd.ngram_lm.MAX_ORDER == 8
    V = 3
    ng = {(c,): (-0.5, -0.25) for c in range(V)}
    for n in range(2, 9):
        ng[(0, 1) * (n // 2) + (0,) * (n % 2)] = (-0.125 * n, -0.5 if n < 8 else 0.0)
    lm = NgramLM.from_ngrams(ng, V)
    assert lm.order == 8 and max(len(h) for h in lm.state_history) == 7
    ref = ngram_ref.Ref(ng, V)
    seq = [0, 1, 0, 1, 0, 1, 0, 1, 2, 0, 1]
    assert abs(lm.score(seq) - ref.score(seq)) <= RTOL * sum(abs(ref.cond(tuple(seq[:i]), c)) for i, c in enumerate(seq))
    nine = {**ng, (0, 1, 0, 1, 0, 1, 0, 1): (-1.0, -0.5), (0, 1, 0, 1, 0, 1, 0, 1, 0): (-1.0, 0.0)}
    with pytest.raises(ValueError, match=r"NgramLM: order 9 above 8"):
        NgramLM.from_ngrams(nine, V)
    path = ngram_ref.write_arpa(nine, str(tmp_path / "nine.arpa"))
    header = 1 + open(path).read().split("\n").index("\\9-grams:")
    assert NgramLM.from_arpa(ngram_ref.write_arpa(ng, str(tmp_path / "eight.arpa")), V).order == 8
    with pytest.raises(ValueError, match=rf"nine\.arpa: line {header}: order 9 above 8"):
        NgramLM.from_arpa(path, V)


GOOD = ["\\data\\", "ngram 1=4", "ngram 2=2", "", "\\1-grams:", "-99\t<s>\t-0.3", "-1.0\t0\t-0.5", "-0.7\t1\t-0.2", "-1.5\t</s>", "", "\\2-grams:",
        "-0.3\t<s> 1", "-0.4\t0 1", "", "\\end\\"]


def _write(tmp_path, lines):
    p = tmp_path / "bad.arpa"
    p.write_text("\n".join(lines) + "\n")
    return str(p)


def test_malformed_files_raise_with_the_line_number(NgramLM, tmp_path):
    lm = NgramLM.from_arpa(_write(tmp_path, GOOD), 2)
    assert lm.order == 2 and lm.num_arcs == 2 and lm.state_history[lm.start] == ("<s>",)
    assert abs(lm.lookup(lm.start, 1)[0] + 0.3 * ngram_ref.LN10) < 1e-6

    def edit(i, text):
        return [text if k == i else l for k, l in enumerate(GOOD)]

    cases = [
        (edit(2, "ngram 2=3"), r"line 11: the 2-gram section holds 2 n-grams, its count line says 3"),
        (edit(1, "ngram 1=3"), r"line 5: the 1-gram section holds 4 n-grams, its count line says 3"),
        (edit(12, "-0.4\t1 0 1 0"), r"line 13: a 2-gram line has 3 or 4 fields, got 5"),
        (edit(11, "-0.3\t<s> 2"), r"line 12: token 2 outside \[0, vocab_size=2\)"),
        (edit(7, "-0.7\t-1\t-0.2"), r"line 8: token -1 outside"),
        (edit(6, "nan\t0\t-0.5"), r"line 7: non-finite number"),
        (edit(6, "-1.0\t0\t-inf"), r"line 7: non-finite number"),
        (edit(6, "-1.0\tzero\t-0.5"), r"line 7: token 'zero'"),
        (edit(7, "-0.7\t0\t-0.2"), r"line 8: n-gram \(0,\) twice"),
        (GOOD[:-1], r"no \\end\\ line"),
    ]
    for lines, msg in cases:
        with pytest.raises(ValueError, match=msg):
            NgramLM.from_arpa(_write(tmp_path, lines), 2)
    # an n-gram whose (n - 1)-token prefix is absent: "1 0" needs the unigram "1"
    lines = [l for l in GOOD if l != "-0.7\t1\t-0.2"]
    lines[1], lines[lines.index("-0.3\t<s> 1")] = "ngram 1=3", "-0.3\t1 0"
    with pytest.raises(ValueError, match=r"prefix of n-gram \(1, 0\) is absent \(line 11\)"):
        NgramLM.from_arpa(_write(tmp_path, lines), 2, unk_logp=-5.0)
