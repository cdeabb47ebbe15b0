"""The yardstick of ngram_score and of NgramLM's end-of-sentence values (a plain helper module: tests/test_ngram_eos.py, the GPU tests of
ngram_score), on top of tests/ngram_ref.py's Ref, which ignores </s>: the textbook log P(</s> | history), the textbook length of the
n-gram that matches a token, and the score of a sequence -- in fp64 and natural logs, straight from the n-gram dict {tuple of tokens:
(log10 prob, log10 back-off)}.  It never looks at the compiled tables."""
from tests.ngram_ref import BOS, EOS, LN10, UNK, Ref


class ScoreRef(Ref):
    def __init__(self, ngrams, vocab_size, unk_logp=None):
        super().__init__(ngrams, vocab_size, unk_logp)
        # the </s> n-grams the model keeps aside: </s> last and only there, <s> first or nowhere, no <unk>
        self.eos = {tuple(k)[:-1]: float(v[0]) for k, v in ngrams.items()
                    if tuple(k)[-1] == EOS and EOS not in tuple(k)[:-1] and BOS not in tuple(k)[1:] and UNK not in tuple(k)}

    def _cut(self, history):
        return tuple(history)[-(self.order - 1):] if self.order > 1 else ()

    def has_eos(self):
        return () in self.eos

    def cond_eos(self, history):
        """log P(</s> | history): the longest h + </s> in the model, else the back-off weight of h (0 where h is no n-gram) and on."""
        h, acc = self._cut(history), 0.0
        while True:
            if h in self.eos:
                return acc + self.eos[h] * LN10
            assert h, "no </s> unigram"
            if h in self.ng:
                acc += self.ng[h][1] * LN10
            h = h[1:]

    def mass_eos(self, history):
        """The sum of the magnitudes of the terms cond_eos adds."""
        h, acc = self._cut(history), 0.0
        while True:
            if h in self.eos:
                return acc + abs(self.eos[h]) * LN10
            if h in self.ng:
                acc += abs(self.ng[h][1]) * LN10
            h = h[1:]

    def matched(self, history, c):
        """The tokens of the n-gram `cond` finds for c behind history: context tokens used (a <s> among them counts) plus 1; 1 for a
        unigram, also for a class that takes <unk>'s value."""
        h = self._cut(history)
        while h and h + (c,) not in self.ng:
            h = h[1:]
        return len(h) + 1

    def begin(self, bos):
        return self.start if bos else ()

    def score(self, tokens, bos=True, eos=False):
        """log P(tokens) from <s> (bos, where the model has it) or from the empty history, with eos plus log P(</s> | all of it)."""
        toks = tuple(int(c) for c in tokens)
        b = self.begin(bos)
        total = sum(self.cond(b + toks[:i], c) for i, c in enumerate(toks))
        return total + (self.cond_eos(b + toks) if eos else 0.0)

    def mass_score(self, tokens, bos=True, eos=False):
        toks = tuple(int(c) for c in tokens)
        b = self.begin(bos)
        return sum(self.mass(b + toks[:i], c) for i, c in enumerate(toks)) + (self.mass_eos(b + toks) if eos else 0.0)

    def orders(self, tokens, bos=True):
        toks = tuple(int(c) for c in tokens)
        b = self.begin(bos)
        return [self.matched(b + toks[:i], c) for i, c in enumerate(toks)]
