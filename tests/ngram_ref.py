"""The yardstick of cat_amd/ngram_lm.py (a plain helper module: tests/test_ngram_lm.py, tests/beam_lm_ref.py, the GPU tests of the fused
beam search): the textbook back-off lookup straight from the n-gram dict {tuple of tokens: (log10 prob, log10 back-off)} -- the longest
match, else bow(h) + p(c | h[1:]) -- in fp64 and natural logs.  It never looks at the compiled tables.  Also a seeded generator of random
models (prefix-closed, NOT suffix-closed: pruned contexts), of models whose values depend on the groups of the tokens only (the exact-tie
cases of the fused beam search), and an ARPA writer for them."""
import itertools
import math

import numpy as np

BOS, EOS, UNK = "<s>", "</s>", "<unk>"
LN10 = math.log(10.0)


def clean(ngrams):
    """The n-grams the model keeps: none with </s>, none with <s> behind the first place, none of order >= 2 with <unk>."""
    out = {}
    for k, v in ngrams.items():
        k = tuple(k)
        if EOS in k or BOS in k[1:] or (UNK in k and len(k) > 1):
            continue
        out[k] = (float(v[0]), float(v[1]))
    return out


class Ref:
    def __init__(self, ngrams, vocab_size, unk_logp=None):
        self.ng = clean(ngrams)
        self.V = vocab_size
        self.order = max(len(k) for k in self.ng if k != (UNK,))
        self.unk = self.ng[(UNK,)][0] if (UNK,) in self.ng else unk_logp
        self.start = (BOS,) if (BOS,) in self.ng else ()
        self._memo = {(): 0.0}

    def cond(self, history, c):
        """log P(c | history) in natural log: the longest match, else the back-off weight of the context (0 where it has none) and on."""
        h = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        acc = 0.0
        while True:
            if h + (c,) in self.ng:
                return acc + self.ng[h + (c,)][0] * LN10
            if not h:
                assert self.unk is not None, c
                return acc + self.unk * LN10
            if h in self.ng:
                acc += self.ng[h][1] * LN10
            h = h[1:]

    def mass(self, history, c):
        """The sum of the magnitudes of the terms `cond` adds (back-off weights and the value found): what bounds the rounding of an
        fp32 sum of them -- positive back-off weights and negative values can cancel, and the result alone does not."""
        h = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        acc = 0.0
        while True:
            if h + (c,) in self.ng:
                return acc + abs(self.ng[h + (c,)][0]) * LN10
            if not h:
                return acc + abs(self.unk) * LN10
            if h in self.ng:
                acc += abs(self.ng[h][1]) * LN10
            h = h[1:]

    def score(self, tokens):
        """log P(tokens) from the start history (<s> where the model has it), no end-of-sentence term; memoised by prefix."""
        tokens = tuple(int(c) for c in tokens)
        if tokens not in self._memo:
            self._memo[tokens] = self.score(tokens[:-1]) + self.cond(self.start + tokens[:-1], tokens[-1])
        return self._memo[tokens]

    def known_suffix(self, history):
        """The longest suffix of `history` of at most order - 1 tokens that is a kept n-gram (the state a walk must be in)."""
        h = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        while h and h not in self.ng:
            h = h[1:]
        return h


def random_model(seed, V, order, bos=True, unk=False, eos=False, fanout=3, keep=0.6):
    """A random model as a dict: unigrams for every class (with unk: for about two thirds of them, and <unk>), then per order n = 2 .. N a
    random part `keep` of the (n - 1)-grams as contexts with up to `fanout` successors each -- every n-gram's prefix is in the model, its
    suffix mostly is not.  Random log10 values in [-3, -0.1] and back-offs in [-1, 0.2].  eos: </s> entries, which the model must drop."""
    rng = np.random.default_rng([seed, V, order])
    val = lambda: (round(float(-0.1 - 2.9 * rng.random()), 4), round(float(-1.0 + 1.2 * rng.random()), 4))
    ng = {}
    for c in range(V):
        if not unk or rng.random() < 2 / 3 or c == 0:
            ng[(c,)] = val()
    if unk:
        ng[(UNK,)] = (val()[0], 0.0)
    if bos:
        ng[(BOS,)] = (-99.0, val()[1])
    if eos:
        ng[(EOS,)] = (val()[0], 0.0)
    level = [k for k in ng if k not in ((UNK,), (EOS,))]
    for n in range(2, order + 1):
        nxt = []
        for ctx in level:
            if rng.random() > keep and nxt:
                continue
            for c in rng.choice(V, size=min(V, 1 + int(rng.integers(fanout))), replace=False):
                k = ctx + (int(c),)
                ng[k] = val() if n < order else (val()[0], 0.0)
                nxt.append(k)
            if eos and rng.random() < 0.3:
                ng[ctx + (EOS,)] = (val()[0], 0.0)
        level = nxt
    return ng


def symmetric_model(seed, V, group, G, order, bos=True, zero_group=None, fanout=3, keep=0.6):
    """A model over V classes whose values depend on the GROUPS of an n-gram's tokens only (group [V]: the group in [0, G) of every
    class): a random prefix-closed model over the G group symbols as `random_model` draws one, every group n-gram expanded to all class
    n-grams of those groups with its (log10 p, log10 bow).  Two token sequences that differ by a permutation inside the groups then take
    the same n-grams' values in the same order: bit-equal log P and bit-equal look-ups, in the textbook and in the compiled tables alike.
    zero_group = g: log10 p = 0.0 for every n-gram whose last token is of group g -- found without a back-off, an extension by such a
    class costs alpha * 0.0 = +0 exactly."""
    rng = np.random.default_rng([seed, V, G, order])
    val = lambda: (round(float(-0.1 - 2.9 * rng.random()), 4), round(float(-1.0 + 1.2 * rng.random()), 4))
    gm = {(g,): val() for g in range(G)}
    if bos:
        gm[(BOS,)] = (-99.0, val()[1])
    level = list(gm)
    for n in range(2, order + 1):
        nxt = []
        for ctx in level:
            if rng.random() > keep and nxt:
                continue
            for g in rng.choice(G, size=min(G, 1 + int(rng.integers(fanout))), replace=False):
                k = ctx + (int(g),)
                gm[k] = val() if n < order else (val()[0], 0.0)
                nxt.append(k)
        level = nxt
    members = [[c for c in range(V) if group[c] == g] for g in range(G)]
    ng = {}
    for k, (lp, bo) in gm.items():
        if zero_group is not None and k[-1] == zero_group:
            lp = 0.0
        for toks in itertools.product(*[[BOS] if g == BOS else members[g] for g in k]):
            ng[toks] = (lp, bo)
    return ng


def write_arpa(ngrams, path, counts=None):
    """The dict as ARPA text (what lmplz --arpa writes); counts: other count lines than the true ones, for the malformed cases."""
    order = max(len(k) for k in ngrams)
    by = {n: sorted((k for k in ngrams if len(k) == n), key=lambda k: tuple(str(w) for w in k)) for n in range(1, order + 1)}
    with open(path, "w") as f:
        f.write("\\data\\\n")
        for n in range(1, order + 1):
            f.write(f"ngram {n}={(counts or {}).get(n, len(by[n]))}\n")
        for n in range(1, order + 1):
            f.write(f"\n\\{n}-grams:\n")
            for k in by[n]:
                lp, bo = ngrams[k]
                f.write(f"{lp!r}\t{' '.join(str(w) for w in k)}" + (f"\t{bo!r}\n" if n < order else "\n"))
        f.write("\n\\end\\\n")
    return path
