"""cat_amd/ngram_lm.py -- a token-level back-off n-gram language model for ctc_beam_search(lm=...): read from the ARPA text that
``lmplz --arpa`` writes over token indices (cat/utils/pipeline/ngram.sh) or given as a dict, and compiled to the state tables that
crf_ctc_beam_lm walks on the device (include/ctc_crf_hip.h crf_ngram_tables).

    lm = NgramLM.from_arpa("lm.arpa", vocab_size=V)
    hyps, hl, hu, scores = ctc_beam_search(log_probs, lx, beam_size=16, lm=lm, alpha=0.5, beta=1.0)

Tokens: the string "17" is class 17; "<s>", "</s>" and "<unk>" are the only non-numeric tokens.  Values are log10 in the file and in the
dict, natural logs in the tables (converted in fp64, stored in fp32).  Dropped: n-grams that hold "<s>" anywhere but first, and n-grams of
order >= 2 that contain "<unk>".  N-grams that end in "</s>" enter no table: they are kept aside and resolved into eos_logp (below); a
"</s>" anywhere but last raises.  A class in [0, vocab_size) without a unigram takes <unk>'s unigram value, or unk_logp (log10) where the
model has no <unk>.

Tables (numpy, one set per model): the states are the empty history (state 0, the root) and every kept n-gram of order 1 .. N - 1, sorted
by history length (so bo_state[s] < s for s > 0); row s of the arcs is arc_*[row_off[s] .. row_off[s + 1]) with arc_label ascending; the
root's row is dense (uni_logp[V], uni_next[V]) and its sparse row empty; arc_next of h + c is the longest suffix of h + c of at most N - 1
tokens that is a state; bo_state[s] is the longest proper suffix of s that is a state, bo_weight[s] the model's back-off weight of s (0
where it gives none); start is the state of "<s>", or the root.

The end-of-sentence values: eos_logp[s] = log P(</s> | history of s) in natural log, float32 [S], or None where the model has no "</s>"
unigram -- resolved here in fp64 by the textbook rule (the longest h + </s> in the model; otherwise the back-off weight of h where h is in
the model, and on without h's oldest token, down to the "</s>" unigram) and rounded to fp32 once: ngram_score(eos=True) and
score(tokens, eos=True) add one entry per hypothesis, without a walk.  A "</s>" n-gram whose context is longer than order - 1 tokens is
the context of no state and is never reached.

Not covered: an end-of-sentence term in the search (it is in ngram_score, not in the search), word-level LMs and lexicons, KenLM's binary
formats, an LM in ctc_sample."""
import ctypes
import math
from typing import Dict, Optional, Tuple

import numpy as np

BOS, EOS, UNK = "<s>", "</s>", "<unk>"
MAX_ORDER = 8
LN10 = math.log(10.0)
_BOS_ID = -1                # <s> inside a history tuple


class _Tables(ctypes.Structure):
    """include/ctc_crf_hip.h crf_ngram_tables"""
    _fields_ = [("row_off", ctypes.c_void_p), ("arc_label", ctypes.c_void_p), ("arc_logp", ctypes.c_void_p), ("arc_next", ctypes.c_void_p),
                ("bo_state", ctypes.c_void_p), ("bo_weight", ctypes.c_void_p), ("uni_logp", ctypes.c_void_p), ("uni_next", ctypes.c_void_p),
                ("S", ctypes.c_int64), ("A", ctypes.c_int64), ("V", ctypes.c_int64), ("order", ctypes.c_int32), ("start", ctypes.c_int32)]


TABLE_NAMES = ("row_off", "arc_label", "arc_logp", "arc_next", "bo_state", "bo_weight", "uni_logp", "uni_next")


def _where(lines, key):
    return f" (line {lines[key]})" if lines and key in lines else ""


class NgramLM:
    """A compiled back-off n-gram model over the classes [0, vocab_size).  Build with from_arpa or from_ngrams."""

    def __init__(self):
        raise TypeError("use NgramLM.from_arpa or NgramLM.from_ngrams")

    # ---- construction ----
    @classmethod
    def from_ngrams(cls, ngrams: Dict[tuple, Tuple[float, float]], vocab_size: int, unk_logp: Optional[float] = None, _lines=None) -> "NgramLM":
        """ngrams: {tuple of tokens: (log10 prob, log10 back-off)}; a token is an int class or one of "<s>", "</s>", "<unk>" (numeric
        strings are taken as ints)."""
        V = int(vocab_size)
        if V < 1:
            raise ValueError(f"NgramLM: vocab_size must be positive, got {vocab_size}")
        kept, unk, eos_ng = {}, None, {}
        for key, val in ngrams.items():
            key = tuple(key)
            at = _where(_lines, key)
            if not key:
                raise ValueError("NgramLM: an empty n-gram")
            if len(key) > MAX_ORDER:
                raise ValueError(f"NgramLM: order {len(key)} above {MAX_ORDER}{at}")
            lp, bo = float(val[0]), float(val[1])
            if not (math.isfinite(lp) and math.isfinite(bo)):
                raise ValueError(f"NgramLM: non-finite number in n-gram {key}{at}")
            toks = []
            for w in key:
                if isinstance(w, str) and w not in (BOS, EOS, UNK):
                    try:
                        w = int(w)
                    except ValueError:
                        raise ValueError(f"NgramLM: token {w!r} is neither a class index nor <s>, </s>, <unk>{at}") from None
                if not isinstance(w, str):
                    w = int(w)
                    if not 0 <= w < V:
                        raise ValueError(f"NgramLM: token {w} outside [0, vocab_size={V}){at}")
                toks.append(w)
            if EOS in toks[:-1]:
                raise ValueError(f"NgramLM: </s> anywhere but last (inside a context) in n-gram {key}{at}")
            if BOS in toks[1:]:
                continue
            if toks[-1] == EOS:                 # kept aside: no table holds it (eos_logp below)
                if UNK not in toks:
                    eos_ng[tuple(_BOS_ID if w == BOS else w for w in toks[:-1])] = lp * LN10
                continue
            if UNK in toks:
                if len(toks) == 1:
                    unk = lp * LN10
                continue
            kept[tuple(_BOS_ID if w == BOS else w for w in toks)] = (lp * LN10, bo * LN10)
        for key in kept:
            if len(key) > 1 and key[:-1] not in kept:
                shown = tuple(BOS if w == _BOS_ID else w for w in key)
                raise ValueError(f"NgramLM: the prefix of n-gram {shown} is absent{_where(_lines, shown)}")
        for ctx in eos_ng:
            if ctx and ctx not in kept:
                shown = tuple(BOS if w == _BOS_ID else w for w in ctx) + (EOS,)
                raise ValueError(f"NgramLM: the prefix of n-gram {shown} is absent{_where(_lines, shown)}")
        if unk is None and unk_logp is not None:
            if not math.isfinite(float(unk_logp)):
                raise ValueError(f"NgramLM: unk_logp must be finite, got {unk_logp}")
            unk = float(unk_logp) * LN10
        order = max([len(k) for k in kept] + [1])
        states = sorted((k for k in kept if len(k) < order), key=lambda k: (len(k), k))
        index = {(): 0}
        for k in states:
            index[k] = len(index)
        S = len(index)

        def longest_state(h):
            h = tuple(h)[-(order - 1):] if order > 1 else ()
            while h not in index:
                h = h[1:]
            return index[h]

        uni_logp, uni_next = np.zeros(V, np.float64), np.zeros(V, np.int32)
        for c in range(V):
            if (c,) in kept:
                uni_logp[c] = kept[(c,)][0]
                uni_next[c] = index.get((c,), 0)
            elif unk is not None:
                uni_logp[c] = unk
            else:
                raise ValueError(f"NgramLM: class {c} has no unigram, and the model has neither <unk> nor unk_logp")
        rows = [[] for _ in range(S)]
        for key, (lp, _) in kept.items():
            if len(key) >= 2:
                rows[index[key[:-1]]].append((key[-1], lp, longest_state(key)))
        row_off = np.zeros(S + 1, np.int32)
        label, logp, nxt = [], [], []
        for s, row in enumerate(rows):
            row.sort()
            for c, lp, n in row:
                label.append(c), logp.append(lp), nxt.append(n)
            row_off[s + 1] = len(label)
        bo_state, bo_weight = np.zeros(S, np.int32), np.zeros(S, np.float64)
        for k, s in index.items():
            if s:
                bo_state[s] = longest_state(k[1:]) if order > 1 else 0
                bo_weight[s] = kept[k][1]
        self = object.__new__(cls)
        self.vocab_size, self.order, self.num_states, self.num_arcs = V, order, S, len(label)
        self.start = index.get((_BOS_ID,), 0)
        self.row_off, self.arc_label = row_off, np.asarray(label, np.int32)
        self.arc_logp, self.arc_next = np.asarray(logp, np.float64).astype(np.float32), np.asarray(nxt, np.int32)
        self.bo_state, self.bo_weight = bo_state, bo_weight.astype(np.float32)
        self.uni_logp, self.uni_next = uni_logp.astype(np.float32), uni_next
        self.state_history = [tuple(BOS if w == _BOS_ID else w for w in k) for k in index]   # per state, for inspection
        self._checked = False
        self._device = {}
        self.eos_logp = None
        if () in eos_ng:                        # log P(</s> | history of s) per state: fp64, one rounding to fp32
            eos = np.zeros(S, np.float64)
            for k, s in index.items():
                h, acc = k, 0.0
                while h not in eos_ng:          # (ends at the </s> unigram)
                    if h in kept:
                        acc += kept[h][1]
                    h = h[1:]
                eos[s] = acc + eos_ng[h]
            self.eos_logp = eos.astype(np.float32)
        for name in ("arc_logp", "bo_weight", "uni_logp") + (("eos_logp",) if self.eos_logp is not None else ()):
            if not np.isfinite(getattr(self, name)).all():
                raise ValueError(f"NgramLM: {name} does not fit fp32")
        return self

    @classmethod
    def from_arpa(cls, path: str, vocab_size: int, unk_logp: Optional[float] = None) -> "NgramLM":
        """Read an ARPA file of token-id n-grams.  A malformed file raises ValueError with the line number."""
        counts, ngrams, lines = {}, {}, {}
        section, seen, header_line, in_data = 0, 0, 0, False

        def bad(n, msg):
            return ValueError(f"{path}: line {n}: {msg}")

        def close_section(n):
            if section and seen != counts.get(section):
                raise bad(header_line, f"the {section}-gram section holds {seen} n-grams, its count line says {counts.get(section)}")

        ended = False
        with open(path) as f:
            for n, raw in enumerate(f, 1):
                line = raw.strip()
                if not line:
                    continue
                if line == "\\data\\":
                    in_data = True
                    continue
                if line == "\\end\\":
                    close_section(n)
                    ended, section = True, 0
                    break
                if line.startswith("\\") and line.endswith("-grams:"):
                    close_section(n)
                    try:
                        section = int(line[1:-len("-grams:")])
                    except ValueError:
                        raise bad(n, f"bad section header {line!r}") from None
                    if section not in counts:
                        raise bad(n, f"section {line!r} has no count line")
                    if section > MAX_ORDER:
                        raise bad(n, f"order {section} above {MAX_ORDER}")
                    seen, header_line, in_data = 0, n, False
                    continue
                if in_data and line.startswith("ngram "):
                    try:
                        k, v = line[len("ngram "):].split("=")
                        counts[int(k)] = int(v)
                    except ValueError:
                        raise bad(n, f"bad count line {line!r}") from None
                    continue
                if not section:
                    raise bad(n, f"unexpected text {line!r}")
                parts = line.split()
                if len(parts) not in (section + 1, section + 2):
                    raise bad(n, f"a {section}-gram line has {section + 1} or {section + 2} fields, got {len(parts)}")
                try:
                    lp = float(parts[0])
                    bo = float(parts[section + 1]) if len(parts) == section + 2 else 0.0
                except ValueError:
                    raise bad(n, f"bad number in {line!r}") from None
                if not (math.isfinite(lp) and math.isfinite(bo)):
                    raise bad(n, f"non-finite number in {line!r}")
                key = []
                for w in parts[1:section + 1]:
                    if w in (BOS, EOS, UNK):
                        key.append(w)
                        continue
                    try:
                        c = int(w)
                    except ValueError:
                        raise bad(n, f"token {w!r} is neither a class index nor <s>, </s>, <unk>") from None
                    if not 0 <= c < int(vocab_size):
                        raise bad(n, f"token {c} outside [0, vocab_size={int(vocab_size)})")
                    key.append(c)
                key = tuple(key)
                if key in ngrams:
                    raise bad(n, f"n-gram {key} twice")
                ngrams[key] = (lp, bo)
                lines[key] = n
                seen += 1
        if not ended:
            raise ValueError(f"{path}: no \\end\\ line")
        for k, v in counts.items():
            if v and not any(len(key) == k for key in ngrams):
                raise ValueError(f"{path}: the count lines announce {v} {k}-grams, the file has no such section")
        try:
            return cls.from_ngrams(ngrams, vocab_size, unk_logp, _lines=lines)
        except ValueError as err:
            raise ValueError(f"{path}: {err}") from None

    # ---- the walk, exactly as the kernels take it (k_ngram_common.h ngram_lookup) ----
    def lookup(self, state: int, token: int) -> Tuple[float, int]:
        """(log P(token | state) in natural log as the fp32 walk gives it, next state)."""
        return self._lookup(state, token)[:2]

    def _lookup(self, state: int, token: int) -> Tuple[float, int, int]:
        """lookup's pair and the state in whose row the token was found (0: the root's dense row)."""
        s, c = int(state), int(token)
        if not (0 <= s < self.num_states and 0 <= c < self.vocab_size):
            raise IndexError(f"NgramLM.lookup: state {s} or token {c} out of range")
        acc = np.float32(0.0)
        for _ in range(self.order):
            if s == 0:
                break
            lo, hi = int(self.row_off[s]), int(self.row_off[s + 1])
            i = lo + int(np.searchsorted(self.arc_label[lo:hi], c))
            if i < hi and self.arc_label[i] == c:
                return float(np.float32(acc + self.arc_logp[i])), int(self.arc_next[i]), s
            acc = np.float32(acc + self.bo_weight[s])
            s = int(self.bo_state[s])
        return float(np.float32(acc + self.uni_logp[c])), int(self.uni_next[c]), 0

    def score(self, tokens, eos: bool = False) -> float:
        """log P_lm(tokens) in natural log: the sum of the walk from `start`; with eos plus eos_logp[state behind the last token] (of
        `start` for an empty sequence), else no end-of-sentence term."""
        if eos and self.eos_logp is None:
            raise ValueError("NgramLM.score: eos=True needs a model with a </s> unigram (eos_logp is None)")
        s, total = self.start, 0.0
        for c in tokens:
            lp, s = self.lookup(s, c)
            total += lp
        return total + float(self.eos_logp[s]) if eos else total

    def token_scores(self, tokens, bos: bool = True):
        """What ngram_score writes per position: (the values lookup gives along the walk from `start` -- bos=False: from the root --, the
        lengths of the n-grams found: the tokens of the history of the state whose row held the token, a <s> among them counted, plus 1;
        1 at the root, also for a class that took <unk>'s value)."""
        s, lps, orders = self.start if bos else 0, [], []
        for c in tokens:
            lp, s, at = self._lookup(s, c)
            lps.append(lp)
            orders.append(len(self.state_history[at]) + 1)
        return lps, orders

    # ---- the device side ----
    def host_tables(self) -> Dict[str, np.ndarray]:
        return {name: getattr(self, name) for name in TABLE_NAMES}

    def _struct(self, ptr) -> _Tables:
        return _Tables(*[ptr(name) for name in TABLE_NAMES], self.num_states, self.num_arcs, self.vocab_size, self.order, self.start)

    def check(self, lib) -> None:
        """crf_ngram_tables_check on the host copies, once per model."""
        if self._checked:
            return
        hold = {name: np.ascontiguousarray(a) for name, a in self.host_tables().items()}
        st = self._struct(lambda name: hold[name].ctypes.data if hold[name].size else None)
        if lib.crf_ngram_tables_check(ctypes.byref(st)) != 0:
            raise RuntimeError(lib.crf_last_error().decode())
        self._checked = True

    def tables(self, device):
        """The tables on `device` (uploaded once per device and kept) as (crf_ngram_tables struct of device pointers, dict of tensors;
        with "eos_logp" where the model has one)."""
        import torch
        from .ctc_crf import _C
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            self.check(_C._lib)
            tens = {name: torch.from_numpy(np.ascontiguousarray(a)).to(device) for name, a in self.host_tables().items()}
            st = self._struct(lambda name: tens[name].data_ptr() if tens[name].numel() else None)
            if self.eos_logp is not None:       # (beside the struct: crf_ngram_score takes it as an argument of its own)
                tens["eos_logp"] = torch.from_numpy(np.ascontiguousarray(self.eos_logp)).to(device)
            self._device[device] = (st, tens)
        return self._device[device]

    def __repr__(self):
        return f"NgramLM(order={self.order}, vocab_size={self.vocab_size}, states={self.num_states}, arcs={self.num_arcs})"
