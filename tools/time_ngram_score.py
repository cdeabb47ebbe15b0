"""tools/time_ngram_score.py -- HIP-event timings of ngram_score (n-gram LM scores of hypothesis rows on the GPU, one wave per row)
against the way a caller has without it (DESIGN.md section 7 (f13) records the output).
`python tools/time_ngram_score.py [--calls 24] [--warmup 4] [--cpu-calls 2] [--out FILE]`

The pairs alternate call by call (A B A B ...) in ONE process, each call between two HIP events on the current stream, `--calls` >= 20
calls per side after `--warmup`; per side: median and the spread min .. max in ms (tools/time_ctc_logits.py `measure`).

  score_vs_floor  A: ctc_crf.ngram_score(hyps, hl, lm, eos=False)
                  B: the same call on the first 4 rows: one workgroup -- what a call costs in launch and enqueue (the Python wrapper, the
                     output tensors, one kernel launch), whatever it scores
  score_vs_host   A: the same call;  B: hyps.cpu(), hl.cpu() and NgramLM.score per row (what a caller has on the parent commit) --
                  `--cpu-calls` calls only (each takes seconds), timed by the same events, which then span the host's work
  tokens_vs_score A: ngram_score(..., return_token_scores=True)   B: ngram_score(...)

at H = 1 024 rows of about 75 tokens (rows 150 wide) and H = 16 384 rows of about 20 tokens (rows 40 wide), for random models of order 1,
3 and 5 over V = 72 and V = 5 000 as tools/time_ctc_beam_lm.py draws them (pruned contexts); the rows are drawn half from the model's
n-grams, half at random, so that look-ups both match deep and back off.  The tables are uploaded before the first timed call.  One JSON
line per pair."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_beam_lm import random_model  # noqa: E402
from time_ctc_logits import measure  # noqa: E402


def make_rows(lm, H, L, W, seed):
    """H rows of about L tokens: walks that follow an arc of the current state with probability 1/2, else a random class."""
    rng = np.random.default_rng([seed, H, L])
    V = lm.vocab_size
    lens = rng.integers(L - L // 5, L + L // 5 + 1, size=H)
    rows = np.zeros((H, W), dtype=np.int32)
    coin, pick, rand = rng.random((H, W)), rng.random((H, W)), rng.integers(0, V, size=(H, W))
    for h in range(H):
        s = lm.start
        for i in range(int(lens[h])):
            lo, hi = int(lm.row_off[s]), int(lm.row_off[s + 1])
            if hi > lo and coin[h, i] < 0.5:
                a = lo + int(pick[h, i] * (hi - lo))
                c, s = int(lm.arc_label[a]), int(lm.arc_next[a])
            else:
                c = int(rand[h, i])
                s = int(lm.uni_next[c])
            rows[h, i] = c
    return torch.tensor(rows).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--cpu-calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    core = ctc_crf._C
    out = []
    for V in (72, 5000):
        for order in (1, 3, 5):
            lm = random_model(V, order)
            for H, L, W in ((1024, 75, 150), (16384, 20, 40)):
                hyps, hl = make_rows(lm, H, L, W, V + order)
                few, few_l = hyps[:4].contiguous(), hl[:4].contiguous()

                def score():
                    return ctc_crf.ngram_score(hyps, hl, lm)

                def floor():
                    return ctc_crf.ngram_score(few, few_l, lm)

                def tokens():
                    return ctc_crf.ngram_score(hyps, hl, lm, return_token_scores=True)

                def by_host():
                    rows, lens = hyps.cpu().numpy(), hl.cpu().numpy()
                    return [lm.score(rows[h, :lens[h]].tolist()) for h in range(H)]

                got, inv = score()
                want = np.asarray(by_host())
                assert not bool(inv.any()) and np.allclose(got.cpu().double().numpy(), want, rtol=1e-6, atol=0)
                _, _, _, to = tokens()
                shape = dict(H=H, W=W, V=V, order=order, states=lm.num_states, arcs=lm.num_arcs, mean_len=round(float(hl.float().mean()), 1),
                             mean_matched=round(float(to.sum()) / float(hl.sum()), 2), kernel="crf_ngram_score_kernel<scores>")
                out.append(measure("score_vs_floor", shape, score, floor, a.calls, a.warmup, "ngram_score", "ngram_score on 4 rows (launch and enqueue)"))
                out.append(measure("tokens_vs_score", shape, tokens, score, a.calls, a.warmup, "ngram_score(return_token_scores=True)", "ngram_score"))
                out.append(measure("score_vs_host", shape, score, by_host, a.cpu_calls, 0, "ngram_score", ".cpu() + NgramLM.score per row"))
    assert core.last_ngram_score_kernel().startswith("crf_ngram_score_kernel")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
