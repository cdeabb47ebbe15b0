"""tools/time_ctc_beam_lm.py -- HIP-event timings of ctc_beam_search with n-gram LM fusion (crf_ctc_beam_lm) against the LM-free call
(crf_ctc_beam) at the same shapes (DESIGN.md section 7 (f11) records the output).
`python tools/time_ctc_beam_lm.py [--calls 24] [--warmup 4] [--out FILE]`

The pairs alternate call by call (A B A B ...) in ONE process, each call between two HIP events on the current stream, `--calls` >= 20
calls per side after `--warmup`; per side: median and the spread min .. max in ms (tools/time_ctc_logits.py `measure`).

  beam_lm_vs_beam  A: ctc_crf.ctc_beam_search(lp, lx, 16, 1, 40, lm=lm, alpha=0.5, beta=1.0)   B: ctc_crf.ctc_beam_search(lp, lx, 16, 1, 40)

at N = 16 and 64, T = 1 500, V = 72 and 5 000, W = 16, C = 40, fp32 log-probs, full-length utterances, for a random model of order 1, 3
and 5 (unigrams for every class with <s>; per higher order 20 000 random n-grams -- or half of all there can be, if fewer -- whose
prefixes are in the model: pruned contexts, so a lookup that misses walks the back-off chain).  The tables are uploaded before the
first timed call.  One JSON line per pair."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_logits import measure  # noqa: E402


def random_model(V, order, per_order=20000, seed=0):
    rng = np.random.default_rng([seed, V, order])
    ng = {(c,): (float(-1.0 - 3.0 * rng.random()), float(-rng.random())) for c in range(V)}
    ng[("<s>",)] = (-99.0, -0.5)
    level = list(ng)
    for n in range(2, order + 1):
        nxt = {}
        want = min(per_order, len(level) * V // 2)          # (V = 72 has 5 256 bigrams in all)
        while len(nxt) < want:
            ctx = level[int(rng.integers(len(level)))]
            nxt[ctx + (int(rng.integers(V)),)] = (float(-0.1 - 2.0 * rng.random()), float(-rng.random()) if n < order else 0.0)
        ng.update(nxt)
        level = list(nxt)
    return ctc_crf.NgramLM.from_ngrams(ng, V)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    out = []
    T, W, C, blank = 1500, 16, 40, 0
    for V in (72, 5000):
        lms = {order: random_model(V, order) for order in (1, 3, 5)}
        for N in (16, 64):
            gen = torch.Generator(device="cuda:0").manual_seed(V + N)
            x = torch.randn((N, T, V), device="cuda:0", generator=gen).mul_(2.0)
            lp = torch.log_softmax(x, -1)
            del x
            lx = torch.full((N,), T, dtype=torch.int32)

            def plain():
                return ctc_crf.ctc_beam_search(lp, lx, W, 1, C, blank=blank)

            for order, lm in lms.items():
                def fused():
                    return ctc_crf.ctc_beam_search(lp, lx, W, 1, C, blank=blank, lm=lm, alpha=0.5, beta=1.0)

                hyps, hl, _, sc = fused()
                assert bool(torch.isfinite(sc).all())
                shape = dict(N=N, T=T, V=V, W=W, C=C, nbest=1, order=order, states=lm.num_states, arcs=lm.num_arcs,
                             mean_len=round(float(hl.float().mean()), 1))
                out.append(measure("beam_lm_vs_beam", shape, fused, plain, a.calls, a.warmup, "ctc_beam_search(lm=order %d)" % order,
                                   "ctc_beam_search (LM-free)"))
            del lp
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
