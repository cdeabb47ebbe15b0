"""tools/time_ctc_beam.py -- HIP-event timings of ctc_beam_search (prefix beam search on the GPU, activations read in place), with
ctc_greedy and ctc_align in the same process as scale (DESIGN.md section 7 (f9) records the output).
`python tools/time_ctc_beam.py [--calls 24] [--warmup 4] [--out FILE]`

There is no GPU competitor on this machine -- the callers' ctcdecode.CTCBeamDecoder is a CPU library that is not installed -- so the
pairs are beam search (A) against a call of known cost (B), alternating call by call (A B A B ...) in ONE process, each call between two
HIP events on the current stream, `--calls` >= 20 calls per side after `--warmup`; per side: median and the spread min .. max in ms.

  beam_vs_greedy  A: ctc_crf.ctc_beam_search(lp, lx, 16, nbest, 40)          B: ctc_crf.ctc_greedy(lp, lx)
  beam_vs_align   A: the same with nbest = 1                                 B: ctc_crf.ctc_align(lp, labels of 250 per utterance, lx, ly)

at N = 16 and 64, T = 1 500, V = 72 and 5 000, W = 16, C = 40, nbest = 1 and 16, fp32 log-probs, full-length utterances.  One JSON line
per pair."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_logits import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    core = ctc_crf._C
    out = []
    T, W, C, L, blank = 1500, 16, 40, 250, 0
    for N in (16, 64):
        for V in (72, 5000):
            gen = torch.Generator(device="cuda:0").manual_seed(V + N)
            x = torch.randn((N, T, V), device="cuda:0", generator=gen).mul_(2.0)
            lp = torch.log_softmax(x, -1)
            del x
            lx = torch.full((N,), T, dtype=torch.int32)
            ly = torch.full((N,), L, dtype=torch.int32)
            lab = torch.randint(1, V, (N * L,), dtype=torch.int32)

            def greedy():
                return ctc_crf.ctc_greedy(lp, lx, blank=blank)

            def align():
                return ctc_crf.ctc_align(lp, lab, lx, ly, blank=blank)

            for nbest in (1, 16):
                def beam():
                    return ctc_crf.ctc_beam_search(lp, lx, W, nbest, C, blank=blank)

                hyps, hl, _, sc = beam()
                shape = dict(N=N, T=T, V=V, W=W, C=C, nbest=nbest, kernel=core.last_beam_kernel(), mean_len=round(float(hl.float().mean()), 1))
                assert bool(torch.isfinite(sc.view(N, nbest)[:, 0]).all())
                out.append(measure("beam_vs_greedy", shape, beam, greedy, a.calls, a.warmup, "ctc_beam_search", "ctc_greedy"))
            out.append(measure("beam_vs_align", dict(N=N, T=T, V=V, W=W, C=C, nbest=1, L=L),
                               lambda: ctc_crf.ctc_beam_search(lp, lx, W, 1, C, blank=blank), align, a.calls, a.warmup,
                               "ctc_beam_search", "ctc_align (250 labels per utterance)"))
            del lp
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
