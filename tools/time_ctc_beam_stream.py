"""tools/time_ctc_beam_stream.py -- HIP-event timings of the streaming beam search, ctc_beam_search_chunk, against the whole-utterance
call ctc_beam_search (DESIGN.md section 7 (f14) records the output).
`python tools/time_ctc_beam_stream.py [--calls 24] [--warmup 4] [--rerun-calls 4] [--out FILE]`

The method of tools/time_ctc_beam.py: two sides alternating call by call (A B A B ...) in ONE process, each side between two HIP events on
the current stream, `--calls` >= 20 per side after `--warmup`; per side: median and the spread min .. max in ms.

  stream_vs_whole  A: the loop of T / chunk ctc_beam_search_chunk calls over one utterance batch (the SUM over the chunk calls: the
                      chunks are contiguous tensors made beforehand, as an encoder that runs chunk by chunk leaves them, the chunk
                      lengths int32 tensors on the device)
                   B: ONE ctc_beam_search call on all T frames
  rerun            what a streaming caller has without the chunk call: after every chunk, ctc_beam_search on all frames so far
                   (input_lengths = frames so far on the full tensor), summed over the chunks -- quadratic in T / chunk, so it is
                   timed with `--rerun-calls` calls after one warm-up, not alternating.

at T = 1 500, W = 16, C = 40, nbest = 1, N = 16 and 64, V = 72 and 5 000, chunk = 16, 64 and 256 frames, without an LM and with an order-3
LM (tools/time_ctc_beam_lm.py's random model, alpha = 0.5, beta = 1.0), fp32 log-probs, full-length utterances.  One JSON line per pair;
`per_chunk_ms` is A's median over the number of chunks, `share_ms` B's median times chunk / T."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rerun-calls", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    out = []
    T, W, C, blank, dev = 1500, 16, 40, 0, "cuda:0"
    for N in (16, 64):
        for V in (72, 5000):
            gen = torch.Generator(device=dev).manual_seed(V + N)
            lp = torch.log_softmax(torch.randn((N, T, V), device=dev, generator=gen).mul_(2.0), -1)
            lx = torch.full((N,), T, dtype=torch.int32)
            for lm in (None, random_model(V, 3)):
                kw = dict(lm=lm, alpha=0.5, beta=1.0) if lm is not None else {}

                def whole():
                    return ctc_crf.ctc_beam_search(lp, lx, W, 1, C, blank=blank, **kw)

                want = whole()
                for chunk in (16, 64, 256):
                    edges = list(range(0, T, chunk)) + [T]
                    chunks = [lp[:, o:e].contiguous() for o, e in zip(edges, edges[1:])]
                    lens = [torch.full((N,), c.size(1), dtype=torch.int32, device=dev) for c in chunks]

                    def stream():
                        state, res = None, None
                        for c, l in zip(chunks, lens):
                            res = ctc_crf.ctc_beam_search_chunk(c, l, state, None, W, 1, C, blank=blank, **kw)
                            state = res[0]
                        return res

                    got = stream()
                    assert torch.equal(got[2], want[1]) and torch.equal(got[4], want[3]), "the chunk loop and the whole call differ"
                    shape = dict(N=N, T=T, V=V, W=W, C=C, nbest=1, lm=lm is not None, chunk=chunk, chunks=len(chunks))
                    rec = measure("stream_vs_whole", shape, stream, whole, a.calls, a.warmup, "sum of ctc_beam_search_chunk calls", "one ctc_beam_search")
                    ms = []
                    for i in range(1 + a.rerun_calls):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for e in edges[1:]:
                            ctc_crf.ctc_beam_search(lp, torch.full((N,), e, dtype=torch.int32), W, 1, C, blank=blank, **kw)
                        e1.record()
                        e1.synchronize()
                        if i:
                            ms.append(e0.elapsed_time(e1))
                    extra = dict(pair="rerun", shape=shape, calls=a.rerun_calls, rerun_median_ms=round(float(np.median(ms)), 3),
                                 rerun_min_ms=round(min(ms), 3), rerun_max_ms=round(max(ms), 3),
                                 per_chunk_ms=round(rec["a"]["median_ms"] / len(chunks), 4), share_ms=round(rec["b"]["median_ms"] * chunk / T, 4))
                    print(json.dumps(extra), flush=True)
                    out += [rec, extra]
                    del chunks
            del lp
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
