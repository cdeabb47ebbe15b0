"""tools/time_ctc_sample.py -- HIP-event timings of ctc_sample and ctc_greedy (label sequences drawn on the GPU, activations read in
place) against the reference's way to the same thing with torch ops on the GPU (DESIGN.md section 7 records the output).
`python tools/time_ctc_sample.py [--calls 24] [--warmup 4] [--out FILE]`

Every pair is measured in ONE process with the two sides alternating call by call (A B A B ...), each call between two HIP events on the
current stream, `--calls` >= 20 calls per side after `--warmup`; per side: median and the spread min .. max in milliseconds.

  sample   A: ctc_crf.ctc_sample(lp, lx, K, seed)
           B: torch.multinomial(lp.exp().view(-1, V), K, True) (cat/ctc/train_jsa.py:256-269), the transpose to [N K][T], and a collapse
              in torch ops: keep mask, cumsum, scatter into a blank-filled row (what stands in for the third-party ctc_align.align_)
  greedy   A: ctc_crf.ctc_greedy(lp, lx)
           B: lp.argmax(-1) and the same collapse

at N = 16, T = 1 500, K = 10 with V = 72 and V = 5 000, fp32 log-probs, full-length utterances.  Before the timed calls the torch collapse
is checked against ctc_sample's own (the same frame paths in, the same rows out).  One JSON line per pair."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_logits import measure  # noqa: E402


def torch_collapse(paths, lx_dev, blank):
    """paths [H][T] (classes), lx_dev [H] -> (hyps [H][T] padded with the blank, lengths [H]): mask, cumsum, scatter."""
    H, T = paths.shape
    t = torch.arange(T, device=paths.device)[None, :]
    prev = torch.cat([paths.new_full((H, 1), -1), paths[:, :-1]], 1)
    keep = (paths != blank) & (paths != prev) & (t < lx_dev[:, None])
    pos = torch.cumsum(keep, 1) - 1
    out = paths.new_full((H, T + 1), blank)
    out.scatter_(1, torch.where(keep, pos, torch.full_like(pos, T)), paths)     # dropped frames land in a spare column
    out[:, T] = blank
    return out[:, :T], keep.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    core = ctc_crf._C
    out = []
    N, T, K, blank = 16, 1500, 10, 0
    for V in (72, 5000):
        x = torch.randn((N, T, V), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(V)).mul_(2.0)
        lp = torch.log_softmax(x, -1)
        del x
        lx = torch.full((N,), T, dtype=torch.int32)
        lx_k = lx.to("cuda:0").repeat_interleave(K)
        lx_1 = lx.to("cuda:0")

        def sample():
            return ctc_crf.ctc_sample(lp, lx, K, 1234, blank=blank)

        def multinomial():
            with torch.no_grad():
                s = torch.multinomial(lp.exp().view(-1, V), K, True)               # [N T][K]
                paths = s.view(N, T, K).permute(0, 2, 1).reshape(N * K, T)
                return torch_collapse(paths, lx_k, blank)

        def greedy():
            return ctc_crf.ctc_greedy(lp, lx, blank=blank)

        def argmax():
            with torch.no_grad():
                return torch_collapse(lp.argmax(-1), lx_1, blank)

        hyps, hl, _, paths = ctc_crf.ctc_sample(lp, lx, K, 1234, blank=blank, return_paths=True)
        kernel = core.last_sample_kernel()
        th, tl = torch_collapse(paths.long(), lx_k, blank)
        assert torch.equal(th.int(), hyps) and torch.equal(tl.int(), hl)
        gh, gl = greedy()
        th, tl = argmax()
        assert torch.equal(th.int(), gh) and torch.equal(tl.int(), gl)
        shape = dict(N=N, T=T, V=V, K=K, kernel=kernel)
        out.append(measure("sample_vs_multinomial", shape, sample, multinomial, a.calls, a.warmup, "ctc_sample",
                           "exp + torch.multinomial + transpose + torch collapse (mask, cumsum, scatter)"))
        out.append(measure("greedy_vs_argmax", dict(N=N, T=T, V=V), greedy, argmax, a.calls, a.warmup, "ctc_greedy",
                           "argmax + torch collapse (mask, cumsum, scatter)"))
        del lp
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
