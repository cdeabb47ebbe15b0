"""tools/time_ctc_score.py -- HIP-event timings of ctc_score (forward-only scores of H hypotheses over N utterances, activations read in
place) against the two ways to the same numbers without it (DESIGN.md section 7 records the output).
`python tools/time_ctc_score.py [--calls 24] [--warmup 4] [--out FILE]`

Every pair is measured in ONE process with the two sides alternating call by call (A B A B ...), each call between two HIP events on the
current stream, `--calls` >= 20 calls per side after `--warmup`; per side: median and the spread min .. max in milliseconds.  Side A is
always ctc_crf.ctc_score; side B is

  repeat   log_probs.repeat_interleave(H / N, 0) + _C.loss_fwd_bwd(..., want_costs=True): the numerator-only loss call on H copies of the
           activations, of which costs_ctc is kept (the backward chain, the grad pass and the H x T x V gradient are thrown away)
  torch    torch.nn.functional.ctc_loss(reduction='none') under no_grad on the same H copies (what cat/ctc/decode_jsa_mls.py:189-191 does)

at N = 16, T = 1 500, V = 72, H = 160 (ten hypotheses per utterance, grouped by utterance) with L = 250 and with L = 20.  Before the
timed calls the three results are compared (rtol 1e-4).  One JSON line per pair."""
import argparse
import json
import os
import sys

import numpy as np
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
    N, T, V, H = 16, 1500, 72, 160
    K = H // N
    for L in (250, 20):
        rng = np.random.default_rng(L)
        x = torch.randn((N, T, V), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(L)).mul_(2.0)
        lp = torch.log_softmax(x, -1)
        del x
        hyps = torch.tensor(rng.integers(1, V, size=(H, L)).astype(np.int32))
        hl = torch.full((H,), L, dtype=torch.int32)
        lx = torch.full((N,), T, dtype=torch.int32)
        lx_rep = lx.repeat_interleave(K)
        utt = torch.arange(N, dtype=torch.int32).repeat_interleave(K)
        hyps_dev, hl_dev, lx_dev = hyps.long().to("cuda:0"), hl.long().to("cuda:0"), lx_rep.long().to("cuda:0")

        def score():
            return ctc_crf.ctc_score(lp, hyps, hl, lx, utt)

        def repeat():
            rep = lp.repeat_interleave(K, 0)
            return core.loss_fwd_bwd(rep, hyps, lx_rep, hl, 0.0, 1.0, None, want_costs=True)[2]["costs_ctc"]

        def torch_ctc():
            with torch.no_grad():
                rep = lp.repeat_interleave(K, 0).transpose(0, 1)
                return -torch.nn.functional.ctc_loss(rep, hyps_dev, lx_dev, hl_dev, blank=0, reduction="none")

        s, r, t = (f().double().cpu().numpy() for f in (score, repeat, torch_ctc))
        agree = dict(repeat=float(np.max(np.abs(s - r) / np.abs(r))), torch=float(np.max(np.abs(s - t) / np.abs(t))))
        assert agree["repeat"] <= 1e-4 and agree["torch"] <= 1e-4, agree
        shape = dict(N=N, T=T, V=V, H=H, L=L, kernel=core.last_score_kernel(), max_rel_diff=agree)
        out.append(measure("score_vs_repeat", shape, score, repeat, a.calls, a.warmup, "ctc_score",
                           "repeat_interleave + loss_fwd_bwd(want_costs=True)"))
        out.append(measure("score_vs_torch", shape, score, torch_ctc, a.calls, a.warmup, "ctc_score",
                           "repeat_interleave + F.ctc_loss(reduction='none') under no_grad"))
        del lp
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
