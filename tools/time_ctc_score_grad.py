"""tools/time_ctc_score_grad.py -- HIP-event timings and peak memory of ctc_logp forward + backward (differentiable scores of H hypotheses
over N utterances, activations read in place, ONE [N,T,V] gradient) against the two ways to the same gradient without it (DESIGN.md
section 7 (f7) records the output).
`python tools/time_ctc_score_grad.py [--calls 24] [--warmup 4] [--out FILE]`

Every pair is measured in ONE process with the two sides alternating call by call (A B A B ...), each call between two HIP events on the
current stream, `--calls` >= 20 calls per side after `--warmup`; per side: median and the spread min .. max in milliseconds, and the peak
of torch.cuda.max_memory_allocated over one call above what was allocated before it.  Side A is always ctc_crf.ctc_logp + backward of
sum_h w_h score_h; side B is

  repeat   log_probs.repeat_interleave(H / N, 0) + _C.loss_fwd_bwd (crf_ctc_fwd_bwd: the numerator-only loss call on H copies of the
           activations, an [H,T,V] gradient) + the weights + index_add_ into [N,T,V]
  torch    the same copies through torch.nn.functional.ctc_loss(reduction='none') and autograd (repeat_interleave's backward folds)

at N = 16, T = 1 500, V = 72, H = 160 (ten hypotheses per utterance, grouped by utterance) with L = 250 and with L = 20.  Before the
timed calls A is compared with `repeat` (1e-4 of the largest entry).  One JSON line per pair."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_logits import measure  # noqa: E402


def peak_mib(f):
    """MiB one call of f allocates at its peak above what is allocated already."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)


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
        utt_dev = utt.long().to("cuda:0")
        hyps_dev, hl_dev, lx_dev = hyps.long().to("cuda:0"), hl.long().to("cuda:0"), lx_rep.long().to("cuda:0")
        w = torch.tensor(rng.normal(size=H).astype(np.float32)).to("cuda:0")

        def logp():
            leaf = lp.detach().requires_grad_(True)
            scores, _ = ctc_crf.ctc_logp(leaf, hyps, hl, lx, utt)
            (w * scores).sum().backward()
            return leaf.grad

        def repeat():
            rep = lp.repeat_interleave(K, 0)
            grad = core.loss_fwd_bwd(rep, hyps, lx_rep, hl, 0.0, -1.0, None)[1]          # c_ctc = -1: + gamma per copy
            return torch.zeros_like(lp).index_add_(0, utt_dev, grad.mul_(w[:, None, None]))

        def torch_ctc():
            leaf = lp.detach().requires_grad_(True)
            rep = leaf.repeat_interleave(K, 0).transpose(0, 1)
            nll = torch.nn.functional.ctc_loss(rep, hyps_dev, lx_dev, hl_dev, blank=0, reduction="none", zero_infinity=True)
            (w * -nll).sum().backward()
            return leaf.grad

        g, r = logp().double(), repeat().double()
        d = core.ctc_score_grad(lp, (hyps, hl, lx, utt), w)[0].double()                  # the call itself, on this thread: names its kernel
        kernel = core.last_score_grad_kernel()
        diff = float(max((g - r).abs().max(), (d - r).abs().max()) / r.abs().max())
        assert diff <= 1e-4, diff
        del g, r, d
        mem = dict(ctc_logp=peak_mib(logp), repeat=peak_mib(repeat), torch=peak_mib(torch_ctc))
        shape = dict(N=N, T=T, V=V, H=H, L=L, kernel=kernel, max_diff_vs_repeat=diff, peak_MiB=mem,
                     workspace_MiB=round(core._lib.crf_ctc_score_grad_workspace_bytes(N, H, T, V, L) / 2**20, 1))
        out.append(measure("logp_vs_repeat", shape, logp, repeat, a.calls, a.warmup, "ctc_logp + backward",
                           "repeat_interleave + loss_fwd_bwd + weights + index_add_"))
        out.append(measure("logp_vs_torch", shape, logp, torch_ctc, a.calls, a.warmup, "ctc_logp + backward",
                           "repeat_interleave + F.ctc_loss(reduction='none') + backward"))
        del lp
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
