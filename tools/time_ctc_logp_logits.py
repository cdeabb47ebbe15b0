"""tools/time_ctc_logp_logits.py -- HIP-event timings and peak memory of ctc_logp(fuse_log_softmax=True) forward + backward on bf16 RAW
network output against the only way to the same gradient without it: ctc_logp on torch.log_softmax(x.float(), -1) with autograd through
the softmax (DESIGN.md section 7 (f8) records the output).
`python tools/time_ctc_logp_logits.py [--calls 24] [--warmup 4] [--out FILE]`

The method of tools/time_ctc_score_grad.py: both sides in ONE process, alternating call by call (A B A B ...), each call between two HIP
events on the current stream, `--calls` >= 20 calls per side after `--warmup`; per side: median and the spread min .. max in
milliseconds, and the peak of torch.cuda.max_memory_allocated over one call above what was allocated before it.  The workload is forward
+ backward of sum_h w_h score_h down to the bf16 input's gradient, at N = 16, T = 1 500, H = 160 (ten hypotheses per utterance, grouped by
utterance), L in {20, 250} x V in {72, 5 000}.  Before the timed calls the fused bf16 gradient is compared with the yardstick's fp32
gradient (one bf16 rounding, at most 2^-8 of an entry, plus 1e-4 of the largest).  One JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_logits import measure  # noqa: E402
from time_ctc_score_grad import peak_mib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    core = ctc_crf._C
    out = []
    N, T, H = 16, 1500, 160
    K = H // N
    for V in (72, 5000):
        for L in (20, 250):
            rng = np.random.default_rng(V + L)
            x = torch.randn((N, T, V), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(V + L)).mul_(2.0).to(torch.bfloat16)
            hyps = torch.tensor(rng.integers(1, V, size=(H, L)).astype(np.int32))
            hl = torch.full((H,), L, dtype=torch.int32)
            lx = torch.full((N,), T, dtype=torch.int32)
            utt = torch.arange(N, dtype=torch.int32).repeat_interleave(K)
            w = torch.tensor(rng.normal(size=H).astype(np.float32)).to("cuda:0")

            def fused():
                leaf = x.detach().requires_grad_(True)
                scores, _ = ctc_crf.ctc_logp(leaf, hyps, hl, lx, utt, fuse_log_softmax=True)
                (w * scores).sum().backward()
                return leaf.grad

            def unfused():
                leaf = x.detach().requires_grad_(True)
                scores, _ = ctc_crf.ctc_logp(torch.log_softmax(leaf.float(), -1), hyps, hl, lx, utt)
                (w * scores).sum().backward()
                return leaf.grad

            x32 = x.float().requires_grad_(True)                     # the yardstick's gradient BEFORE its cast to bf16: one rounding apart
            (w * ctc_crf.ctc_logp(torch.log_softmax(x32, -1), hyps, hl, lx, utt)[0]).sum().backward()
            r = x32.grad.double()
            del x32
            g = fused()
            assert g.dtype == torch.bfloat16 and unfused().dtype == torch.bfloat16
            excess = float(((g.double() - r).abs() - 2.0 ** -8 * r.abs()).max() / r.abs().max())
            assert excess <= 1e-4, excess
            del g, r
            core.ctc_score_grad(x, (hyps, hl, lx, utt), w, fused=True)   # the call itself, on this thread: names its kernel
            kernel = core.last_score_grad_kernel()
            mem = dict(fused=peak_mib(fused), unfused=peak_mib(unfused))
            shape = dict(N=N, T=T, V=V, H=H, L=L, dtype="bf16", kernel=kernel, excess_over_one_bf16_rounding=excess,
                         peak_MiB=mem, workspace_MiB=round(core._lib.crf_ctc_score_grad_logits_workspace_bytes(N, H, T, V, L) / 2**20, 1))
            out.append(measure("logp_fused_vs_unfused", shape, fused, unfused, a.calls, a.warmup, "ctc_logp(fuse_log_softmax=True) + backward",
                               "log_softmax(x.float()) + ctc_logp + backward through the softmax"))
            del x
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
