"""tools/time_ctc_score_rows.py -- HIP-event timings and peak memory of the sample -> score -> backward chain with the hypotheses copied
to the host in between (what ctc_logp needed before it took device rows) against the same chain on the rows where ctc_sample left them
(DESIGN.md section 7 (f12) records the output).
`python tools/time_ctc_score_rows.py [--calls 24] [--warmup 4] [--out FILE]`

The method of tools/time_ctc_score_grad.py: every pair in ONE process, the two sides alternating call by call (A B A B ...), each call
between two HIP events on the current stream, `--calls` >= 20 calls per side after `--warmup`; per side median and min .. max in
milliseconds, the peak of torch.cuda.max_memory_allocated over one call, and `host_ms`: the median time the host spends inside one call
on an idle device (side A waits there for the samples; side B only enqueues).

  A   ctc_sample -> hyps.cpu(), hyp_lengths.cpu(), hyp_utt.cpu() -> ctc_logp -> backward     (the host learns the longest hypothesis)
  B   ctc_sample -> ctc_logp(max_hyp_len=...) -> backward on the device rows                   (the host knows only the bound)

at N = 64, K = 16 (H = 1 024 rows of W = T = 1 500 words), T = 1 500, V = 72 and V = 5 000, with max_hyp_len tight (the true maximum,
read once before the timed calls) and at its default (min(W, 255): the gradient's widest class).  The log-probs favour the blank (0.95
per frame), so the sampled hypotheses hold about 75 labels.  One JSON line per pair."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_logits import measure  # noqa: E402
from time_ctc_score_grad import peak_mib  # noqa: E402


def host_ms(f, calls, warmup):
    """Median milliseconds the HOST spends inside one call of f on an idle device: what the next piece of Python waits for."""
    ms = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    torch.cuda.synchronize()
    return round(sorted(ms)[len(ms) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    core = ctc_crf._C
    out = []
    N, T, K, P_BLANK = 64, 1500, 16, 0.95
    for V in (72, 5000):
        x = torch.randn((N, T, V), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(V))
        x[..., 0] = torch.logsumexp(x[..., 1:], -1) + float(torch.log(torch.tensor(P_BLANK / (1.0 - P_BLANK))))
        lp = torch.log_softmax(x, -1)
        del x
        lx = torch.full((N,), T, dtype=torch.int32)
        risk = torch.rand(N, K, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(V + 1))
        _, hl0, _ = ctc_crf.ctc_sample(lp, lx, K, 2024)
        longest = int(hl0.max())               # (a synchronisation, once, outside the timed calls)
        assert longest <= 255, longest

        def chain(device_rows, bound):
            def f():
                leaf = lp.detach().requires_grad_(True)
                hyps, hl, hu = ctc_crf.ctc_sample(leaf, lx, K, 2024)
                if device_rows:
                    scores, _ = ctc_crf.ctc_logp(leaf, hyps, hl, lx, hu, max_hyp_len=bound)
                else:
                    scores, _ = ctc_crf.ctc_logp(leaf, hyps.cpu(), hl.cpu(), lx, hu.cpu())
                (torch.softmax(scores.view(N, K), -1) * risk).sum().backward()
                return scores.detach(), leaf.grad
            return f

        host = chain(False, None)
        s_a, g_a = host()
        for name, bound in (("tight", longest), ("default", None)):
            rows = chain(True, bound)
            s_b, g_b = rows()
            kernel = core.last_score_kernel()
            sdiff = float(((s_a - s_b).abs() / s_a.abs()).max())      # (A scores every row with the longest one's kernel, B each with its own class's)
            diff = float((g_a - g_b).abs().max() / g_a.abs().max())
            assert sdiff <= 1e-4 and diff <= 1e-4, (sdiff, diff)
            cap = bound if bound is not None else min(T, 255)
            shape = dict(N=N, T=T, V=V, K=K, H=N * K, W=T, longest=longest, max_hyp_len=name, len_cap=cap, score_kernel=kernel,
                         max_score_diff=sdiff, max_grad_diff=diff,
                         host_ms=dict(host=host_ms(host, a.calls, a.warmup), rows=host_ms(rows, a.calls, a.warmup)), peak_MiB=dict(host=peak_mib(host), rows=peak_mib(rows)),
                         workspace_MiB=dict(host=round(core._lib.crf_ctc_score_grad_workspace_bytes(N, N * K, T, V, longest) / 2**20, 1),
                                            rows=round(core._lib.crf_ctc_score_grad_rows_workspace_bytes(N, N * K, T, V, cap, -1) / 2**20, 1)))
            out.append(measure(f"rows_vs_host_{name}", shape, host, rows, a.calls, a.warmup, "ctc_sample + .cpu() + ctc_logp + backward",
                               f"ctc_sample + ctc_logp(device rows, max_hyp_len {name}) + backward"))
            del s_b, g_b
        del lp, s_a, g_a
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
