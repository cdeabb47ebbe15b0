"""tools/time_ctc_logits.py -- HIP-event timings of the numerator-only surface on raw network output against the unfused way to the same
result (DESIGN.md section 7 records the output).  `python tools/time_ctc_logits.py [--calls 24] [--warmup 4] [--out FILE]`

Every pair is measured in ONE process with the two sides alternating call by call (A B A B ...), each call between two HIP events on the
current stream, `--calls` >= 20 calls per side after `--warmup`; per side: median and the spread min .. max in milliseconds.

  1. align_f32        crf_ctc_align on fp32 log-probs            | numerator-only crf_ctc_fwd_bwd at the same shape   (B 64, T 1500, V 72, L 250)
  2. align_bf16       ctc_align(fuse_log_softmax=True) on bf16   | ctc_align(torch.log_softmax(x.float(), -1))         (that shape, and V = 5000)
  3. ctc_bf16         WARP_CTC_LOSS(fuse_log_softmax=True), forward + backward, on bf16
                                                                 | log_softmax(x.float()) + WARP_CTC_LOSS + autograd through the softmax
                                                                                                                     (that shape, batch- and time-major)
One JSON line per pair."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402


def batch(B, T, V, L, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.randn((B, T, V), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(seed)).mul_(2.0)
    ly = np.full(B, L, dtype=np.int32)
    labels = rng.integers(1, V, size=int(ly.sum())).astype(np.int32)
    return x, torch.tensor(labels), torch.full((B,), T, dtype=torch.int32), torch.tensor(ly)


def measure(name, shape, a, b, calls, warmup, note_a, note_b):
    ms = {0: [], 1: []}
    for i in range(warmup + calls):
        for k, f in enumerate((a, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    st = lambda v: dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))   # noqa: E731
    rec = dict(pair=name, shape=shape, calls=calls, a=dict(what=note_a, **st(ms[0])), b=dict(what=note_b, **st(ms[1])))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    core = ctc_crf._C
    out = []
    B, T, L = 64, 1500, 250

    x, lab, lx, ly = batch(B, T, 72, L)
    lp = torch.log_softmax(x, -1)
    g_out = torch.empty_like(lp)
    out.append(measure("align_f32", dict(B=B, T=T, V=72, L=L),
                       lambda: core.ctc_align(lp, lab, lx, ly), lambda: core.loss_fwd_bwd(lp, lab, lx, ly, 0.0, 1.0, None, grad_out=g_out),
                       a.calls, a.warmup, "ctc_align(log_probs f32)", "numerator-only loss_fwd_bwd (crf_ctc_fwd_bwd)"))
    del lp, g_out
    for V in (72, 5000):
        x, lab, lx, ly = batch(B, T, V, L)
        xb = x.to(torch.bfloat16)
        del x
        out.append(measure("align_bf16", dict(B=B, T=T, V=V, L=L),
                           lambda: ctc_crf.ctc_align(xb, lab, lx, ly, fuse_log_softmax=True),
                           lambda: ctc_crf.ctc_align(torch.log_softmax(xb.float(), -1), lab, lx, ly),
                           a.calls, a.warmup, "ctc_align(bf16, fuse_log_softmax=True)", "ctc_align(log_softmax(x.float()))"))
        del xb
        torch.cuda.empty_cache()
    x, lab, lx, ly = batch(B, T, 72, L)
    for tm in (False, True):
        xb = (x.transpose(0, 1).contiguous() if tm else x).to(torch.bfloat16).requires_grad_(True)
        fused, plain = ctc_crf.WARP_CTC_LOSS(fuse_log_softmax=True, time_major=tm), ctc_crf.WARP_CTC_LOSS(time_major=tm)

        def run_fused():
            xb.grad = None
            fused(xb, lab, lx, ly).backward()

        def run_plain():
            xb.grad = None
            plain(torch.log_softmax(xb.float(), -1), lab, lx, ly).backward()
        out.append(measure("ctc_bf16", dict(B=B, T=T, V=72, L=L, time_major=tm), run_fused, run_plain, a.calls, a.warmup,
                           "WARP_CTC_LOSS(fuse_log_softmax=True) fwd+bwd", "log_softmax(x.float()) + WARP_CTC_LOSS + autograd"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
