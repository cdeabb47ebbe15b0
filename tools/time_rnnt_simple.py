"""tools/time_rnnt_simple.py -- HIP-event timings of ctc_crf.rnnt_loss_simple forward + backward against the only other way to train a
model whose joiner is f + g: materialise the (N, T, U+1, V) tensor and hand it to rnnt_loss (DESIGN.md section 7 (f16) records the output).
`python tools/time_rnnt_simple.py [--calls 20] [--warmup 3] [--out FILE] [--only N,V,dtype]`

Every pair is measured in ONE process with the two sides alternating call by call (A B A B ...), each call between two HIP events on the
current stream (tools/time_ctc_logits.py measure); per side the median and the spread min .. max in milliseconds.  Side A is
rnnt_loss_simple(f, g, ..., reduction="sum") + backward; side B is rnnt_loss(f.unsqueeze(2) + g.unsqueeze(1), fuse_log_softmax=True,
reduction="sum") + backward to f and g (the broadcast add, the loss, and autograd's two reductions of the joint gradient).  Shapes: those of
the (f15) table -- N = 16 and 64, T = 250, U = 50, V = 1 024 and 5 000, bf16 and fp32, every utterance of full length, the lengths on the
device.  Before the timed calls one call of each side is run alone between torch.cuda.reset_peak_memory_stats and
torch.cuda.max_memory_allocated: `peak_MiB` is the rise above what was allocated before the call (f, g, the labels).  The two sides'
gradients are compared as max |A - B| / max |B|.  `a_below_b` is the claim to check: A's median below B's by more than B's own min .. max
span.  One JSON line per pair."""
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="N,V,dtype of the one shape to run, e.g. 16,1024,bfloat16")
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    T, U, blank = 250, 50, 0
    out = []
    for N in (16, 64):
        for V in (1024, 5000):
            for dtype in (torch.bfloat16, torch.float32):
                name = str(dtype).split(".")[1]
                if a.only and a.only != f"{N},{V},{name}":
                    continue
                gen = torch.Generator(device=dev).manual_seed(N + V)
                f = torch.randn((N, T, V), device=dev, generator=gen).mul_(2.0).to(dtype)
                g = torch.randn((N, U + 1, V), device=dev, generator=gen).mul_(2.0).to(dtype)
                labels = torch.randint(1, V, (N, U), device=dev, generator=gen, dtype=torch.int32)
                lx = torch.full((N,), T, dtype=torch.int32, device=dev)
                ly = torch.full((N,), U, dtype=torch.int32, device=dev)

                def simple():
                    lf, lg = f.detach().requires_grad_(True), g.detach().requires_grad_(True)
                    ctc_crf.rnnt_loss_simple(lf, lg, labels, lx, ly, blank=blank, reduction="sum").backward()
                    return lf.grad, lg.grad

                def joint():
                    lf, lg = f.detach().requires_grad_(True), g.detach().requires_grad_(True)
                    ctc_crf.rnnt_loss(lf.unsqueeze(2) + lg.unsqueeze(1), labels, lx, ly, blank=blank, fuse_log_softmax=True, reduction="sum").backward()
                    return lf.grad, lg.grad

                peak, grads = {}, {}
                for side, fn in (("a", simple), ("b", joint)):
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats(dev)
                    before = torch.cuda.max_memory_allocated(dev)
                    grads[side] = fn()
                    torch.cuda.synchronize()
                    peak[side] = round((torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20, 1)
                err = [float((x.double() - y.double()).abs().max()) / float(y.double().abs().max()) for x, y in zip(grads["a"], grads["b"])]
                del grads
                esz = f.element_size()
                shape = dict(N=N, T=T, U=U, V=V, dtype=name, f_and_g_MiB=round((f.numel() + g.numel()) * esz / 2 ** 20, 1),
                             joint_MiB=round(N * T * (U + 1) * V * esz / 2 ** 20, 1), peak_MiB=peak, grad_a_vs_b_over_max_b=dict(df=err[0], dg=err[1]))
                rec = measure("simple_vs_materialised", shape, simple, joint, a.calls, a.warmup, "rnnt_loss_simple(f, g) + backward",
                              "rnnt_loss(f.unsqueeze(2) + g.unsqueeze(1), fuse_log_softmax=True) + backward to f and g")
                rec["speedup"] = round(rec["b"]["median_ms"] / rec["a"]["median_ms"], 2)
                rec["a_below_b"] = bool(rec["b"]["median_ms"] - rec["a"]["median_ms"] > rec["b"]["max_ms"] - rec["b"]["min_ms"])
                print(json.dumps(dict(pair=rec["pair"], speedup=rec["speedup"], a_below_b=rec["a_below_b"])), flush=True)
                out.append(rec)
                del f, g
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
