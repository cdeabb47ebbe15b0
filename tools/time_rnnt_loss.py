"""tools/time_rnnt_loss.py -- HIP-event timings of ctc_crf.rnnt_loss forward + backward on raw joiner output against what a caller
without warp_rnnt can write today: log_softmax(x.float()) and the anti-diagonal recursion in plain torch ops, differentiated by autograd
(DESIGN.md section 7 (f15) records the output).
`python tools/time_rnnt_loss.py [--calls 20] [--warmup 3] [--out FILE] [--only N,V,dtype]`

Every pair is measured in ONE process with the two sides alternating call by call (A B A B ...), each call between two HIP events on the
current stream (tools/time_ctc_logits.py measure); per side the median and the spread min .. max in milliseconds.  Side A is
rnnt_loss(fuse_log_softmax=True, reduction="sum") + backward on the padded (N, T, U+1, V) tensor, or -- `compact` -- on the same rows as
(N T (U+1), V) with the lengths on the device; side B is the torch recursion on the padded tensor.  Shapes: N = 16 and 64, T = 250,
U = 50, V = 1 024 and 5 000, bf16 and fp32, every utterance of full length.  Before the timed calls the gradient of both sides is compared,
on the first four utterances, with the same torch recursion in fp64 on the upcast input: max |err| / max |ref|.  `hbm_share` is the time
three passes over the tensor (two reads, one write) take at the 8 TB/s of the HBM, divided by A's median.  One JSON line per pair."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from time_ctc_logits import measure  # noqa: E402

NEG = -1e30          # stands for -inf in the torch recursion: logaddexp of two -inf has a NaN gradient
HBM_BYTES_PER_MS = 8.0e9


def torch_rnnt(lp, labels, blank):
    """costs [N] of normalised lp [N, T, U1, V] (every utterance of full length) by anti-diagonals: A_d[u] = alpha[d - u][u]."""
    N, T, U1, _ = lp.shape
    U = U1 - 1
    dev = lp.device
    lb = lp[..., blank]                                                           # [N, T, U1]
    ll = torch.gather(lp[:, :, :U, :], 3, labels.long()[:, None, :, None].expand(N, T, U, 1)).squeeze(3)
    ll = torch.nn.functional.pad(ll, (0, 1), value=NEG)                           # [N, T, U1]: no label behind the last one
    D = T + U
    d = torch.arange(D, device=dev)[:, None]
    u = torch.arange(U1, device=dev)[None, :]
    t = d - u
    ok = (t >= 0) & (t < T)
    tc = t.clamp(0, T - 1)
    LB = torch.where(ok, lb[:, tc, u.expand(D, U1)], torch.full((), NEG, dtype=lp.dtype, device=dev))   # [N, D, U1]
    LL = torch.where(ok, ll[:, tc, u.expand(D, U1)], torch.full((), NEG, dtype=lp.dtype, device=dev))
    a = torch.full((N, U1), NEG, dtype=lp.dtype, device=dev)
    a[:, 0] = 0.0
    for k in range(1, D):
        stay = a + LB[:, k - 1]
        move = torch.nn.functional.pad((a + LL[:, k - 1])[:, :-1], (1, 0), value=NEG)
        a = torch.where(ok[k], torch.logaddexp(stay, move), torch.full((), NEG, dtype=lp.dtype, device=dev))
    return -(a[:, U] + lb[:, T - 1, U])


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
                if a.only and a.only != f"{N},{V},{str(dtype).split('.')[1]}":
                    continue
                gen = torch.Generator(device=dev).manual_seed(N + V)
                x = torch.randn((N, T, U + 1, V), device=dev, generator=gen).mul_(2.0).to(dtype)
                labels = torch.randint(1, V, (N, U), device=dev, generator=gen, dtype=torch.int32)
                lx = torch.full((N,), T, dtype=torch.int32, device=dev)
                ly = torch.full((N,), U, dtype=torch.int32, device=dev)
                rows, flat = x.view(-1, V), labels.view(-1)

                def fused(compact=False):
                    leaf = (rows if compact else x).detach().requires_grad_(True)
                    ctc_crf.rnnt_loss(leaf, flat if compact else labels, lx, ly, blank=blank, compact=compact, fuse_log_softmax=True,
                                      reduction="sum").backward()
                    return leaf.grad

                def plain(n=N, double=False):
                    leaf = x[:n].detach().requires_grad_(True)
                    lp = torch.log_softmax(leaf.double() if double else leaf.float(), -1)
                    torch_rnnt(lp, labels[:n], blank).sum().backward()
                    return leaf.grad

                ref = plain(4, True).double()
                top = float(ref.abs().max())
                err = dict(rnnt_loss=float((fused()[:4].double() - ref).abs().max()) / top,
                           rnnt_loss_compact=float((fused(True).view_as(x)[:4].double() - ref).abs().max()) / top,
                           torch=float((plain(4).double() - ref).abs().max()) / top)
                del ref
                shape = dict(N=N, T=T, U=U, V=V, dtype=str(dtype).split(".")[1], tensor_MiB=round(x.numel() * x.element_size() / 2**20, 1),
                             grad_err_over_max_ref=err)
                roof_ms = 3 * x.numel() * x.element_size() / HBM_BYTES_PER_MS
                for name, f in (("padded_vs_torch", lambda: fused(False)), ("compact_vs_torch", lambda: fused(True))):
                    rec = measure(name, shape, f, plain, a.calls, a.warmup, "rnnt_loss(fuse_log_softmax=True) + backward",
                                  "log_softmax(x.float()) + torch anti-diagonals + backward")
                    rec["hbm_roof_ms"] = round(roof_ms, 4)
                    rec["hbm_share"] = round(roof_ms / rec["a"]["median_ms"], 3)
                    rec["speedup"] = round(rec["b"]["median_ms"] / rec["a"]["median_ms"], 2)
                    print(json.dumps(dict(pair=name, hbm_roof_ms=rec["hbm_roof_ms"], hbm_share=rec["hbm_share"], speedup=rec["speedup"])), flush=True)
                    out.append(rec)
                del x, rows
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
