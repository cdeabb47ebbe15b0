"""tools/time_ctct_loss.py -- HIP-event timings and peak memory of ctc_crf.ctct_loss forward + backward on raw joiner output against what
a caller without warp_ctct can write today: log_softmax(x.float()) and the same recursion frame by frame in plain torch ops,
differentiated by autograd (DESIGN.md section 7 (f17) records the output).
`python tools/time_ctct_loss.py [--calls 20] [--warmup 3] [--out FILE] [--only N,V,dtype]`

Every pair is measured in ONE process with the two sides alternating call by call (A B A B ...), each call between two HIP events on the
current stream (tools/time_ctc_logits.py measure); per side the median and the spread min .. max in milliseconds.  Side A is
ctct_loss(fuse_log_softmax=True, reduction="sum") + backward on the padded (N, T, U+1, V) tensor with the lengths on the device; side B is
the torch recursion on the same tensor.  Shapes, those of tools/time_rnnt_loss.py: N = 16 and 64, T = 250, U = 50, V = 1 024 and 5 000,
bf16 and fp32, every utterance of full length.  Before the timed calls the gradient of both sides is compared, on the first four
utterances, with the same torch recursion in fp64 on the upcast input: max |err| / max |ref|; and one call of each side is run alone
for its peak of allocated device memory above what the input itself takes.  `hbm_share` is the time three passes over the tensor (two
reads, one write) take at the 8 TB/s of the HBM, divided by A's median.  One JSON line per pair."""
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


def torch_ctct(lp, labels, blank):
    """costs [N] of normalised lp [N, T, U1, V] (every utterance of full length), a frame at a time over all columns."""
    N, T, U1, _ = lp.shape
    U = U1 - 1
    pad = torch.nn.functional.pad
    lab = labels.long()[:, None, :, None].expand(N, T, U, 1)
    b = lp[..., blank]                                                            # [N, T, U1]
    e = pad(torch.gather(lp[:, :, :U, :], 3, lab).squeeze(3), (0, 1), value=NEG)  # y_{u+1} at row u: none behind the last label
    r = pad(torch.gather(lp[:, :, 1:, :], 3, lab).squeeze(3), (1, 0), value=NEG)  # y_u at row u: none at row 0
    skip = torch.ones((N, U1), dtype=torch.bool, device=lp.device)                # y_{u+1} may follow y_u directly
    if U >= 2:
        skip[:, 1:U] = labels[:, 1:] != labels[:, :-1]
    ab = torch.full((N, U1), NEG, dtype=lp.dtype, device=lp.device)
    ab[:, 0] = 0.0
    an = torch.full_like(ab, NEG)
    for t in range(T):
        s = torch.logaddexp(ab, an)
        move = pad((torch.where(skip, s, ab) + e[:, t])[:, :-1], (1, 0), value=NEG)
        ab, an = s + b[:, t], torch.logaddexp(an + r[:, t], move)
    return -torch.logaddexp(ab[:, U], an[:, U])


def peak_mib(f):
    """Peak of allocated device memory during one call of f above what is allocated in front of it, in MiB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del g
    return round((peak - base) / 2**20, 1)


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
                labels[:, 1::7] = labels[:, 0:-1:7]                                 # (a repeated label every seven: the no-direct-move rule is on the path)
                lx = torch.full((N,), T, dtype=torch.int32, device=dev)
                ly = torch.full((N,), U, dtype=torch.int32, device=dev)

                def fused():
                    leaf = x.detach().requires_grad_(True)
                    ctc_crf.ctct_loss(leaf, labels, lx, ly, blank=blank, fuse_log_softmax=True, reduction="sum").backward()
                    return leaf.grad

                def plain(n=N, double=False):
                    leaf = x[:n].detach().requires_grad_(True)
                    lp = torch.log_softmax(leaf.double() if double else leaf.float(), -1)
                    torch_ctct(lp, labels[:n], blank).sum().backward()
                    return leaf.grad

                ref = plain(4, True).double()
                top = float(ref.abs().max())
                err = dict(ctct_loss=float((fused()[:4].double() - ref).abs().max()) / top, torch=float((plain(4).double() - ref).abs().max()) / top)
                del ref
                shape = dict(N=N, T=T, U=U, V=V, dtype=str(dtype).split(".")[1], tensor_MiB=round(x.numel() * x.element_size() / 2**20, 1),
                             grad_err_over_max_ref=err, peak_MiB=dict(ctct_loss=peak_mib(fused), torch=peak_mib(plain)))
                roof_ms = 3 * x.numel() * x.element_size() / HBM_BYTES_PER_MS
                rec = measure("ctct_vs_torch", shape, fused, plain, a.calls, a.warmup, "ctct_loss(fuse_log_softmax=True) + backward",
                              "log_softmax(x.float()) + torch frame-by-frame recursion + backward")
                rec["hbm_roof_ms"] = round(roof_ms, 4)
                rec["hbm_share"] = round(roof_ms / rec["a"]["median_ms"], 3)
                rec["speedup"] = round(rec["b"]["median_ms"] / rec["a"]["median_ms"], 2)
                print(json.dumps(dict(pair=rec["pair"], hbm_roof_ms=rec["hbm_roof_ms"], hbm_share=rec["hbm_share"], speedup=rec["speedup"])), flush=True)
                out.append(rec)
                del x
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
