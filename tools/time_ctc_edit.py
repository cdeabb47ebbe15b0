"""tools/time_ctc_edit.py -- HIP-event timings of ctc_edit_distance (token edit distance and operation counts of N x K hypotheses on the
GPU, one wave per hypothesis) against the two ways a caller has without it (DESIGN.md section 7 (f10) records the output).
`python tools/time_ctc_edit.py [--calls 24] [--warmup 4] [--cpu-calls 2] [--out FILE]`

The callers' own tool, the third-party `Levenshtein` extension (cat/ctc/train.py:200-210), is NOT installed on this machine and is not
measured.  The pairs alternate call by call (A B A B ...) in ONE process, each call between two HIP events on the current stream,
`--calls` >= 20 calls per side after `--warmup`; per side: median and the spread min .. max in ms.

  edit_vs_torch  A: ctc_crf.ctc_edit_distance(hyps, hl, labels, ly, hu, return_ops=True)
                 B: the same distances (NO counts) by a batched anti-diagonal dynamic program in torch ops on the GPU, one step per
                    anti-diagonal over all N K pairs padded to the longest
  edit_vs_host   A: the same call;  B: hyps.cpu().tolist() + tests/edit_ref.py's NumPy anti-diagonal form per utterance -- `--cpu-calls`
                    calls only (each takes seconds), timed by the same events, which then span the host's work

at N = 64 utterances with K = 16 hypotheses each, reference and hypothesis lengths around 250 and around 50 (hypotheses = the reference
with about 15 % errors of the three kinds), rows 1 500 wide as ctc_sample leaves them, 72 symbols.  One JSON line per pair."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_crf  # noqa: E402
from tests import edit_ref  # noqa: E402
from time_ctc_logits import measure  # noqa: E402


def make(N, K, L, W, V, seed):
    rng = np.random.default_rng(seed)
    refs = [rng.integers(1, V, int(rng.integers(L - L // 5, L + L // 5 + 1))).tolist() for _ in range(N)]
    hyps = []
    for n in range(N):
        for _ in range(K):
            y = []
            for t in refs[n]:
                k = rng.random()
                if k < 0.05:
                    continue
                y.append(int(rng.integers(1, V)) if k < 0.10 else t)
                if k > 0.95:
                    y.append(int(rng.integers(1, V)))
            hyps.append(y[:W])
    rows = torch.zeros((N * K, W), dtype=torch.int32)
    for h, y in enumerate(hyps):
        rows[h, :len(y)] = torch.tensor(y, dtype=torch.int32)
    hl = torch.tensor([len(y) for y in hyps], dtype=torch.int32)
    hu = torch.arange(N * K, dtype=torch.int32) // K
    lab = torch.tensor([t for r in refs for t in r], dtype=torch.int32)
    ly = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    return refs, rows.cuda(), hl.cuda(), hu.cuda(), lab, ly


def torch_antidiag(r, yr, Rs, Ys, Rm, Ym):
    """Distances only.  r [H, Rm]: references padded with -1; yr [H, Ym]: hypotheses REVERSED (y_j at column Ym - j), padded with -2."""
    H = r.size(0)
    out = torch.zeros(H, dtype=torch.int32, device=r.device)
    p1 = p2 = None
    for d in range(Rm + Ym + 1):
        cur = torch.zeros((H, Rm + 1), dtype=torch.int32, device=r.device)
        if d <= Ym:
            cur[:, 0] = d
        if d <= Rm:
            cur[:, d] = d
        lo, hi = max(1, d - Ym), min(Rm, d - 1)
        if lo <= hi:
            ne = (r[:, lo - 1:hi] != yr[:, Ym - d + lo:Ym - d + hi + 1]).to(torch.int32)
            cur[:, lo:hi + 1] = torch.minimum(torch.minimum(p2[:, lo - 1:hi] + ne, p1[:, lo - 1:hi] + 1), p1[:, lo:hi + 1] + 1)
        out = torch.where(Rs + Ys == d, cur.gather(1, Rs[:, None])[:, 0], out)
        p2, p1 = p1, cur
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--cpu-calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.calls >= 20 and torch.cuda.is_available()
    core = ctc_crf._C
    out = []
    N, K, W, V = 64, 16, 1500, 72
    for L in (250, 50):
        refs, rows, hl, hu, lab, ly = make(N, K, L, W, V, L)

        def edit():
            return ctc_crf.ctc_edit_distance(rows, hl, lab, ly, hu, return_ops=True)

        # the torch side's operands, staged once outside the timed calls
        Rs = ly.cuda()[hu.long()].long()
        Rm, Ym = int(ly.max()), int(hl.max())
        r = torch.full((N * K, Rm), -1, dtype=torch.int32)
        for n in range(N):
            r[n * K:(n + 1) * K, :len(refs[n])] = torch.tensor(refs[n], dtype=torch.int32)
        r = r.cuda()
        col = torch.arange(Ym, device="cuda")[None, :]
        yr = rows.gather(1, (Ym - 1 - col).expand(N * K, Ym))             # column Ym - j holds y_j = rows[:, j - 1]
        yr = torch.where(col >= Ym - hl[:, None], yr, torch.full_like(yr, -2))

        def by_torch():
            return torch_antidiag(r, yr, Rs, hl, Rm, Ym)

        def by_host():
            lists, lens, utt = rows.cpu().tolist(), hl.cpu().tolist(), hu.cpu().tolist()
            res = np.zeros((N * K, 4), dtype=np.int64)
            for n in range(N):
                mine = [h for h in range(N * K) if utt[h] == n]
                res[mine] = edit_ref.antidiag_batch([refs[n]] * len(mine), [lists[h][:lens[h]] for h in mine])
            return res

        d, s, de, i = edit()
        want = by_host()
        assert np.array_equal(torch.stack([d, s, de, i], 1).cpu().numpy(), want) and bool(torch.equal(by_torch(), d))
        shape = dict(N=N, K=K, W=W, V=V, mean_ref=round(float(ly.float().mean()), 1), mean_hyp=round(float(hl.float().mean()), 1),
                     kernel=core.last_edit_kernel(), wer=round(edit_ref.wer(want[:, 0], [len(refs[n]) for n in range(N) for _ in range(K)]), 4))
        out.append(measure("edit_vs_torch", shape, edit, by_torch, a.calls, a.warmup, "ctc_edit_distance (distance and counts)",
                           "anti-diagonal DP in torch ops on the GPU (distance only)"))
        out.append(measure("edit_vs_host", shape, edit, by_host, a.cpu_calls, 0, "ctc_edit_distance (distance and counts)",
                           ".cpu().tolist() + NumPy anti-diagonal form per utterance (distance and counts)"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
