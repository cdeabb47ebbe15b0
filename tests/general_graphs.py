"""Seeded generators of denominator graphs WITHOUT the T o LM structure, and of T o LM graphs with a few arcs changed (a plain helper
module: tests/test_general_graph_layouts.py, tests/test_gpu_general_graphs.py, tests/test_gpu_guard_bands.py).

Every generator writes an OpenFst binary with cat_amd.den_lm.write_fst and returns (path, oracle.fst_io.read_fst(path)): the graph the
tests hand to the oracle is the one the library's own reader sees.  A class is ilabel - 1; class 0 (the CTC blank) sits on arcs like any
other class.

`general` guarantees, whatever its other arguments:
  * the states [0, live) are strongly connected: a ring i -> (i + 1) % live, plus random arcs among them;
  * dead-end states follow: each is entered from the live part, has no out-arcs and is not final;
  * unreachable states come last: nobody enters them, their arcs lead into the live part;
  * the start state is a parameter (a live state);
  * the state one ring step from the start is final AND carries a self loop, so that a path of every length >= 1 ends in a final state:
    Z > 0 for every utterance of at least one frame;
  * unless `finals` is given, the start state is final too, so that an utterance of no frames has Z > 0 as well.

CATALOGUE names the graphs of the tests by the property each must have; tests/test_general_graph_layouts.py asserts those properties
from crf_graph_stats, so that a change to this file cannot silently lose them."""
import os

import numpy as np

from cat_amd.den_lm import synth_den_lm, write_fst
from oracle import fst_io


def general(path, S, V, start, seed, dead=0, unreach=0, extra=2.0, hubs=0, hub_deg=300, classes=None, finals=None, cost_hi=2.0,
            self_loops=False, dup=0, full_pairs=0):
    """S states over V classes (arcs carry classes < `classes`, default V).  extra: random arcs per live state beside the ring; hubs: that
    many live states are entered by `hub_deg` arcs of ONE class from distinct states and left by `hub_deg` arcs of random classes;
    finals: None -- the start, its ring successor and about a tenth of the live states are final -- or n: the ring successor and n - 1
    other live states (not the start); costs of arcs and final states uniform in [0, cost_hi]; self_loops: every state, dead ends
    excepted, has one; dup: that many arcs appended once more with a cost drawn anew; full_pairs: that many (src, dst) pairs of
    live states joined by one arc of every class."""
    rng = np.random.default_rng(seed)
    C = int(V if classes is None else classes)
    live = S - dead - unreach
    assert live >= 3 and 0 <= start < live and 1 <= C <= V and (hubs == 0 or hub_deg <= live - 1)
    src, dst, lab = [], [], []

    def arc(a, b, c):
        src.append(int(a)); dst.append(int(b)); lab.append(int(c))

    for i in range(live):                                           # the ring
        arc(i, (i + 1) % live, rng.integers(0, C))
    for _ in range(int(round(extra * live))):                       # random arcs among the live states
        arc(rng.integers(0, live), rng.integers(0, live), rng.integers(0, C))
    nxt = (start + 1) % live
    arc(nxt, nxt, rng.integers(0, C))                               # a path of every length >= 1 ends in `nxt`
    hub_ids = []
    for _ in range(hubs):
        h = int(rng.choice([s for s in range(live) if s not in (start, nxt) and s not in hub_ids]))
        hub_ids.append(h)
        c = int(rng.integers(0, C))
        for a in rng.choice([s for s in range(live) if s != h], size=hub_deg, replace=False):
            arc(a, h, c)                                            # one class: ONE forward row of hub_deg arcs
        for b in rng.integers(0, live, size=hub_deg):
            arc(h, b, rng.integers(0, C))
    for d in range(live, live + dead):                              # dead ends: entered, never left
        for _ in range(2):
            arc(rng.integers(0, live), d, rng.integers(0, C))
    for u in range(live + dead, S):                                 # unreachable: nobody enters them
        for _ in range(2):
            arc(u, rng.integers(0, live), rng.integers(0, C))
    if self_loops:
        for s in list(range(live)) + list(range(live + dead, S)):
            if s != nxt:
                arc(s, s, rng.integers(0, C))
    for _ in range(full_pairs):
        a, b = int(rng.integers(0, live)), int(rng.integers(0, live))
        for c in range(C):
            arc(a, b, c)
    cost = list(rng.uniform(0.0, cost_hi, size=len(src)))
    for k in rng.integers(0, len(src), size=dup):                   # the same (src, dst, class) once more with another weight
        arc(src[k], dst[k], lab[k])
        cost.append(rng.uniform(0.0, cost_hi))
    final = np.full(S, np.inf, dtype=np.float32)
    if finals is None:
        fin = set(int(s) for s in rng.integers(0, live, size=max(1, live // 10))) | {start, nxt}
    else:
        others = [s for s in range(live) if s not in (start, nxt)]
        fin = set(int(s) for s in rng.choice(others, size=finals - 1, replace=False)) | {nxt}
    for s in sorted(fin):
        final[s] = rng.uniform(0.0, cost_hi)
    lab = np.asarray(lab, dtype=np.int32)
    write_fst(path, S, start, src, dst, lab + 1, lab + 1, np.asarray(cost, dtype=np.float32), final)
    return path, fst_io.read_fst(path)


# name -> (V of the activations, arguments of `general`); sizes and what each graph is for: tests/test_general_graph_layouts.py
CATALOGUE = {
    "multi": (5, dict(S=64, V=5, start=3, seed=101, dead=2, unreach=2, extra=2.5)),
    "hub": (9, dict(S=400, V=9, start=7, seed=102, extra=2.0, hubs=1)),
    "wide": (40, dict(S=1500, V=40, start=11, seed=103, dead=5, unreach=10, extra=3.2, hubs=2)),
    "lds_edge": (72, dict(S=3000, V=72, start=5, seed=104, extra=2.0, hubs=2)),
    "parallel": (12, dict(S=200, V=12, classes=6, start=9, seed=105, extra=2.0, self_loops=True, dup=40, full_pairs=12)),
    "one_final": (9, dict(S=300, V=9, start=4, seed=106, extra=2.5, finals=1, cost_hi=12.0)),
}


def catalogue(name, directory):
    """(path, graph, V of the activations) of the catalogue graph `name`, written into `directory`."""
    V, kw = CATALOGUE[name]
    path, g = general(os.path.join(str(directory), f"general_{name}.fst"), **kw)
    return path, g, V


KINDS = ("del", "wt", "dup", "add", "relabel", "redirect")
BASES = {"b24": (24, 96, 8, 13), "b40": (40, 300, 6, 3)}             # (vocab, histories, fanout, seed) of synth_den_lm
SEEDS = (1, 2)


def near_tolm(base, kind, seed, path):
    """`base` (a synth_den_lm graph) with three random arcs changed: del -- deleted; wt -- weight lowered by 0.1 ... 1 nat; dup -- a
    copy 0.3 nats lighter appended; add -- a random arc (any source, destination and class of the base's vocabulary) appended; relabel
    -- another class; redirect -- another destination."""
    assert kind in KINDS
    rng = np.random.default_rng(1000 * KINDS.index(kind) + seed)
    S, V = int(base["S"]), int(base["vocab"])
    src, dst, lab = (base[k].astype(np.int64).copy() for k in ("src", "dst", "lab"))
    w = base["w"].astype(np.float64).copy()
    pick = rng.choice(len(src), size=3, replace=False)
    if kind == "del":
        keep = np.ones(len(src), dtype=bool)
        keep[pick] = False
        src, dst, lab, w = src[keep], dst[keep], lab[keep], w[keep]
    elif kind == "wt":
        w[pick] -= rng.uniform(0.1, 1.0, size=3)
    elif kind == "dup":
        src, dst, lab, w = (np.concatenate([a, a[pick]]) for a in (src, dst, lab, w))
        w[-3:] -= 0.3
    elif kind == "add":
        src = np.concatenate([src, rng.integers(0, S, size=3)])
        dst = np.concatenate([dst, rng.integers(0, S, size=3)])
        lab = np.concatenate([lab, rng.integers(0, V, size=3)])
        w = np.concatenate([w, -rng.uniform(0.0, 2.0, size=3)])
    elif kind == "relabel":
        lab[pick] = (lab[pick] + rng.integers(1, V, size=3)) % V
    elif kind == "redirect":
        dst[pick] = (dst[pick] + rng.integers(1, S, size=3)) % S
    write_fst(path, S, int(base["start"]), src, dst, lab + 1, lab + 1, -w.astype(np.float32), -base["end_w"])
    return path, fst_io.read_fst(path)


def near_tolm_case(base_name, kind, seed, directory):
    """(path of the base graph, path of the changed one, changed graph, V)."""
    V, H, d, s = BASES[base_name]
    bp = os.path.join(str(directory), f"tolm_{base_name}.fst")
    base = synth_den_lm(V, H, d, s, path=bp)
    p, g = near_tolm(base, kind, seed, os.path.join(str(directory), f"tolm_{base_name}_{kind}_{seed}.fst"))
    return bp, p, g, V


LX, LX0 = (40, 23, 2, 1), (40, 23, 2, 0)


def batches_of(name):
    """[(tag, sigma, lx, seed)]: the batches the GPU tests run on the catalogue graph `name` (any other name: a near-T o LM graph).
    sigma = 2 for every graph, once more with an utterance of no frames, and sigma = 8 for `hub` and `one_final`.  `one_final` has no
    batch with an empty utterance: its start state is not final, so Z = 0 there."""
    if name not in CATALOGUE:
        return [("s2", 2.0, LX, 77)]
    k = list(CATALOGUE).index(name)
    out = [("s2", 2.0, LX, 10 + k)]
    if name != "one_final":
        out.append(("s2_lx0", 2.0, LX0, 20 + k))
    if name in ("hub", "one_final"):
        out.append(("s8", 8.0, LX, 30 + k))
    return out


def batch(V, sigma, seed, lx=LX, T=40):
    """log_softmax(normal * sigma) [B,T,V] fp32; random labels in [1, V) with ly <= lx // 3 (the utterances of one and two frames
    have none); lx, ly int32."""
    rng = np.random.default_rng(seed)
    lx = np.asarray(lx, dtype=np.int32)
    x = rng.normal(size=(len(lx), T, V)) * sigma
    m = x.max(-1, keepdims=True)
    logits = (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)
    ly = np.array([int(rng.integers(0, n // 3 + 1)) if n >= 3 else 0 for n in lx], dtype=np.int32)
    ly[0] = max(int(ly[0]), 1)
    labels = rng.integers(1, V, size=int(ly.sum())).astype(np.int32)
    return logits, labels, lx, ly
