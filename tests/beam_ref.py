"""The yardstick of ctc_beam_search (a plain helper module: tests/test_ctc_beam_api.py, tests/test_gpu_ctc_beam.py): an fp64 NumPy
restatement of the contract of crf_ctc_beam (include/ctc_crf_hip.h), with the beam a dict keyed by label TUPLES.

`search` runs the contract; `replay` follows a GIVEN trace frame by frame, rebuilds that beam's prefixes, computes every candidate of the
contract in fp64 from the fp64 state of the slots the trace chose, and reports by how much an unchosen candidate beats a chosen one --
errors do not cascade, and no case needs to be skipped for a near-tie.  `brute` sums all V^T labellings."""
import itertools
import math

import numpy as np

NEG = -np.inf


def lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(min(a, b) - m))


def upcast_rows(x, normalize):
    """x [T, V] any float dtype -> fp64 rows as the call takes them: log_softmax of the upcast values with normalize."""
    x = np.asarray(x, dtype=np.float64)
    if normalize:
        m = x.max(-1, keepdims=True)
        x = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    return x


def top_classes(order_row, blank, C):
    """E_t as a list: the C non-blank classes of largest value (of `order_row`: the upcast values), equal values to the lower index first."""
    idx = [v for v in np.lexsort((np.arange(len(order_row)), -np.asarray(order_row, dtype=np.float64))) if v != blank]
    return [int(v) for v in idx[:C]]


def candidates(beam, row, E, blank, merge=True, counters=None):
    """Every candidate of one frame.  beam: list of dict(prefix, pb, pnb[, born]) in slot order.  -> list of dict(score, kind (0 stay /
    1 extension), parent, cls, prefix, pb, pnb), unsorted, candidates at -inf dropped."""
    slot = {ent["prefix"]: i for i, ent in enumerate(beam)}
    pos = {c: j for j, c in enumerate(E)}
    stays = []
    for i, ent in enumerate(beam):
        e = ent["prefix"][-1] if ent["prefix"] else None
        tot = lse(ent["pb"], ent["pnb"])
        stays.append(dict(kind=0, parent=i, cls=-1, place=-1, prefix=ent["prefix"], pb=row[blank] + tot,
                          pnb=row[e] + ent["pnb"] if e in pos else NEG))
    exts = []
    for i, ent in enumerate(beam):
        e = ent["prefix"][-1] if ent["prefix"] else None
        tot = lse(ent["pb"], ent["pnb"])
        for c in E:
            v = row[c] + (ent["pb"] if c == e else tot)
            child = ent["prefix"] + (c,)
            if merge and child in slot:
                k = slot[child]
                stays[k]["pnb"] = lse(stays[k]["pnb"], v)
                if counters is not None and v > NEG:
                    counters["merged"] += 1
                    if ent.get("born", 0) > beam[k].get("born", 0):
                        counters["reentered"] += 1
            else:
                exts.append(dict(kind=1, parent=i, cls=c, place=pos[c], prefix=child, pb=NEG, pnb=v))
    out = stays + exts
    for c in out:
        c["score"] = lse(c["pb"], c["pnb"])
    return [c for c in out if c["score"] > NEG]


def order_key(c):
    """score descending, stay before extension, parent slot ascending, then the place in E_t (equal values: class ascending)"""
    return (-c["score"], c["kind"], c["parent"], c["place"])


def word(c):
    return c["parent"] + 64 * (c["cls"] + 1)


def search(x, lx, W, nbest, C, blank, normalize=False, merge=True):
    """The contract on one utterance.  x [T, V].  -> dict(nbest=[(prefix tuple, score)] of the ranks the beam holds, up to nbest;
    trace [T, W] int32; merged, reentered: the two event counters)."""
    x = np.asarray(x)
    T, V = x.shape
    lx = max(0, min(int(lx), T))
    rows = upcast_rows(x, normalize)
    order = np.asarray(x, dtype=np.float64)
    C = min(C, V - 1)
    beam = [dict(prefix=(), pb=0.0, pnb=NEG, born=-1)]
    trace = np.full((T, W), -1, dtype=np.int32)
    counters = dict(merged=0, reentered=0)
    for t in range(lx):
        E = top_classes(order[t], blank, C)
        cand = sorted(candidates(beam, rows[t], E, blank, merge, counters), key=order_key)[:W]
        new = []
        for k, c in enumerate(cand):
            trace[t, k] = word(c)
            new.append(dict(prefix=c["prefix"], pb=c["pb"], pnb=c["pnb"], born=beam[c["parent"]]["born"] if c["kind"] == 0 else t))
        beam = new
    return dict(nbest=[(ent["prefix"], lse(ent["pb"], ent["pnb"])) for ent in beam[:nbest]], trace=trace, **counters)


def spell(trace, lx, W):
    """The prefixes a trace spells: [(prefix tuple) or None per slot] after frame lx - 1."""
    beam = [()] + [None] * (W - 1)
    for t in range(lx):
        new = []
        for k in range(W):
            w = int(trace[t, k])
            if w < 0:
                new.append(None)
                continue
            par, c = w & 63, (w >> 6) - 1
            assert par < W and beam[par] is not None, ("the trace names an empty slot", t, k, w)
            new.append(beam[par] if c < 0 else beam[par] + (c,))
        beam = new
    return beam


def replay(x, lx, trace, W, C, blank, normalize=False):
    """Follow `trace` [T, W] on x [T, V].  -> dict(excess: the largest (unchosen score - chosen score) / |chosen score| over all frames and
    all pairs of a finite unchosen and a chosen candidate (0 where no unchosen one beats a chosen one; inf where the trace is not a
    selection among the contract's candidates at all: a word that names no candidate, a prefix twice in the beam, an empty slot in front
    of a used one or beside a finite unchosen candidate), prefixes: per slot the prefix after frame lx - 1 or None, scores: their fp64
    scores (-inf for an empty slot), why: the first reason for an infinite excess)."""
    x = np.asarray(x)
    T, V = x.shape
    lx = max(0, min(int(lx), T))
    rows = upcast_rows(x, normalize)
    order = np.asarray(x, dtype=np.float64)
    C = min(C, V - 1)
    beam = [dict(prefix=(), pb=0.0, pnb=NEG)]
    excess, why = 0.0, None

    def bad(reason):
        nonlocal excess, why
        excess = np.inf
        why = why or reason

    for t in range(lx):
        E = top_classes(order[t], blank, C)
        cand = {word(c): c for c in candidates(beam, rows[t], E, blank)}
        words = [int(w) for w in trace[t, :W]]
        used = [w for w in words if w >= 0]
        if words[:len(used)] != used:
            bad(f"frame {t}: an empty slot in front of a used one")
        if len(set(used)) != len(used):
            bad(f"frame {t}: a candidate taken twice")
        chosen = []
        for w in used:
            if w not in cand:
                bad(f"frame {t}: word {w} names no candidate of the contract")
            else:
                chosen.append(cand[w])
        if len({c["prefix"] for c in chosen}) != len(chosen):
            bad(f"frame {t}: a prefix twice in the beam")
        rest = [c for w, c in cand.items() if w not in set(used)]
        if rest and len(used) < W:
            bad(f"frame {t}: {W - len(used)} slots empty beside {len(rest)} finite candidates")
        if rest and chosen:
            lo = min(c["score"] for c in chosen)
            hi = max(c["score"] for c in rest)
            if hi > lo:
                excess = max(excess, (hi - lo) / max(abs(lo), 1e-300))
        if why:
            break
        beam = [dict(prefix=c["prefix"], pb=c["pb"], pnb=c["pnb"]) for c in chosen]
    if why:
        return dict(excess=excess, prefixes=None, scores=None, why=why)
    pre = [ent["prefix"] for ent in beam] + [None] * (W - len(beam))
    sc = [lse(ent["pb"], ent["pnb"]) for ent in beam] + [NEG] * (W - len(beam))
    return dict(excess=excess, prefixes=pre, scores=np.array(sc), why=None)


def collapse(path, blank):
    return tuple(c for c, _ in itertools.groupby(path) if c != blank)


def brute(x, lx, blank, normalize=False):
    """{label tuple: log of the sum over all V^lx labellings that collapse to it} in fp64."""
    x = np.asarray(x)
    lx = max(0, min(int(lx), x.shape[0]))
    rows = upcast_rows(x, normalize)[:lx]
    V = x.shape[1]
    acc = {}
    for path in itertools.product(range(V), repeat=lx):
        lp = float(sum(rows[t, c] for t, c in enumerate(path)))
        acc.setdefault(collapse(path, blank), []).append(lp)
    out = {}
    for k, v in acc.items():
        v = np.array(v)
        m = v.max()
        out[k] = float(m + np.log(np.exp(v - m).sum())) if m > NEG else NEG
    return out


def make_inputs(seed, B, T, V, scale=2.0):
    """log_softmax(normal * scale) as the score tests take it: fp32 [B, T, V]."""
    rng = np.random.default_rng(seed)
    x = scale * rng.standard_normal((B, T, V))
    m = x.max(-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)


# The seeded cases of the GPU replay test: (seed, V, W, C, T, lx per utterance, blank).  Checked on the CPU to raise both event counters
# (tests/test_ctc_beam_api.py), run on the GPU by tests/test_gpu_ctc_beam.py.
# The seeds are the first ones (searched on the CPU, by this module's own `search`) at which the case raises the events it can raise:
# every case with W >= 2 and more than one frame merges an extension into a beam prefix, and the narrow beams over two labels -- the
# drop-and-re-enter path -- also see a prefix that left the beam and came back merge into a child that had stayed.  (With inputs of this
# kind that second event is rare: at V = 3, W = 2 seed 794 is the first of the seeds from 1 on that shows it; at V >= 65 none of the first
# 12 does, and a search there costs seconds per seed.)
REPLAY_CASES = [
    (1, 2, 1, 1, 17, (17, 0, 1, 9), 0),             # W = 1: nothing can merge
    (794, 3, 2, 8, 30, (30, 30, 1, 0), 0),          # the drop-and-re-enter path: a narrow beam over two labels
    (1, 3, 3, 40, 30, (30, 29, 17, 30), 2),
    (4, 3, 4, 64, 30, (30, 30, 30, 5), 1),
    (1, 5, 4, 1, 64, (64, 33, 0, 1), 4),
    (2, 5, 16, 8, 64, (64, 64, 17, 63), 0),
    (1, 65, 64, 64, 64, (64, 1, 40), 64),           # W = C = 64 = V - 1: every lane a slot and a class
    (1, 72, 16, 40, 150, (150, 149, 64, 0), 0),
    (1, 72, 64, 8, 17, (17, 16, 1), 71),
    (3, 300, 16, 40, 64, (64, 17, 1, 0), 299),
    (40, 300, 2, 64, 17, (17, 17), 7),
    (1, 65, 4, 40, 150, (150, 1, 0, 77), 3),
    (1, 2, 64, 64, 1, (1, 0), 1),                   # one frame: the widest beam on the smallest row
]
