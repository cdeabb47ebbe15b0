"""The yardstick of ctc_beam_search (a plain helper module: tests/test_ctc_beam_api.py, tests/test_gpu_ctc_beam.py): an fp64 NumPy
restatement of the contract of crf_ctc_beam (include/ctc_crf_hip.h), with the beam a dict keyed by label TUPLES.

`search` runs the contract; `replay` follows a GIVEN trace frame by frame, rebuilds that beam's prefixes, computes every candidate of the
contract in fp64 from the fp64 state of the slots the trace chose, and reports by how much an unchosen candidate beats a chosen one --
errors do not cascade, and no case needs to be skipped for a near-tie.  `brute` sums all V^T labellings.  `planted_rows`,
`grouped_inputs` (with `class_groups`, its class-to-group map), `audit_ties` and TIE_CASES build and vet the inputs on which exact ties decide, where only equality with `search` will do."""
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


def lse32(a, b):
    """The kernel's sum (k_beam.hip beam_lse2): fp64 maximum and result, fp32 exp / log of the differences.  `search` takes it as `lse`."""
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + float(np.log(np.exp(np.float32(a - m)) + np.exp(np.float32(b - m))))


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


def candidates(beam, row, E, blank, merge=True, counters=None, lse=lse):
    """Every candidate of one frame.  beam: list of dict(prefix, pb, pnb[, born]) in slot order.  -> list of dict(score, kind (0 stay /
    1 extension), parent, cls, prefix, pb, pnb), unsorted, candidates at -inf dropped.  lse: the sum of two log masses (`lse` or `lse32`)."""
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


def search(x, lx, W, nbest, C, blank, normalize=False, merge=True, lse=lse, on_frame=None, key=None):
    """The contract on one utterance.  x [T, V].  -> dict(nbest=[(prefix tuple, score)] of the ranks the beam holds, up to nbest;
    trace [T, W] int32; merged, reentered: the two event counters).  lse: the arithmetic of a sum of two log masses -- `lse` (fp64
    throughout) or `lse32` (the kernel's); on_frame(t, candidates in the contract's order, ALL of them) is called once per frame; key:
    another order than the contract's `order_key` -- for the negative controls of the tie cases only."""
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
        cand = sorted(candidates(beam, rows[t], E, blank, merge, counters, lse), key=key or order_key)
        if on_frame is not None:
            on_frame(t, cand)
        new = []
        for k, c in enumerate(cand[:W]):
            trace[t, k] = word(c)
            new.append(dict(prefix=c["prefix"], pb=c["pb"], pnb=c["pnb"], born=beam[c["parent"]]["born"] if c["kind"] == 0 else t))
        beam = new
    return dict(nbest=[(ent["prefix"], lse(ent["pb"], ent["pnb"])) for ent in beam[:nbest]], trace=trace, **counters)


def audit_ties(x, lx, W, C, blank, normalize=False):
    """Runs the contract and looks, per frame, at the sorted candidates of ranks 0 .. W (the first loser included).  -> dict(gap: the
    smallest relative difference (a - b) / |b| between adjacent candidates whose scores are not bit-equal (inf where there is none);
    stay_ext, slot, place: the bit-equal adjacent pairs by the level of the total order that separates them (a stay from an extension,
    two parent slots, two places in E_t of one parent); cut: how many of those pairs are ranks W - 1 and W -- a tie the beam's edge cuts)."""
    out = dict(gap=np.inf, stay_ext=0, slot=0, place=0, cut=0)

    def frame(t, cand):
        for k, (a, b) in enumerate(zip(cand[:W], cand[1:W + 1])):
            if a["score"] != b["score"]:
                out["gap"] = min(out["gap"], (a["score"] - b["score"]) / max(abs(b["score"]), 1e-300))
                continue
            out["stay_ext" if a["kind"] != b["kind"] else "slot" if a["parent"] != b["parent"] else "place"] += 1
            out["cut"] += k == W - 1

    search(x, lx, W, W, C, blank, normalize, on_frame=frame)
    return out


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


def through(a, dtype):
    """a rounded to `dtype` ("fp32", "bf16", "fp16"; to nearest, ties to even) and back: fp32 values the dtype holds exactly."""
    a = np.asarray(a, dtype=np.float32)
    if dtype == "fp32":
        return a.copy()
    if dtype == "fp16":
        return a.astype(np.float16).astype(np.float32)
    assert dtype == "bf16", dtype
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


PLANTED_LOGPROB_ONLY = ("zeros",)      # the rows of planted_rows that are for normalize = False only


def planted_rows(V, dtype, blank=0, C=64, seed=0):
    """Rows [V] (fp32 values that `dtype` holds exactly) whose E_t the row stage can only get right with every one of its tie rules, as a
    list of (name, row).  V >= 64.  The background is -8 - U(0, 1) through the dtype; the planted values are the levels -(k + 1) / 16
    (exact in bf16), best first: ONE class at level 0, then PAIRS of classes at equal values -- so with an even C the value at place C - 1
    of E_t is also that of place C, the first class left out.  With Ce = min(C, V - 1):
      column  Ce + 3 classes (or as many as there are) of ONE column v & 63, the one with the most non-blank classes: every round of the
              row stage strikes an entry of the same lane and needs the re-scan.  The pairs are (v, v + 64) -- one lane of the first pass,
              neighbouring lanes of the re-scan -- and, for V > 4096, (v, v + 4096) -- one lane of the re-scan, its second step -- in
              turns, so E_t has members on both sides of 4096.  The blank is at -30.
      spread  Ce + 2 classes anywhere (V > 4096: the highest non-blank class among them, half of them from either side of 4096); the
              blank is ON TOP (-1/32).
      sparse  fewer than Ce classes above -inf (at most 5, a pair (v, v + 64) among them), everything else at -inf, the blank at -30.
      zeros   -0.0, +0.0, -0.0 (V > 4096: and +0.0) in index order on top -- one value, so they come by index -- at v, v + 64 (a second
              column where V = 64), a third column and, for V > 4096, v + 4096; the levels below them, the blank at -30.  For
              normalize = False only."""
    assert V >= 64 and 0 <= blank < V
    rng = np.random.default_rng([seed, V, C, blank])
    Ce = min(C, V - 1)
    rows = []

    def background():
        return through(-8.0 - rng.random(V), dtype)

    def plant(row, order):
        for q, v in enumerate(order):
            row[v] = -((q + 1) // 2 + 1) / 16.0

    # column
    row = background()
    members = [[v for v in range(col, V, 64) if v != blank] for col in range(64)]
    most = max(len(m) for m in members)
    cols = [col for col in range(64) if len(members[col]) == most]
    col = cols[(5 * len(cols)) // 8]
    mset, used, far, near = set(members[col]), set(), [], []
    for i in range(0, 64, 2):
        v0, v1 = col + 64 * i, col + 64 * (i + 1)
        todo = [(v0, v0 + 4096), (v1, v1 + 4096)] if V > 4096 and (i // 2) % 2 == 0 else [(v0, v1), (v0 + 4096, v1 + 4096)]
        for a, b in todo:
            if a in mset and b in mset and a not in used and b not in used:
                (far if b - a == 4096 else near).append((a, b))
                used.update((a, b))
    far = [far[i] for i in rng.permutation(len(far))]
    near = [near[i] for i in rng.permutation(len(near))]
    pairs = [p for ab in itertools.zip_longest(far, near) for p in ab if p is not None]
    flat = [v for p in pairs for v in p] + [v for v in members[col] if v not in used]
    plant(row, (flat[-1:] + flat[:-1])[:Ce + 3])
    row[blank] = -30.0
    rows.append(("column", row))

    # spread
    row = background()
    others = np.array([v for v in range(V) if v != blank])
    K = min(Ce + 2, V - 1)
    if others[-1] >= 4096 and K >= 4:
        lo, hi = others[others < 4096], others[others >= 4096][:-1]
        nhi = min(K // 2 - 1, len(hi))
        pick = np.concatenate([others[-1:], rng.choice(hi, nhi, replace=False), rng.choice(lo, K - 1 - nhi, replace=False)])
    else:
        pick = rng.choice(others, K, replace=False)
    plant(row, [int(v) for v in rng.permutation(pick)])
    row[blank] = -1.0 / 32
    rows.append(("spread", row))

    # sparse
    row = np.full(V, NEG, dtype=np.float32)
    nfin = max(1, min(5, Ce - 1))
    a = int(others[(blank + 11) % len(others)])
    pick = [a] + ([a + 64] if a + 64 < V and a + 64 != blank and nfin >= 2 else [])
    rest = [int(v) for v in rng.permutation(others) if v not in pick]
    pick = rest[:1] + pick + rest[1:]              # (the pair takes places 1 and 2: one value)
    plant(row, pick[:nfin])
    row[blank] = -30.0
    rows.append(("sparse", row))

    # zeros
    row = background()
    a = (blank + 3) & 63
    b = a + 64 if a + 64 < V and a + 64 != blank else (blank + 7) & 63
    c = (blank + 40) & 63
    zeros = sorted([a, b, c] + ([a + 4096] if a + 4096 < V and a + 4096 != blank else []))
    rest = [int(v) for v in rng.permutation(others) if v not in zeros]
    plant(row, rest[:min(Ce + 2, len(rest))])
    for i, v in enumerate(zeros):
        row[v] = 0.0 if i & 1 else -0.0            # (the lowest index holds -0.0: an order by the bits would put +0.0 first)
    row[blank] = -30.0
    rows.append(("zeros", row))
    for name, row in rows:
        assert np.array_equal(through(row, dtype).view(np.int32), row.view(np.int32)), name
    return rows


def class_groups(seed, V, groups, rng=None):
    """The group of every class [V] as `grouped_inputs` draws it for this seed (the first draw of its generator; rng: that generator)."""
    rng = np.random.default_rng(seed) if rng is None else rng
    return rng.permutation(np.arange(V) % groups)


def grouped_inputs(seed, T, V, blank, groups):
    """fp32 rows [T, V] (taken with normalize = False) with EXACT ties between candidates: every class belongs to one of `groups` groups
    for the whole utterance, per frame each group has one random value in about [-3.3, -0.3] that all its classes share; in every second
    frame the blank has a value of its own.  Prefixes that differ by a permutation inside a group carry bit-equal (pb, pnb) in any
    arithmetic, so their candidates tie exactly and only the total order of the contract decides; any other equality has probability 0."""
    rng = np.random.default_rng(seed)
    group = class_groups(seed, V, groups, rng)
    x = (-0.3 - 3.0 * rng.random((T, groups)))[:, group]
    own = -0.3 - 3.0 * rng.random(T)
    x[1::2, blank] = own[1::2]
    return x.astype(np.float32)


# The seeded cases of the GPU replay test: (seed, V, W, C, T, lx per utterance, blank).  Checked on the CPU to raise both event counters
# (tests/test_ctc_beam_api.py), run on the GPU by tests/test_gpu_ctc_beam.py.
# The seeds are the first ones (searched on the CPU, by this module's own `search`) at which the case raises the events it can raise:
# every case with W >= 2 and more than one frame merges an extension into a beam prefix, and the narrow beams over two labels -- the
# drop-and-re-enter path -- also see a prefix that left the beam and came back merge into a child that had stayed.  (With inputs of this
# kind that second event is rare: at V = 3, W = 2 seed 794 is the first of the seeds from 1 on that shows it; at V >= 65 none of the first
# 12 does, and a search there costs seconds per seed.)
# Inputs of this kind hold no exact tie between two candidates, and `replay` counts a tie as excess 0 whichever way it went: the total
# order of the contract on ties is held by TIE_CASES (below), wide rows and the row stage's tie rules by `planted_rows`.
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
    (1, 9, 64, 8, 130, (130, 129, 128, 65, 64, 1), 4),   # W = 64 with a back-trace of three 64-frame chunks, of two, to and off a boundary
]

# The cases of the exact-tie test: (seed, V, W, C, T, blank, groups) of `grouped_inputs`, taken with normalize = False at lx = T, T - 1, 1.
# Each is the first seed from 1 on (searched on the CPU with `audit_ties`) at which, over the T frames, every level of the total order
# separates at least one pair of bit-equal candidates among the ranks 0 .. W -- a stay from an extension, two parent slots, two places of
# one parent -- at least one such pair is cut by the beam's edge (ranks W - 1 and W), every pair that is NOT bit-equal differs by >= 1e-3
# relative (ten times the bound on a kernel score: fp32 exp / log inside the sums reorders nothing but an exact tie), and `search` gives
# one trace with `lse` and with `lse32`.  The last two prune (C < V - 1), which is what brings a stay in one slot level with an extension
# of ANOTHER, lower slot, and a prefix' extension by its own last label level with the head of its list (a stay whose label was pruned has
# pnb = -inf): their seeds are the first at which, beyond the above, every altered order of tests/test_ctc_beam_api.py changes the trace.
TIE_CASES = [
    (1, 6, 4, 8, 8, 0, 2),
    (1, 6, 8, 3, 10, 5, 2),
    (1, 9, 16, 8, 8, 3, 3),
    (1, 70, 64, 64, 6, 69, 3),                      # W = C = 64: every lane a slot and a place
    (5, 5, 2, 4, 12, 1, 2),
    (7, 9, 16, 2, 10, 0, 3),
    (2, 8, 4, 2, 11, 4, 2),
]
