"""The yardstick of ctc_beam_search(lm=...) (a plain helper module): tests/beam_ref.py's `candidates`, `search` and `replay` with the LM
terms of the contract of crf_ctc_beam_lm (include/ctc_crf_hip.h) from the textbook lookup tests/ngram_ref.py, all in fp64: a prefix
carries lm = alpha * log P_lm(prefix) + beta * len, a candidate's score is its acoustic score + lm, and the extensions of one parent are
ordered by x[c] + lmw before their place in E_t.  `audit_ties`, LM_TIE_CASES and LM_ALTERED_ORDERS build and vet the inputs on which exact
ties decide while the LM is live, where only equality with `search` will do."""
import numpy as np

from tests import beam_ref, ngram_ref

NEG = -np.inf


def candidates(beam, row, E, blank, lm, alpha, beta, lse=beam_ref.lse):
    """beam_ref.candidates with, per candidate: ac (the acoustic score), lm, score = ac + lm, and for an extension key = x[c] + lmw."""
    out = beam_ref.candidates(beam, row, E, blank, lse=lse)
    for c in out:
        c["ac"] = c["score"]
        c["lm"] = alpha * lm.score(c["prefix"]) + beta * len(c["prefix"])
        c["score"] = c["ac"] + c["lm"]
        c["key"] = row[c["cls"]] + (alpha * lm.cond(lm.start + c["prefix"][:-1], c["cls"]) + beta) if c["kind"] else 0.0
    return out


def order_key(c):
    """score descending, stay before extension, parent slot ascending, x[c] + lmw descending, then the place in E_t"""
    return (-c["score"], c["kind"], c["parent"], -c["key"], c["place"])


def search(x, lx, W, nbest, C, blank, lm, alpha, beta, normalize=False, lse=beam_ref.lse, on_frame=None, key=None):
    """The contract on one utterance.  -> dict(nbest=[(prefix, fused score, lm)], trace [T, W], gap: the smallest difference of the fused
    scores of adjacent candidates among the ranks 0 .. W over all frames, relative to |acoustic| + |lm| of the lower one).  lse, on_frame
    (t, ALL candidates in the contract's order) and key (another order than `order_key`: negative controls only) as in beam_ref.search."""
    x = np.asarray(x)
    T, V = x.shape
    lx = max(0, min(int(lx), T))
    rows = beam_ref.upcast_rows(x, normalize)
    order = np.asarray(x, dtype=np.float64)
    C = min(C, V - 1)
    beam = [dict(prefix=(), pb=0.0, pnb=NEG)]
    trace = np.full((T, W), -1, dtype=np.int32)
    gap = np.inf
    for t in range(lx):
        E = beam_ref.top_classes(order[t], blank, C)
        cand = sorted(candidates(beam, rows[t], E, blank, lm, alpha, beta, lse), key=key or order_key)
        if on_frame is not None:
            on_frame(t, cand)
        for a, b in zip(cand[:W], cand[1:W + 1]):
            gap = min(gap, (a["score"] - b["score"]) / (abs(b["ac"]) + abs(b["lm"])))
        beam = []
        for k, c in enumerate(cand[:W]):
            trace[t, k] = beam_ref.word(c)
            beam.append(dict(prefix=c["prefix"], pb=c["pb"], pnb=c["pnb"]))
    out = []
    for ent in beam[:nbest]:
        l = alpha * lm.score(ent["prefix"]) + beta * len(ent["prefix"])
        out.append((ent["prefix"], lse(ent["pb"], ent["pnb"]) + l, l))
    return dict(nbest=out, trace=trace, gap=gap)


def audit_ties(x, lx, W, C, blank, lm, alpha, beta, normalize=False, lse=beam_ref.lse):
    """beam_ref.audit_ties on the fused scores: runs the contract and looks, per frame, at the sorted candidates of ranks 0 .. W (the
    first loser included).  -> dict(gap: the smallest difference of the fused scores of adjacent candidates that are not bit-equal, relative
    to |acoustic| + |lm| of the lower one (inf where there is none); stay_ext, slot, place: the bit-equal adjacent pairs by the level of
    the total order that separates them (a stay from an extension, two parent slots, two extensions of one parent); cut: how many of
    those pairs are ranks W - 1 and W; key_level: the pairs of `place` whose keys x[c] + lmw are NOT equal -- the fourth level would
    decide them, on a key the kernel forms from fp32 terms: a vetted case has none, so that its `place` pairs come by the place in E_t;
    reordered: the (frame, parent) pairs in which an extension among those ranks comes BEFORE an extension of the same parent, of any
    rank, at a lower place of E_t -- the LM's term moved the head of that slot's row off the next place; the extension by the parent's own
    last label, whose base is pb and which the LM-free order moves too, is not counted)."""
    out = dict(gap=np.inf, stay_ext=0, slot=0, place=0, cut=0, key_level=0, reordered=0)

    def frame(t, cand):
        for k, (a, b) in enumerate(zip(cand[:W], cand[1:W + 1])):
            if a["score"] != b["score"]:
                out["gap"] = min(out["gap"], (a["score"] - b["score"]) / max(abs(b["ac"]) + abs(b["lm"]), 1e-300))
                continue
            level = "stay_ext" if a["kind"] != b["kind"] else "slot" if a["parent"] != b["parent"] else "place"
            out[level] += 1
            out["cut"] += k == W - 1
            out["key_level"] += level == "place" and a["key"] != b["key"]
        low, jumped = {}, set()
        for k, c in reversed(list(enumerate(cand))):
            if c["kind"] and not (len(c["prefix"]) >= 2 and c["prefix"][-2] == c["cls"]):
                if k <= W and low.get(c["parent"], 64) < c["place"]:
                    jumped.add(c["parent"])
                low[c["parent"]] = min(low.get(c["parent"], 64), c["place"])
        out["reordered"] += len(jumped)

    search(x, lx, W, W, C, blank, lm, alpha, beta, normalize, lse, on_frame=frame)
    return out


def lm_tie_inputs(case):
    """(x [T, V] fp32 values that bf16 holds exactly, the n-gram dict) of one entry of LM_TIE_CASES."""
    seed, V, W, C, T, blank, G, order, alpha, beta, zero_group = case
    x = beam_ref.through(beam_ref.grouped_inputs(seed, T, V, blank, G), "bf16")
    return x, ngram_ref.symmetric_model(seed, V, beam_ref.class_groups(seed, V, G), G, order, zero_group=zero_group)


# The cases of the exact-tie test under a live LM: (seed, V, W, C, T, blank, G, order, alpha, beta, zero_group): `grouped_inputs` through
# bf16 (one set of values for all three input dtypes) with ngram_ref.symmetric_model over the same class-to-group map, taken with
# normalize = False at lx = T, T - 1, 1.  The model's values depend on the groups only, so prefixes that differ by a permutation inside a
# group carry bit-equal (pb, pnb) AND bit-equal lm, in fp64 and in the kernel's fp32 / fp64 mix alike (the same values summed in the same
# order): their candidates tie exactly and the contract's order alone decides, while alpha, beta != 0 move the heads of the rows off the
# place order.  The shapes are those of beam_ref.TIE_CASES; each seed is the first from 1 on (searched on the CPU with `audit_ties`) that
# meets the conditions tests/test_ctc_beam_lm_api.py holds the list to: every pair among the ranks 0 .. W that is not bit-equal differs by
# >= 1e-3 relative, key_level == 0, one trace with `lse` and `lse32`, a trace other than the LM-free one, reordered > 0, and
#   live cases (alpha = 0.5, beta = 1.0, no zero group): slot, place and cut ties, the altered orders "higher slot first" and "higher
#     place first" change the trace;
#   zero-group cases (alpha = 1.5, beta = 0, the classes of one group at log10 p = 0): stay_ext ties as well -- a live model never levels
#     a stay with an extension, which pays lmw -- and both altered orders of that level change the trace too: "an extension before a
#     stay" and "an extension of a LOWER slot before a stay", which is what the kernel's rounds give without their ballot of the stays.
#     Here the search runs over (seed, zero group), the groups 0 .. G - 1 in turn within a seed.
LM_TIE_CASES = [
    (2, 6, 4, 8, 8, 0, 2, 3, 0.5, 1.0, None),
    (2, 6, 8, 3, 10, 5, 2, 3, 0.5, 1.0, None),          # C < V - 1: E_t prunes
    (1, 70, 64, 64, 6, 69, 3, 2, 0.5, 1.0, None),       # W = C = 64: every lane a slot and a place (order 2: 70 classes)
    (3, 5, 2, 4, 12, 1, 2, 3, 0.5, 1.0, None),
    (24, 9, 16, 8, 8, 3, 3, 3, 1.5, 0.0, 0),
    (2, 70, 64, 64, 6, 69, 3, 2, 1.5, 0.0, 2),
]

# the contract's order with one level altered: what a kernel that mis-writes that rule would compute (negative controls)
# name -> (the level of audit_ties it alters, the key)
LM_ALTERED_ORDERS = {
    "an extension before a stay": ("stay_ext", lambda c: (-c["score"], -c["kind"], c["parent"], -c["key"], c["place"])),
    "an extension of a lower slot before a stay": ("stay_ext", lambda c: (-c["score"], c["parent"], c["kind"], -c["key"], c["place"])),
    "the higher slot first": ("slot", lambda c: (-c["score"], c["kind"], -c["parent"], -c["key"], c["place"])),
    "the higher place first": ("place", lambda c: (-c["score"], c["kind"], c["parent"], -c["key"], -c["place"])),
}


def replay(x, lx, trace, W, C, blank, lm, alpha, beta, normalize=False):
    """beam_ref.replay on the fused scores.  The excess of an unchosen candidate over the lowest chosen one is measured relative to
    |acoustic score| + |lm| of that chosen candidate, so that a fused score near 0 does not inflate it.  -> dict(excess, prefixes, scores
    (fused, fp64), lms, why)."""
    x = np.asarray(x)
    T, V = x.shape
    lx = max(0, min(int(lx), T))
    rows = beam_ref.upcast_rows(x, normalize)
    order = np.asarray(x, dtype=np.float64)
    C = min(C, V - 1)
    beam = [dict(prefix=(), pb=0.0, pnb=NEG)]
    excess, why = 0.0, None

    def bad(reason):
        nonlocal excess, why
        excess = np.inf
        why = why or reason

    for t in range(lx):
        E = beam_ref.top_classes(order[t], blank, C)
        cand = {beam_ref.word(c): c for c in candidates(beam, rows[t], E, blank, lm, alpha, beta)}
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
            lo = min(chosen, key=lambda c: c["score"])
            hi = max(c["score"] for c in rest)
            if hi > lo["score"]:
                excess = max(excess, (hi - lo["score"]) / max(abs(lo["ac"]) + abs(lo["lm"]), 1e-300))
        if why:
            break
        beam = [dict(prefix=c["prefix"], pb=c["pb"], pnb=c["pnb"]) for c in chosen]
    if why:
        return dict(excess=excess, prefixes=None, scores=None, lms=None, why=why)
    pad = W - len(beam)
    lms = [alpha * lm.score(ent["prefix"]) + beta * len(ent["prefix"]) for ent in beam]
    sc = [beam_ref.lse(ent["pb"], ent["pnb"]) + l for ent, l in zip(beam, lms)]
    return dict(excess=excess, prefixes=[ent["prefix"] for ent in beam] + [None] * pad, scores=np.array(sc + [NEG] * pad),
                lms=np.array(lms + [0.0] * pad), why=None)


def back_off_case(closed=False, order=5):
    """closed: with the suffixes (1 2 3), (2 3), (1 2) of the chain's contexts as n-grams of their own, so that the walk from the state
    of (0 1 2 3) passes the states (1 2 3), (2 3), (3) -- four sparse rows, then the root's; without, the compiled walk skips the
    contexts the model does not hold ((0 1 2 3) -> (3) -> root) as the textbook does with back-off weights of 0.
    An order-5 model of unigrams and ONE 5-gram chain (0 1 2 3 4 with its prefixes, which the format demands): from the state of
    (0 1 2 3) every class but 4 walks four back-offs down to the root, 4 is found at once; from the shorter states 3, 2, 1 back-offs.
    Frames planted so that the beam walks the chain, with a rival of 4 in the frame where the 5-gram is found.
    order: the same with ONE chain 0 .. order - 1 over V = order + 2 classes and T = order + 1 frames -- at order 8, the largest the
    tables take, from the state of (0 .. 6) every class but 7 walks seven back-offs in the suffix-closed form.
    -> (ngrams, x [1, T, V] fp32, (V, W, C, T, blank, alpha, beta))."""
    V, W, C, T, blank = order + 2, 16, order + 1, order + 1, order + 1
    rng = np.random.default_rng(2 if order == 5 else [1, order])     # (the first draws that keep the candidates of both forms >= 1e-5 apart)
    ng = {(c,): (round(-0.3 - float(rng.random()), 3), round(-0.2 - float(rng.random()), 3)) for c in range(V)}
    for n in range(2, order + 1):
        ng[tuple(range(n))] = (round(-0.1 - 0.2 * float(rng.random()), 3), round(-0.5 - float(rng.random()), 3) if n < order else 0.0)
    if closed:
        runs = [tuple(range(i, j + 1)) for i in range(1, order - 1) for j in range(i + 1, order - 1)]
        for k in sorted(runs, key=lambda k: (len(k), k)):
            ng[k] = (round(-0.4 - float(rng.random()), 3), round(-0.3 - float(rng.random()), 3))
    x = np.full((1, T, V), -6.0) - rng.random((1, T, V))
    for t in range(order):
        x[0, t, t] = -0.2
    x[0, order - 1, order] = -0.25
    return ng, x.astype(np.float32), (V, W, C, T, blank, 1.5, 0.5)


def row_edges_case(V=8192):
    """Order 2, T = 2, W = C = 64.  Unigrams for all V classes; bigram contexts: class 1 with V - 1 arcs (every class but the last) and
    classes 10 .. 16 with 0, 1, 2, 3, 63, 64 and 65 arcs at labels spread over the vocabulary.  Frame 0 brings the eight contexts into the
    beam; frame 1's E_t holds, of every row, its first and its last label and a label it does not hold (a neighbour of the first; for the
    widest row class V - 1): the search of a row hits its first and last arc and misses inside and outside it.
    -> (ngrams, rows {context: labels}, x [1, T, V] fp32, (V, W, C, T, blank, alpha, beta))."""
    W, C, T, blank = 64, 64, 2, 5
    rng = np.random.default_rng(8)
    ng = {(c,): (round(-2.0 - 2.0 * float(rng.random()), 4), round(-0.1 - float(rng.random()), 4)) for c in range(V)}
    rows = {1: list(range(0, V - 1))}
    for ctx, n in zip(range(10, 17), (0, 1, 2, 3, 63, 64, 65)):
        rows[ctx] = sorted(int(c) for c in rng.choice(np.arange(20, V), size=n, replace=False))
    for ctx, labels in rows.items():
        for c in labels:
            ng[(ctx, c)] = (round(-0.2 - 1.5 * float(rng.random()), 4), 0.0)
    x = (np.full((1, T, V), -12.0) - rng.random((1, T, V))).astype(np.float32)
    for i, ctx in enumerate(rows):
        x[0, 0, ctx] = -1.0 - 0.11 * i
    E = {0, V - 2, V - 1, 19}
    for ctx, labels in rows.items():
        if ctx != 1 and labels:
            E.update((labels[0], labels[-1], labels[0] + 1 if labels[0] + 1 not in labels else labels[0] - 1))
    E.discard(blank)
    assert len(E) <= C
    for i, c in enumerate(sorted(E)):
        x[0, 1, c] = -1.5 - 0.07 * i
    return ng, rows, x, (V, W, C, T, blank, 1.5, -1.0)
