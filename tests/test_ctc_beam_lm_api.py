"""CPU tests (no GPU) of ctc_beam_search(lm=...): the exports, crf_ngram_tables_check on corrupted host tables, the argument errors of the
Python binding and of crf_ctc_beam_lm answered before any HIP call (include/ctc_crf_hip.h), the yardstick tests/beam_lm_ref.py against
brute force and against tests/beam_ref.py at zero weights, the planted inputs of the GPU tests with the separation they must have, and
the exact-tie cases under a live LM (beam_lm_ref.LM_TIE_CASES) with the conditions they must meet and the altered orders they must tell apart."""
import ctypes

import numpy as np
import pytest
import torch

from tests import beam_lm_ref, beam_ref, ngram_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ngram_tables_check", "crf_ctc_beam_lm_workspace_bytes", "crf_ctc_beam_lm")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


@pytest.fixture(scope="module")
def lm():
    import ctc_crf
    return ctc_crf.NgramLM.from_ngrams(ngram_ref.random_model(1, 8, 3), 8)


def test_symbols_exported_and_surface(core):
    import inspect
    import ctc_crf
    import cat_amd.ctc_crf
    import cat_amd.ngram_lm
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = open(core.LIB_PATH.rsplit("/cat_amd/", 1)[0] + "/include/ctc_crf_hip.h").read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in core.EXPORTED_SYMBOLS and s + "(" in hdr, s
    assert ctc_crf.NgramLM is cat_amd.ctc_crf.NgramLM is cat_amd.ngram_lm.NgramLM
    par = inspect.signature(ctc_crf.ctc_beam_search).parameters
    assert list(par)[-4:] == ["lm", "alpha", "beta", "return_lm_scores"]
    assert (par["lm"].default, par["alpha"].default, par["beta"].default, par["return_lm_scores"].default) == (None, 0.0, 0.0, False)
    for doc in (ctc_crf.ctc_beam_search.__doc__, cat_amd.ngram_lm.__doc__, hdr):
        for out_of_scope in ("end-of-sentence", "word-level", "binary", "ctc_sample"):
            assert out_of_scope in doc, out_of_scope
    ws, ws0 = core._lib.crf_ctc_beam_lm_workspace_bytes, core._lib.crf_ctc_beam_workspace_bytes
    for shape in ((1, 1, 2, 1, 1), (3, 150, 72, 16, 40), (2, 6, 8192, 64, 64)):
        assert ws(*shape) == ws0(*shape) > 0
    assert ws(2, 10, 8193, 4, 4) == -1 and ws(2, 10, 8, 65, 4) == -1


def _check(core, lm, **change):
    """crf_ngram_tables_check on host copies with one entry changed: table name -> (index, value), or a scalar's name -> value."""
    hold = {n: np.ascontiguousarray(a).copy() for n, a in lm.host_tables().items()}
    scal = dict(S=lm.num_states, A=lm.num_arcs, V=lm.vocab_size, order=lm.order, start=lm.start)
    for k, v in change.items():
        if k in hold:
            hold[k][v[0]] = v[1]
        else:
            scal[k] = v
    import cat_amd.ngram_lm as m
    st = m._Tables(*[hold[n].ctypes.data for n in m.TABLE_NAMES], scal["S"], scal["A"], scal["V"], scal["order"], scal["start"])
    rc = core._lib.crf_ngram_tables_check(ctypes.byref(st))
    return rc, core._lib.crf_last_error().decode()


def test_tables_check_names_the_first_offending_entry(core, lm):
    assert _check(core, lm)[0] == OK
    S, A, V = lm.num_states, lm.num_arcs, lm.vocab_size
    s = next(s for s in range(1, S) if lm.row_off[s + 1] - lm.row_off[s] >= 2)          # a row of two arcs or more
    i = int(lm.row_off[s])
    cases = [
        (dict(arc_label=(i + 1, int(lm.arc_label[i]))), f"arc_label[{i + 1}] = {int(lm.arc_label[i])} does not ascend in row {s}"),   # an unsorted row
        (dict(arc_label=(A - 1, V)), f"arc_label[{A - 1}] = {V} outside [0, V={V})"),
        (dict(bo_state=(3, 3)), "bo_state[3] = 3 is not below its state"),
        (dict(arc_next=(2, S)), f"arc_next[2] = {S} outside [0, S={S})"),
        (dict(arc_logp=(1, np.nan)), "arc_logp[1] is not finite"),
        (dict(bo_weight=(2, np.inf)), "bo_weight[2] is not finite"),
        (dict(uni_logp=(V - 1, np.nan)), f"uni_logp[{V - 1}] is not finite"),
        (dict(uni_next=(0, -1)), "uni_next[0] = -1 outside"),
        (dict(order=9), "order 9 outside [1, 8]"),
        (dict(order=0), "order 0 outside [1, 8]"),
        (dict(row_off=(S, A - 1)), f"row_off[{S}] = {A - 1}"),
        (dict(row_off=(s + 1, int(lm.row_off[s]) - 1)), f"row_off[{s + 1}] = {int(lm.row_off[s]) - 1} is below"),
        (dict(start=S), f"start {S} outside [0, S={S})"),
    ]
    for change, msg in cases:
        rc, got = _check(core, lm, **change)
        assert rc == ERR_ARG and got.startswith("crf_ngram_tables_check: ") and msg in got, (change, rc, got)
    assert core._lib.crf_ngram_tables_check(None) == ERR_ARG


PTRS = dict(act=0x1000, lx=0x2000, hyps=0x3000, len=0x4000, score=0x5000, trace=0x6000, ws=0x7000, lm_score=0x8000)


def _call(core, ptrs=None, dtype=0, blank=0, normalize=0, B=2, T=10, V=8, W=4, nbest=2, C=5, ws_bytes=None, alpha=0.5, beta=1.0, lm="fake", **tab):
    """crf_ctc_beam_lm with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    import cat_amd.ngram_lm as m
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    f = dict(S=5, A=7, V=8, order=3, start=1, **{n: 0x9000 + 0x100 * i for i, n in enumerate(m.TABLE_NAMES)})
    f.update(tab)
    st = m._Tables(*[f[n] for n in m.TABLE_NAMES], f["S"], f["A"], f["V"], f["order"], f["start"])
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_beam_lm_workspace_bytes(B, T, V, W, C))
    rc = core._lib.crf_ctc_beam_lm(vp(p["act"]), dtype, 0, blank, normalize, vp(p["lx"]), B, T, V, W, nbest, C, ctypes.byref(st) if lm else None,
                                   alpha, beta, vp(p["hyps"]), vp(p["len"]), vp(p["score"]), vp(p["lm_score"]), vp(p["trace"]), vp(p["ws"]),
                                   ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_c_abi_argument_errors_without_gpu(core):
    for name in ("act", "lx", "hyps", "len", "score", "ws"):
        rc, msg = _call(core, {name: 0})
        assert rc == ERR_ARG and "crf_ctc_beam_lm" in msg and "null" in msg, (name, rc, msg)
    rc, msg = _call(core, lm=None)
    assert rc == ERR_ARG and "null" in msg
    for kw, word in ((dict(dtype=3), "dtype"), (dict(normalize=2), "normalize"), (dict(blank=8), "blank"), (dict(W=65, nbest=1, ws_bytes=1 << 20), "beam width"),
                     (dict(C=0, ws_bytes=1 << 20), "top_classes"), (dict(nbest=5), "nbest"), (dict(B=0, ws_bytes=1 << 20), "B/T/V")):
        rc, msg = _call(core, **kw)
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)
    rc, msg = _call(core, V=8193, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "8192" in msg
    for kw in (dict(alpha=float("nan")), dict(alpha=float("inf")), dict(beta=float("-inf")), dict(beta=float("nan"))):
        rc, msg = _call(core, **kw)
        assert rc == ERR_ARG and "finite" in msg, (kw, rc, msg)
    rc, msg = _call(core, V=9)
    assert rc == ERR_ARG and "LM's V 8" in msg and "V 9" in msg, msg
    for tab in (dict(S=0), dict(order=0), dict(order=9), dict(start=5), dict(start=-1), dict(A=-1)):
        rc, msg = _call(core, **tab)
        assert rc == ERR_ARG and "bad LM tables" in msg and str(list(tab.values())[0]) in msg, (tab, rc, msg)
    for name in ("row_off", "arc_label", "bo_state", "bo_weight", "uni_logp", "uni_next"):
        rc, msg = _call(core, **{name: 0})
        assert rc == ERR_ARG and "null LM table" in msg, (name, rc, msg)
    need = core._lib.crf_ctc_beam_lm_workspace_bytes(2, 10, 8, 4, 5)
    rc, msg = _call(core, ws_bytes=need - 1)
    assert rc == ERR_WORKSPACE and str(need) in msg


def test_binding_host_checks(lm):
    """What the binding refuses before it touches the device -- on CPU tensors: the last check of all is the device's."""
    import ctc_crf
    N, T, V = 2, 6, 8
    x, lx = torch.zeros(N, T, V), torch.tensor([6, 4], dtype=torch.int32)
    fn = lambda **kw: ctc_crf.ctc_beam_search(x, lx, **kw)
    with pytest.raises(RuntimeError, match="GPU"):                                     # all arguments fine: only the device is missing
        fn(lm=lm, alpha=0.5, beta=-1.0, return_lm_scores=True)
    with pytest.raises(RuntimeError, match=r"lm must be an NgramLM.*got str: 'lm.arpa'"):
        fn(lm="lm.arpa", alpha=0.5)
    with pytest.raises(RuntimeError, match=r"the LM is over 8 classes, the activations have V=5"):
        ctc_crf.ctc_beam_search(torch.zeros(N, T, 5), lx, lm=lm)
    for kw in (dict(alpha=float("nan")), dict(alpha=float("inf")), dict(beta=float("-inf")), dict(beta="1")):
        with pytest.raises(RuntimeError, match=r"(alpha|beta) must be a finite number, got"):
            fn(lm=lm, **kw)
    with pytest.raises(RuntimeError, match=r"without lm they must be 0, got alpha=0.5, beta=0"):
        fn(alpha=0.5)
    with pytest.raises(RuntimeError, match=r"without lm they must be 0, got alpha=0.0, beta=2"):
        fn(beta=2)
    with pytest.raises(RuntimeError, match=r"return_lm_scores needs lm"):
        fn(return_lm_scores=True)
    with pytest.raises(RuntimeError, match=r"beam_size must lie in \[1, 64\], got 65"):  # the LM-free checks come first
        fn(lm=lm, beam_size=65)


def test_reference_against_brute_force_and_the_lm_free_reference():
    """V = 3, T <= 5, W = 64, C = 2: the fused reference search returns every label sequence with brute force + alpha * textbook LM +
    beta * len, in non-increasing order, and replay accepts its trace; at alpha = beta = 0 its trace is beam_ref.search's."""
    ng = ngram_ref.random_model(2, 3, 3)
    ref = ngram_ref.Ref(ng, 3)
    for T in range(0, 6):
        x = beam_ref.make_inputs(200 + T, 1, max(T, 1), 3)[0]
        for blank in range(3):
            want = {k: v for k, v in beam_ref.brute(x, T, blank).items() if v > -np.inf}
            got = beam_lm_ref.search(x, T, 64, 64, 2, blank, ref, 1.5, -1.0)
            assert {k for k, _, _ in got["nbest"]} == set(want)
            for k, v, l in got["nbest"]:
                assert abs(l - (1.5 * ref.score(k) - len(k))) < 1e-12 and abs(v - (want[k] + l)) <= 1e-12
            assert all(a[1] >= b[1] for a, b in zip(got["nbest"], got["nbest"][1:]))
            rp = beam_lm_ref.replay(x, T, got["trace"], 64, 2, blank, ref, 1.5, -1.0)
            assert rp["why"] is None and rp["excess"] == 0 and [p for p in rp["prefixes"] if p is not None] == [k for k, _, _ in got["nbest"]]
            zero = beam_lm_ref.search(x, T, 64, 64, 2, blank, ref, 0.0, 0.0)
            assert np.array_equal(zero["trace"], beam_ref.search(x, T, 64, 64, 2, blank)["trace"])
    # a trace that leaves out the LM's favourite is caught: follow the LM-free trace under a strong LM
    x = beam_ref.make_inputs(7, 1, 12, 3)[0]
    plain = beam_ref.search(x, 12, 2, 2, 2, 0)
    assert beam_lm_ref.replay(x, 12, plain["trace"], 2, 2, 0, ref, 3.0, 0.0)["excess"] > 1e-3


def test_order_key_levels_and_audit_hand_worked():
    """Every level of beam_lm_ref.order_key on hand-made candidates that differ at that level alone, and audit_ties on one frame with
    probabilities (0.5, 0.25, 0.25) under a unigram model that gives both labels log10 p = -0.5: W = 2, alpha = 1, beta = 0 -- the stay of
    () at log 0.5, then () + 1 and () + 2 level at log 0.25 - 0.5 ln 10, two places of one parent on the cut, equal keys."""
    base = dict(score=-1.0, kind=1, parent=2, key=-0.5, place=3)
    want = [dict(base, score=-0.5, kind=1, parent=9, key=-9.0, place=9), dict(base, kind=0, parent=9, key=0.0, place=-1),
            dict(base, parent=1, key=-9.0, place=9), dict(base, key=-0.25, place=9), dict(base, place=2), base, dict(base, score=-1.5, kind=0, parent=0)]
    for perm in (want[::-1], want[3:] + want[:3]):
        assert sorted(perm, key=beam_lm_ref.order_key) == want
    for name, (level, key) in beam_lm_ref.LM_ALTERED_ORDERS.items():
        assert sorted(want, key=key) != want, name
    ng = {(0,): (-1.0, 0.0), (1,): (-0.5, 0.0), (2,): (-0.5, 0.0)}
    ref = ngram_ref.Ref(ng, 3)
    x = np.log([[0.5, 0.25, 0.25]])
    a = beam_lm_ref.audit_ties(x, 1, 2, 2, 0, ref, 1.0, 0.0)
    l = 0.5 * ngram_ref.LN10
    assert a == dict(gap=(np.log(0.5) - (np.log(0.25) - l)) / (abs(np.log(0.25)) + l), stay_ext=0, slot=0, place=1, cut=1, key_level=0, reordered=0)
    # label 2 dearer to the LM than label 1: it goes first from place 1 -- a head that is not the next place of E_t
    ref = ngram_ref.Ref({**ng, (2,): (-0.25, 0.0)}, 3)
    a = beam_lm_ref.audit_ties(x, 1, 2, 2, 0, ref, 1.0, 0.0)
    r = beam_lm_ref.search(x, 1, 2, 2, 2, 0, ref, 1.0, 0.0)
    assert (a["place"], a["reordered"]) == (0, 1) and r["trace"].tolist() == [[0, 0 + 64 * 3]]


@pytest.fixture(scope="module")
def lm_tie_runs():
    """Per LM_TIE_CASES entry: (x, ref, audit, search at lx = T) -- once."""
    out = []
    for case in beam_lm_ref.LM_TIE_CASES:
        seed, V, W, C, T, blank, G, order, alpha, beta, zero_group = case
        x, ng = beam_lm_ref.lm_tie_inputs(case)
        ref = ngram_ref.Ref(ng, V)
        out.append((x, ng, ref, beam_lm_ref.audit_ties(x, T, W, C, blank, ref, alpha, beta), beam_lm_ref.search(x, T, W, W, C, blank, ref, alpha, beta)))
    return out


def test_symmetric_model_depends_on_the_groups_only(lm_tie_runs):
    """ngram_ref.symmetric_model as LM_TIE_CASES take it: over the class-to-group map of grouped_inputs (classes of one group share
    every frame's value), prefix-closed, of the case's order, one (log10 p, log10 bow) per group n-gram, log10 p = 0.0 behind the zero
    group and nowhere else; the textbook's log P of two sequences that differ inside the groups is the same fp64 number, and so is the
    compiled tables' fp32 look-up in every state."""
    import ctc_crf
    for case, (x, ng, ref, _, _) in zip(beam_lm_ref.LM_TIE_CASES, lm_tie_runs):
        seed, V, W, C, T, blank, G, order, alpha, beta, zero_group = case
        group = beam_ref.class_groups(seed, V, G)
        raw = beam_ref.grouped_inputs(seed, T, V, blank, G)
        assert np.array_equal(x.view(np.int32), beam_ref.through(x, "bf16").view(np.int32)) and np.abs(x - raw).max() <= 2.0 ** -8 * 3.3
        assert sorted(np.bincount(group, minlength=G)) == sorted(np.bincount(np.arange(V) % G, minlength=G))
        for t in range(0, T, 2):                                   # (in the other frames the blank has a value of its own)
            assert all(len({x[t, c] for c in range(V) if group[c] == g}) == 1 for g in range(G)), (case, t)
        gof = lambda k: tuple(w if isinstance(w, str) else int(group[w]) for w in k)
        by = {}
        for k, v in ng.items():
            assert len(k) == 1 or k[:-1] in ng, (case, k)
            assert (v[0] == 0.0) == (zero_group is not None and gof(k)[-1] == zero_group), (case, k, v)
            assert by.setdefault(gof(k), v) == v, (case, k)
        assert max(len(k) for k in ng) == order and len(ng) == sum(int(np.prod([1 if g == ngram_ref.BOS else (group == g).sum() for g in gk])) for gk in by)
        rng = np.random.default_rng(seed)
        members = [np.flatnonzero(group == g) for g in range(G)]
        lm = ctc_crf.NgramLM.from_ngrams(ng, V) if V <= 9 else None
        for _ in range(20):
            gs = rng.integers(0, G, size=int(rng.integers(1, 7)))
            a, b = (tuple(int(rng.choice(members[g])) for g in gs) for _ in range(2))
            assert ref.score(a) == ref.score(b), (case, a, b)
            if lm is not None:
                sa, sb = lm.start, lm.start
                for ca, cb in zip(a, b):
                    (la, sa), (lb, sb) = lm.lookup(sa, ca), lm.lookup(sb, cb)
                    assert la == lb and gof(lm.state_history[sa]) == gof(lm.state_history[sb]), (case, a, b)


def test_lm_tie_cases_meet_their_conditions(lm_tie_runs):
    """LM_TIE_CASES as the GPU test needs them (the conditions are listed above the list in tests/beam_lm_ref.py): the shapes are those
    of beam_ref.TIE_CASES with W = C = 64 among them, live and zero-group cases both; per case the smallest gap that is no tie >= 1e-3,
    no pair decided by unequal keys, one trace in both arithmetics, an LM that changes the trace and moves heads off the place order,
    ties at every level the case claims, one on the cut, and a changed trace under every altered order of a level it claims.  (The
    search is causal: the rows of lx = T - 1 and 1, which the GPU test also takes, are the first rows of lx = T's.)"""
    cases = beam_lm_ref.LM_TIE_CASES
    assert 5 <= len(cases) <= 7 and {c[1:7] for c in cases} <= {c[1:] for c in beam_ref.TIE_CASES}
    zero = [c for c in cases if c[10] is not None]
    assert len(zero) >= 2 and len(cases) - len(zero) >= 2 and any(c[1:4] == (70, 64, 64) for c in zero) and any(c[1:4] == (70, 64, 64) and c[10] is None for c in cases)
    for case, (x, ng, ref, a, r) in zip(cases, lm_tie_runs):
        seed, V, W, C, T, blank, G, order, alpha, beta, zero_group = case
        assert (alpha, beta) == ((0.5, 1.0) if zero_group is None else (1.5, 0.0)) and order == (2 if V == 70 else 3) and T <= 12
        print(case, {k: float(v) for k, v in a.items()})
        assert a["gap"] >= 1e-3, (case, a)
        assert a["key_level"] == 0 and a["reordered"] > 0, (case, a)
        levels = ["slot", "place"] + (["stay_ext"] if zero_group is not None else [])
        assert all(a[k] > 0 for k in levels + ["cut"]), (case, a)
        assert zero_group is not None or a["stay_ext"] == 0, (case, a)
        assert r["gap"] == 0.0                                       # (the search's own figure counts the ties: check_equals_search cannot take it)
        r32 = beam_lm_ref.search(x, T, W, W, C, blank, ref, alpha, beta, lse=beam_ref.lse32)
        assert np.array_equal(r["trace"], r32["trace"]) and [p for p, _, _ in r["nbest"]] == [p for p, _, _ in r32["nbest"]], case
        assert np.allclose([s for _, s, _ in r["nbest"]], [s for _, s, _ in r32["nbest"]], rtol=1e-6, atol=0)
        assert beam_lm_ref.replay(x, T, r["trace"], W, C, blank, ref, alpha, beta)["excess"] == 0
        assert not np.array_equal(r["trace"], beam_ref.search(x, T, W, W, C, blank)["trace"]), case
        for name, (level, key) in beam_lm_ref.LM_ALTERED_ORDERS.items():
            if level not in levels:
                continue
            bad = beam_lm_ref.search(x, T, W, W, C, blank, ref, alpha, beta, key=key)
            assert not np.array_equal(bad["trace"], r["trace"]), (case, name)
            if V <= 9:
                assert beam_lm_ref.replay(x, T, bad["trace"], W, C, blank, ref, alpha, beta)["excess"] == 0     # (replay cannot tell)


def test_planted_cases_are_well_separated():
    """The inputs of the GPU tests that demand EQUALITY with the reference search: adjacent candidates among the ranks 0 .. W differ by at
    least 1e-5 relative -- a hundred times what fp32 rounding of lmw and of the sums can move them -- and the cases reach what they are for."""
    import ctc_crf
    assert beam_lm_ref.back_off_case.__defaults__ == (False, 5)
    for order, closed in ((5, False), (5, True), (8, False), (8, True)):
        ng, x, (V, W, C, T, blank, alpha, beta) = beam_lm_ref.back_off_case(closed, order)
        lm, ref = ctc_crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
        r = beam_lm_ref.search(x[0], T, W, W, C, blank, ref, alpha, beta)
        assert r["gap"] >= 1e-5 and tuple(range(order)) in beam_ref.spell(r["trace"], T, W)
        assert V == order + 2 >= 7 and lm.order == order and lm.num_arcs == ((order - 1) * (order - 2) // 2 + 1 if closed else order - 1)
        s, depth = lm.state_history.index(tuple(range(order - 1))), 0       # (order 8: the state of seven tokens, the longest there is)
        while s:
            s, depth = int(lm.bo_state[s]), depth + 1
        assert depth == (order - 1 if closed else 2)
        if closed:                                                  # every class but the chain's last walks order - 1 sparse rows and misses
            for c in range(V):
                s, rows = lm.state_history.index(tuple(range(order - 1))), 0
                while s and c not in lm.arc_label[lm.row_off[s]:lm.row_off[s + 1]]:
                    s, rows = int(lm.bo_state[s]), rows + 1
                assert rows == (0 if c == order - 1 else order - 1), (order, c, rows)
    ng, rows, x, (V, W, C, T, blank, alpha, beta) = beam_lm_ref.row_edges_case()
    lm, ref = ctc_crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
    assert V == 8192 and lm.order == 2 and sorted(len(v) for v in rows.values()) == [0, 1, 2, 3, 63, 64, 65, 8191]
    r = beam_lm_ref.search(x[0], T, W, W, C, blank, ref, alpha, beta)
    assert r["gap"] >= 1e-5
    E = set(beam_ref.top_classes(x[0, 1].astype(np.float64), blank, C))
    for ctx, labels in rows.items():
        if labels:
            assert labels[0] in E and (labels[-1] in E or labels[-1] == blank) and (E - set(labels)), ctx
    found = {p for p in beam_ref.spell(r["trace"], T, W) if p and len(p) == 2 and p[1] in rows.get(p[0], ())}
    assert len({p[0] for p in found}) >= 4
