"""CPU tests (no GPU) of ctc_beam_search(lm=...): the exports, crf_ngram_tables_check on corrupted host tables, the argument errors of the
Python binding and of crf_ctc_beam_lm answered before any HIP call (include/ctc_crf_hip.h), the yardstick tests/beam_lm_ref.py against
brute force and against tests/beam_ref.py at zero weights, and the planted inputs of the GPU tests with the separation they must have."""
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


def test_planted_cases_are_well_separated():
    """The inputs of the GPU tests that demand EQUALITY with the reference search: adjacent candidates among the ranks 0 .. W differ by at
    least 1e-5 relative -- a hundred times what fp32 rounding of lmw and of the sums can move them -- and the cases reach what they are for."""
    import ctc_crf
    for closed in (False, True):
        ng, x, (V, W, C, T, blank, alpha, beta) = beam_lm_ref.back_off_case(closed)
        lm, ref = ctc_crf.NgramLM.from_ngrams(ng, V), ngram_ref.Ref(ng, V)
        r = beam_lm_ref.search(x[0], T, W, W, C, blank, ref, alpha, beta)
        assert r["gap"] >= 1e-5 and (0, 1, 2, 3, 4) in beam_ref.spell(r["trace"], T, W)
        assert lm.order == 5 and lm.num_arcs == (7 if closed else 4)
        s, depth = lm.state_history.index((0, 1, 2, 3)), 0
        while s:
            s, depth = int(lm.bo_state[s]), depth + 1
        assert depth == (4 if closed else 2)
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
