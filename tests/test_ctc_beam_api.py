"""CPU tests (no GPU) of ctc_beam_search: the NumPy yardstick itself (tests/beam_ref.py: against brute force over all V^T labellings, a
hand-worked case, the event counters of the GPU tests' seeded inputs, `replay` on its own trace and on a negative control, the planted
rows and the exact-tie cases of the GPU tests with the conditions they must meet and the altered orders they must tell apart), the host
checks of the Python binding (cat_amd/ctc_crf/_C.py ctc_beam_search) and the C ABI's answers before any HIP call (include/ctc_crf_hip.h
crf_ctc_beam_workspace_bytes, crf_ctc_beam)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import beam_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_beam_workspace_bytes", "crf_ctc_beam", "crf_last_beam_kernel")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_reference_against_brute_force():
    """V = 3, T <= 6, every blank, a beam that holds every prefix (at most 41 at T = 6), C = V - 1: the search is exact -- every label
    sequence of finite mass is returned, with the sum over its paths to 1e-12."""
    for T in range(0, 7):
        x = beam_ref.make_inputs(100 + T, 1, max(T, 1), 3)[0]
        for blank in range(3):
            want = {k: v for k, v in beam_ref.brute(x, T, blank).items() if v > -np.inf}
            assert len(want) <= 41
            got = beam_ref.search(x, T, 64, 64, 2, blank)["nbest"]
            assert len(got) == len(want) and {k for k, _ in got} == set(want), (T, blank)
            for k, v in got:
                assert abs(v - want[k]) <= 1e-12, (T, blank, k, v, want[k])
            assert all(a[1] >= b[1] for a, b in zip(got, got[1:]))
    # raw rows with normalize: the scores of log_softmax
    x = (3.0 * np.random.default_rng(5).standard_normal((5, 3))).astype(np.float32)
    want = beam_ref.brute(x, 5, 1, normalize=True)
    for k, v in beam_ref.search(x, 5, 64, 64, 2, 1, normalize=True)["nbest"]:
        assert abs(v - want[k]) <= 1e-12


def test_hand_worked_case():
    """Two frames over (blank, a, b), probabilities (0.5, 0.3, 0.2) and (0.4, 0.5, 0.1), W = 2, C = 2.
    Frame 0: () 0.5, (a) 0.3, (b) 0.2 -> beam [(), (a)].
    Frame 1: stay ()  = 0.5 * 0.4 = 0.20;  stay (a) = pb' 0.3 * 0.4 + pnb' [0.3 * 0.5 repeat + 0.5 * 0.5 merged from ()] = 0.52;
             () + b = 0.5 * 0.1 = 0.05;  (a) + b = 0.03;  (a) + a = 0.5 * pb(a) = 0 -- dropped.  -> beam [(a) 0.52, () 0.20]."""
    x = np.log(np.array([[0.5, 0.3, 0.2], [0.4, 0.5, 0.1]]))
    r = beam_ref.search(x, 2, 2, 2, 2, 0)
    assert [k for k, _ in r["nbest"]] == [(1,), ()]
    assert np.allclose([v for _, v in r["nbest"]], np.log([0.52, 0.20]), rtol=0, atol=1e-14)
    assert r["trace"].tolist() == [[0, 0 + 64 * 2], [1, 0]] and r["merged"] == 1 and r["reentered"] == 0
    assert beam_ref.spell(r["trace"], 2, 2) == [(1,), ()]
    # without the merge (a) would carry 0.27 only and the extension would take a slot of its own
    bad = beam_ref.search(x, 2, 2, 2, 2, 0, merge=False)
    assert [k for k, _ in bad["nbest"]] == [(1,), (1,)]
    # W = 1, top_classes = 1 (class a alone at both frames): () 0.5, then () + a = 0.5 * 0.5 = 0.25 beats the stay 0.5 * 0.4 = 0.20
    r = beam_ref.search(x, 2, 1, 1, 1, 0)
    assert r["nbest"][0][0] == (1,) and abs(r["nbest"][0][1] - np.log(0.25)) < 1e-14 and r["trace"].tolist() == [[0], [64 * 2]]
    # lx = 0: the empty prefix at score 0, no trace
    r = beam_ref.search(x, 0, 2, 2, 2, 0)
    assert r["nbest"] == [((), 0.0)] and (r["trace"] == -1).all()


@pytest.fixture(scope="module")
def case_runs():
    """search on every seeded case of the GPU replay test, once."""
    out = []
    for seed, V, W, C, T, lxs, blank in beam_ref.REPLAY_CASES:
        x = beam_ref.make_inputs(seed, len(lxs), T, V)
        out.append([(x[b], lx, beam_ref.search(x[b], lx, W, W, C, blank)) for b, lx in enumerate(lxs)])
    return out


def test_seeded_cases_raise_both_events(case_runs):
    """Every seeded input of the GPU replay test in which two prefixes can meet at all (W >= 2, more than one frame) merges an extension
    into a beam prefix, and the narrow-beam cases over two labels (V = 3, W = 2 .. 4, T = 30: the drop-and-re-enter path) and the
    list as a whole also see a parent that re-entered merge into a child that had stayed."""
    tot = 0
    for case, runs in zip(beam_ref.REPLAY_CASES, case_runs):
        seed, V, W, C, T, lxs, blank = case
        merged, reentered = sum(r["merged"] for _, _, r in runs), sum(r["reentered"] for _, _, r in runs)
        tot += reentered
        if W >= 2 and T > 1:
            assert merged >= 1, (case, merged)
        if V == 3:
            assert W in (2, 3, 4) and T == 30 and merged >= 1 and reentered >= 1, (case, merged, reentered)
    assert tot >= 3


def test_replay_accepts_its_own_trace_and_sees_a_missing_merge(case_runs):
    """replay reports 0 on beam_ref's own trace, with the same prefixes and scores; on the trace of the same search with the merge left
    out (the negative control) it reports a violation wherever that search differed at all, and it does differ in the merging cases."""
    seen = 0
    for case, runs in zip(beam_ref.REPLAY_CASES, case_runs):
        seed, V, W, C, T, lxs, blank = case
        for x, lx, r in runs:
            rp = beam_ref.replay(x, lx, r["trace"], W, C, blank)
            assert rp["excess"] == 0 and rp["why"] is None, (case, lx, rp["why"])
            got = [(p, s) for p, s in zip(rp["prefixes"], rp["scores"]) if p is not None]
            assert [p for p, _ in got] == [p for p, _ in r["nbest"]] == [p for p in beam_ref.spell(r["trace"], max(0, min(lx, T)), W) if p is not None]
            assert np.array_equal([s for _, s in got], [s for _, s in r["nbest"]])
            if V <= 5 and r["merged"]:
                bad = beam_ref.search(x, lx, W, W, C, blank, merge=False)
                rb = beam_ref.replay(x, lx, bad["trace"], W, C, blank)
                if not np.array_equal(bad["trace"], r["trace"]):
                    assert rb["excess"] == np.inf and rb["why"], (case, lx)
                    seen += 1
    assert seen >= 4
    # a trace that picks a worse candidate: the excess is the relative gap
    x = np.log(np.array([[0.5, 0.3, 0.2], [0.4, 0.5, 0.1]]))
    tr = np.array([[0, 0 + 64 * 3], [0, 1]], dtype=np.int32)                       # frame 0 keeps (b) 0.2 instead of (a) 0.3
    rp = beam_ref.replay(x, 1, tr, 2, 2, 0)
    assert abs(rp["excess"] - (np.log(0.3) - np.log(0.2)) / abs(np.log(0.2))) < 1e-12 and rp["prefixes"] == [(), (2,)]
    assert beam_ref.replay(x, 2, tr, 2, 2, 0)["excess"] > rp["excess"]              # (frame 1: () + a at 0.25 beats the stay of (b) at 0.15)
    tr = np.array([[0, -1], [0, -1]], dtype=np.int32)                               # a slot left empty beside finite candidates
    assert beam_ref.replay(x, 2, tr, 2, 2, 0)["excess"] == np.inf


def test_lse32_is_the_kernels_sum():
    """fp64 maximum and result, fp32 exp / log of the difference: within fp32 rounding of `lse`, exact where a term is -inf, symmetric."""
    rng = np.random.default_rng(3)
    for a, b in rng.uniform(-40, 0, (200, 2)):
        got = beam_ref.lse32(a, b)
        assert abs(got - beam_ref.lse(a, b)) <= 3e-7 and got == beam_ref.lse32(b, a)
    NEG = -np.inf
    assert beam_ref.lse32(NEG, NEG) == NEG and beam_ref.lse32(-3.25, NEG) == -3.25 and beam_ref.lse32(NEG, 0.0) == 0.0
    assert beam_ref.lse32(-2.0, -2.0) == -2.0 + float(np.log(np.float32(2)))
    assert beam_ref.lse32(0.0, -200.0) == 0.0                                       # (fp32 exp underflows: the small term is lost)


def test_through_rounds_to_the_dtype():
    a = np.array([1.0, -0.0, 1 + 2 ** -8, 1 + 3 * 2 ** -8, 1 + 2 ** -11, -np.inf, 3.14159, -8.7654], dtype=np.float32)
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
        want = torch.tensor(a).to(dt).float().numpy()
        assert np.array_equal(beam_ref.through(a, name).view(np.int32), want.view(np.int32)), name


@pytest.mark.parametrize("V", [64, 129, 4096, 4097, 8191, 8192])
def test_planted_rows_have_their_properties(V):
    """planted_rows, read with the reference's own top_classes: (a) a row whose E_t lies in ONE column, (b) equal values at v and v + 64
    and, beyond 4096 classes, at v and v + 4096, next to each other in E_t and the lower index first, (c) E_t on both sides of 4096, (d) the
    value at place C also outside E_t, at a higher index, (e) a row with fewer than C classes above -inf, (f) a row with -0.0 and +0.0 on
    top, in index order, (g) the blank far below in some rows and on top in another -- each wherever the shape leaves room for it: a
    column of V holds V / 64 classes, V = 4097 has one class beyond 4096 (none with the blank there), C >= V - 1 leaves no class out."""
    for dtype in ("fp32", "bf16", "fp16"):
        for C in (8, 64):
            for blank in (0, V - 1):
                Ce = min(C, V - 1)
                rows = dict(beam_ref.planted_rows(V, dtype, blank, C))
                assert list(rows) == ["column", "spread", "sparse", "zeros"] and set(beam_ref.PLANTED_LOGPROB_ONLY) == {"zeros"}
                what = (V, dtype, C, blank)
                for name, row in rows.items():
                    assert row.dtype == np.float32 and row.shape == (V,) and not np.isnan(row).any() and row.max() <= 0, (what, name)
                    assert np.array_equal(beam_ref.through(row, dtype).view(np.int32), row.view(np.int32)), (what, name)
                E = {name: beam_ref.top_classes(row, blank, Ce) for name, row in rows.items()}
                pairs = lambda name, step: [(a, b) for a, b in zip(E[name], E[name][1:]) if b == a + step and rows[name][a] == rows[name][b]]
                # (a), (b), (c): the column row
                room = len([v for v in range(E["column"][0] & 63, V, 64) if v != blank])
                if room >= Ce:
                    assert len({v & 63 for v in E["column"]}) == 1, what
                if room >= 3:
                    assert pairs("column", 64), what
                if V >= 8191:
                    assert min(len(pairs("column", 4096)), len(pairs("column", 64))) >= (1 if C == 8 else 8), what
                    assert min(E["column"]) < 4096 <= max(E["column"]), what
                # (c), (d), (g): the spread row
                if max(v for v in range(V) if v != blank) >= 4096:
                    assert min(E["spread"]) < 4096 <= max(E["spread"]), what
                    assert V == 4097 or sum(v >= 4096 for v in E["spread"]) >= Ce // 4, what
                if Ce < V - 1:
                    for name in ("spread",) + (("column",) if room >= Ce + 1 else ()):
                        full = beam_ref.top_classes(rows[name], blank, V - 1)
                        assert rows[name][full[Ce]] == rows[name][full[Ce - 1]] and full[Ce] > full[Ce - 1], (what, name)
                assert rows["spread"][blank] > np.delete(rows["spread"], blank).max(), what
                for name in ("column", "sparse", "zeros"):
                    finite = np.delete(rows[name], blank)
                    assert rows[name][blank] == -30 and rows[name][blank] < finite[np.isfinite(finite)].min() - 20, (what, name)
                # (e)
                finite = np.isfinite(np.delete(rows["sparse"], blank)).sum()
                assert 1 <= finite < Ce and np.isneginf(rows["sparse"]).sum() == V - 1 - finite, what
                assert np.isfinite(rows["sparse"][E["sparse"][:finite]]).all() and (V < 129 or pairs("sparse", 64)), what
                # (f)
                zeros = [v for v in range(V) if rows["zeros"][v] == 0]
                assert len(zeros) == (4 if V >= 8191 else 3) and E["zeros"][:len(zeros)] == zeros, what
                sign = [bool(np.signbit(rows["zeros"][v])) for v in zeros]
                assert sign == [True, False, True, False][:len(zeros)] and (zeros[0] + 64 in zeros or V == 64), what
                assert len({v & 63 for v in zeros}) >= 2 and (V < 8191 or zeros[0] + 4096 in zeros), what


def test_grouped_inputs_share_one_value_per_group():
    for seed, V, W, C, T, blank, groups in beam_ref.TIE_CASES:
        x = beam_ref.grouped_inputs(seed, T, V, blank, groups)
        assert x.dtype == np.float32 and x.shape == (T, V) and x.max() <= -0.3 + 1e-6 and x.min() >= -3.3 - 1e-6
        assert np.array_equal(x, beam_ref.grouped_inputs(seed, T, V, blank, groups))
        part = {}
        for v in range(V):
            if v != blank:
                part.setdefault(tuple(x[:, v]), []).append(v)
        assert len(part) <= groups and sum(len(p) for p in part.values()) == V - 1
        for t in range(T):
            shared = any(x[t, blank] == x[t, v] for v in range(V) if v != blank)
            assert shared == (t % 2 == 0), (seed, V, t)
            assert len(set(x[t])) == min(groups, V) + (t % 2), (seed, V, t)


def test_audit_ties_hand_worked():
    """One frame, probabilities (0.5, 0.25, 0.25), W = 2, C = 2: the stay of () at 0.5, then () + 1 and () + 2 level at 0.25 -- two places
    of one parent, ranks W - 1 and W; the one pair that is not level differs by log 2 / |log 0.25| = 0.5.  With the blank at 0.25 too the
    stay is level with both extensions: one more pair, a stay beside an extension."""
    a = beam_ref.audit_ties(np.log([[0.5, 0.25, 0.25]]), 1, 2, 2, 0)
    assert a == dict(gap=0.5, stay_ext=0, slot=0, place=1, cut=1)
    a = beam_ref.audit_ties(np.log([[0.25, 0.25, 0.25]]), 1, 2, 2, 0)
    assert a == dict(gap=np.inf, stay_ext=1, slot=0, place=1, cut=1)
    # two frames, W = 3.  Frame 0 as above (its level pair is ranks 1 and 2: not on the cut).  Frame 1, (0.25, 0.5, 0.5): the stays of (1)
    # and (2) level at 0.4375 (two slots), then the stay of () at 0.25 * 0.5 level with (1) + 2 at 0.5 * 0.25 -- the same two addends in
    # the log domain -- a stay beside an extension, ranks W - 1 and W
    x = np.log([[0.5, 0.25, 0.25], [0.25, 0.5, 0.5]])
    a = beam_ref.audit_ties(x, 2, 3, 2, 0)
    r = beam_ref.search(x, 2, 3, 3, 2, 0)
    assert [p for p, _ in r["nbest"]] == [(1,), (2,), ()] and np.allclose(np.exp([s for _, s in r["nbest"]]), [0.4375, 0.4375, 0.125])
    assert (a["slot"], a["place"], a["stay_ext"], a["cut"]) == (1, 1, 1, 1) and a["gap"] == 0.5


# the total order with one rule altered: what a kernel that mis-writes that rule would compute
def _own_label(c):
    return c["kind"] == 1 and len(c["prefix"]) >= 2 and c["prefix"][-2] == c["cls"]


ALTERED_ORDERS = {
    "an extension of a lower slot before a stay": lambda c: (-c["score"], c["parent"], c["kind"], c["place"]),
    "the highest slot first": lambda c: (-c["score"], c["kind"], -c["parent"], c["place"]),
    "the extension by the own last label first": lambda c: (-c["score"], c["kind"], c["parent"], -1 if _own_label(c) else c["place"]),
    "the extension by the own last label last": lambda c: (-c["score"], c["kind"], c["parent"], 99 if _own_label(c) else c["place"]),
    "places descending": lambda c: (-c["score"], c["kind"], c["parent"], -c["place"]),
}


def test_tie_cases_meet_their_conditions():
    """TIE_CASES as the GPU test needs them: W in {2, 4, 8, 16, 64}, W = C = 64 at V = 70, blanks first, last and between, T <= 12; every
    count of audit_ties >= 1, the one on the cut included; the smallest gap that is no tie >= 1e-3 relative (10 x the rtol of a kernel
    score); one trace in both arithmetics at every lx the GPU test takes; and every altered order changes the trace of some case."""
    cases = beam_ref.TIE_CASES
    assert len(cases) >= 5 and {c[2] for c in cases} >= {2, 4, 8, 16, 64} and any(c[1:4] == (70, 64, 64) for c in cases)
    assert any(c[5] == 0 for c in cases) and any(c[5] == c[1] - 1 for c in cases) and any(0 < c[5] < c[1] - 1 for c in cases)
    bites = {name: 0 for name in ALTERED_ORDERS}
    for case in cases:
        seed, V, W, C, T, blank, groups = case
        assert T <= 12 and groups >= 2
        x = beam_ref.grouped_inputs(seed, T, V, blank, groups)
        a = beam_ref.audit_ties(x, T, W, C, blank)
        print(case, a)
        assert min(a["stay_ext"], a["slot"], a["place"], a["cut"]) >= 1, (case, a)
        assert a["gap"] >= 1e-3, (case, a)
        for lx in (T, T - 1, 1):
            r = beam_ref.search(x, lx, W, W, C, blank)
            r32 = beam_ref.search(x, lx, W, W, C, blank, lse=beam_ref.lse32)
            assert np.array_equal(r["trace"], r32["trace"]) and [p for p, _ in r["nbest"]] == [p for p, _ in r32["nbest"]], (case, lx)
            assert np.allclose([s for _, s in r["nbest"]], [s for _, s in r32["nbest"]], rtol=1e-6, atol=0)
            assert beam_ref.replay(x, lx, r["trace"], W, C, blank)["excess"] == 0
            for name, key in ALTERED_ORDERS.items():
                bad = beam_ref.search(x, lx, W, W, C, blank, key=key)
                if not np.array_equal(bad["trace"], r["trace"]):
                    bites[name] += 1
                    assert beam_ref.replay(x, lx, bad["trace"], W, C, blank)["excess"] == 0     # (replay cannot tell: only equality can)
    print(bites)
    assert all(n >= 2 for n in bites.values()), bites


def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    assert callable(ctc_crf.ctc_beam_search) and ctc_crf.ctc_beam_search is cat_amd.ctc_crf.ctc_beam_search
    assert callable(core.ctc_beam_search) and callable(core.last_beam_kernel)
    assert "CTCBeamDecoder" in ctc_crf.ctc_beam_search.__doc__ and "KenLM" in ctc_crf.ctc_beam_search.__doc__


def test_workspace_bytes(core):
    """At least the three sections, a multiple of 256, monotone in every argument; the ranges."""
    ws = core._lib.crf_ctc_beam_workspace_bytes
    for B in (1, 3, 16):
        for T in (1, 63, 64, 1500):
            for V in (1, 2, 41, 72, 5000, 8192):
                for W in (1, 16, 63):
                    for C in (1, 40, 63):
                        w = ws(B, T, V, W, C)
                        rs = min(C, V - 1) + 1
                        assert w >= 4 * B * T * (2 * rs + W) and w % 256 == 0, (B, T, V, W, C, w)
                        assert ws(B + 1, T, V, W, C) >= w and ws(B, T + 1, V, W, C) >= w
                        assert ws(B, T, V, W + 1, C) >= w and ws(B, T, V, W, C + 1) >= w
                        assert V == 8192 or ws(B, T, V + 1, W, C) >= w
    assert ws(16, 1500, 72, 16, 40) == 4 * 16 * 1500 * (41 + 41 + 16)                 # (every section a multiple of 256 as it is)
    for bad in ((0, 10, 8, 4, 4), (2, 0, 8, 4, 4), (2, 10, 0, 4, 4), (-1, 10, 8, 4, 4), (2, 10, 8, 0, 4), (2, 10, 8, 65, 4), (2, 10, 8, 4, 0),
                (2, 10, 8, 4, 65), (2, 10, 8, -3, 4)):
        assert ws(*bad) == -1 and core._lib.crf_last_error(), bad
    assert ws(1 << 20, 1 << 12, 72, 4, 4) == -1 and b"B * T > INT32_MAX" in core._lib.crf_last_error()
    assert ws(2, 10, 8193, 4, 4) == -1 and b"8192" in core._lib.crf_last_error()


PTRS = dict(act=0x1000, lx=0x2000, hyps=0x3000, len=0x4000, score=0x5000, trace=0x6000, ws=0x7000)


def _call(core, ptrs=None, dtype=0, time_major=0, blank=0, normalize=0, B=2, T=10, V=8, W=4, nbest=2, C=5, ws_bytes=None):
    """crf_ctc_beam with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_beam_workspace_bytes(B, T, V, W, C))
    rc = core._lib.crf_ctc_beam(vp(p["act"]), dtype, time_major, blank, normalize, vp(p["lx"]), B, T, V, W, nbest, C, vp(p["hyps"]),
                                vp(p["len"]), vp(p["score"]), vp(p["trace"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_argument_errors_without_gpu(core):
    for name in ("act", "lx", "hyps", "len", "score", "ws"):
        rc, msg = _call(core, {name: 0})
        assert rc == ERR_ARG and "null" in msg, (name, rc, msg)
    for dtype in (-1, 3, 17):
        rc, msg = _call(core, dtype=dtype)
        assert rc == ERR_ARG and "dtype" in msg, (dtype, rc, msg)
    for normalize in (-1, 2):
        rc, msg = _call(core, normalize=normalize)
        assert rc == ERR_ARG and "normalize" in msg and str(normalize) in msg, (normalize, rc, msg)
    for blank in (-1, 8, 100):
        rc, msg = _call(core, blank=blank)
        assert rc == ERR_ARG and "blank" in msg and str(blank) in msg, (blank, rc, msg)
    for kw in (dict(B=0), dict(B=-3), dict(T=0), dict(T=-1), dict(V=0)):
        rc, msg = _call(core, ws_bytes=1 << 20, **kw)
        assert rc == ERR_ARG and msg, (kw, rc, msg)
    for W in (0, -1, 65, 1000):
        rc, msg = _call(core, W=W, nbest=1, ws_bytes=1 << 20)
        assert rc == ERR_ARG and "beam width" in msg and str(W) in msg, (W, rc, msg)
    for C in (0, -1, 65):
        rc, msg = _call(core, C=C, ws_bytes=1 << 20)
        assert rc == ERR_ARG and "top_classes" in msg and str(C) in msg, (C, rc, msg)
    for nbest in (0, -1, 5, 64):
        rc, msg = _call(core, nbest=nbest)
        assert rc == ERR_ARG and "nbest" in msg and str(nbest) in msg, (nbest, rc, msg)
    rc, msg = _call(core, B=1 << 20, T=1 << 12, ws_bytes=1 << 50)
    assert rc == ERR_ARG and "B * T > INT32_MAX" in msg, (rc, msg)
    rc, msg = _call(core, V=8193, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "8192" in msg, (rc, msg)
    need = core._lib.crf_ctc_beam_workspace_bytes(2, 10, 8, 4, 5)
    assert need >= 4 * 2 * 10 * (6 + 6 + 4)
    for short in (0, 1, need - 1):
        rc, msg = _call(core, ws_bytes=short)
        assert rc == ERR_WORKSPACE and str(need) in msg, (short, rc, msg)
    assert core.last_beam_kernel() in ("", "crf_beam_row_kernel<f32>", "crf_beam_row_kernel<bf16>", "crf_beam_row_kernel<f16>")


def _i32(*a):
    return torch.tensor(a, dtype=torch.int32)


def test_binding_host_checks():
    """What the binding refuses before it touches the device -- on CPU tensors: the last check of all is the device's."""
    import ctc_crf
    N, T, V = 2, 6, 5
    x, lx = torch.zeros(N, T, V), _i32(6, 4)
    fn = lambda **kw: ctc_crf.ctc_beam_search(kw.pop("x", x), kw.pop("lx", lx), **kw)
    with pytest.raises(RuntimeError, match="GPU"):                                     # CPU activations: there is no CPU path
        fn()
    with pytest.raises(RuntimeError, match="GPU"):
        fn(x=torch.zeros(T, N, V), time_major=True, beam_size=64, nbest=64, top_classes=64, fuse_log_softmax=True, return_trace=True)
    for dtype in (torch.float64, torch.int32):
        with pytest.raises(RuntimeError, match=r"float32, bfloat16 or float16.*" + str(dtype).replace(".", r"\.")):
            fn(x=torch.zeros(N, T, V, dtype=dtype))
    for blank in (-1, 5, 70):
        with pytest.raises(RuntimeError, match=rf"blank must lie in \[0, V-1=4\], got {blank}"):
            fn(blank=blank)
    for W in (0, -1, 65):
        with pytest.raises(RuntimeError, match=rf"beam_size must lie in \[1, 64\], got {W}"):
            fn(beam_size=W)
    for nbest in (0, 17):
        with pytest.raises(RuntimeError, match=rf"nbest must lie in \[1, beam_size=16\], got {nbest}"):
            fn(nbest=nbest)
    for C in (0, 65):
        with pytest.raises(RuntimeError, match=rf"top_classes must lie in \[1, 64\], got {C}"):
            fn(top_classes=C)
    with pytest.raises(RuntimeError, match=r"expect 2 input lengths, got 3"):
        fn(lx=_i32(6, 4, 4))
    with pytest.raises(RuntimeError, match=r"expect 6 input lengths, got 2"):          # time-major: N is the second dimension
        fn(time_major=True)
    with pytest.raises(RuntimeError, match=r"frame lengths must lie in \[0, T=6\], got max 7"):
        fn(lx=_i32(7, 4))
    with pytest.raises(RuntimeError, match=r"got 2 dimensions"):
        fn(x=torch.zeros(T, V))
