"""CPU tests (no GPU) of the streaming beam search: the exports and the surface, the size of a state record, the argument errors of the
Python call and of crf_ctc_beam_chunk answered before any device use (include/ctc_crf_hip.h; the C errors with fake pointers that are
never dereferenced), and the BeamState mismatches by name."""
import ctypes
import inspect

import pytest
import torch

from tests import ngram_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_beam_state_record_bytes", "crf_ctc_beam_chunk_workspace_bytes", "crf_ctc_beam_chunk")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


@pytest.fixture(scope="module")
def lm():
    import ctc_crf
    return ctc_crf.NgramLM.from_ngrams(ngram_ref.random_model(1, 8, 3), 8)


def test_symbols_exported_and_surface(core):
    import cat_amd.ctc_crf
    import ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = open(core.LIB_PATH.rsplit("/cat_amd/", 1)[0] + "/include/ctc_crf_hip.h").read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in core.EXPORTED_SYMBOLS and s + "(" in hdr, s
    assert ctc_crf.ctc_beam_search_chunk is cat_amd.ctc_crf.ctc_beam_search_chunk
    assert ctc_crf.BeamState is cat_amd.ctc_crf.BeamState is core.BeamState
    par = inspect.signature(ctc_crf.ctc_beam_search_chunk).parameters
    assert list(par) == ["log_probs", "input_lengths", "state", "reset", "beam_size", "nbest", "top_classes", "blank", "time_major",
                         "fuse_log_softmax", "lm", "alpha", "beta", "max_hyp_len", "return_trace", "return_lm_scores"]
    assert [par[k].default for k in list(par)[2:]] == [None, None, 16, 1, 40, 0, False, False, None, 0.0, 0.0, 512, False, False]
    doc = ctc_crf.ctc_beam_search_chunk.__doc__
    for word in ("chunk_infer", "decode.py", "for chunk", "max_hyp_len", "reset", "index_select", "Endpointing".lower(), "end-of-sentence",
                 "stable common prefix"):
        assert word in doc, word
    assert "ctc_beam_search_chunk" in cat_amd.ctc_crf.__doc__
    for word in ("record_bytes = (56 W + 4 W cap + 15) & ~15", "state_in_dev", "reset_dev", "endpointing"):
        assert word in hdr, word


def test_record_bytes(core):
    f = core._lib.crf_ctc_beam_state_record_bytes
    for W in (1, 2, 3, 16, 63, 64):
        for cap in (1, 2, 7, 8, 512, 8191, 8192):
            n = f(W, cap)
            assert n == (56 * W + 4 * W * cap + 15) // 16 * 16 and n % 16 == 0 and n >= 56 * W + 4 * W * cap
            if W < 64:
                assert f(W + 1, cap) > n
            if cap < 8192:
                assert f(W, cap + 1) >= n
            if cap + 4 <= 8192:
                assert f(W, cap + 4) > n
    for W, cap, word in ((0, 8, "beam width"), (65, 8, "beam width"), (4, 0, "cap"), (4, 8193, "cap"), (4, -1, "cap")):
        assert f(W, cap) == -1 and word in core._lib.crf_last_error().decode(), (W, cap)
    assert core._lib.crf_ctc_beam_chunk_workspace_bytes(3, 32, 72, 16, 40) == core._lib.crf_ctc_beam_workspace_bytes(3, 32, 72, 16, 40)
    assert core._lib.crf_ctc_beam_chunk_workspace_bytes(3, 0, 72, 16, 40) == -1


PTRS = dict(act=0x1000, lx=0x2000, hyps=0x3000, len=0x4000, score=0x5000, trace=0x6000, ws=0x7000, lm_score=0x8000, state_in=0x100000,
            state_out=0x200000, reset=0xa000)


def _call(core, ptrs=None, dtype=0, blank=0, normalize=0, B=2, T=10, V=8, W=4, nbest=2, C=5, cap=16, ws_bytes=None, alpha=0.5, beta=1.0, lm=True,
          **tab):
    """crf_ctc_beam_chunk with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    import cat_amd.ngram_lm as m
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    f = dict(S=5, A=7, V=8, order=3, start=1, **{n: 0x9000 + 0x100 * i for i, n in enumerate(m.TABLE_NAMES)})
    f.update(tab)
    st = m._Tables(*[f[n] for n in m.TABLE_NAMES], f["S"], f["A"], f["V"], f["order"], f["start"])
    if ws_bytes is None:
        ws_bytes = max(0, core._lib.crf_ctc_beam_chunk_workspace_bytes(B, T, V, W, C))
    rc = core._lib.crf_ctc_beam_chunk(vp(p["act"]), dtype, 0, blank, normalize, vp(p["lx"]), B, T, V, W, nbest, C, ctypes.byref(st) if lm else None,
                                      alpha, beta, vp(p["state_in"]), vp(p["reset"]), vp(p["state_out"]), cap, vp(p["hyps"]), vp(p["len"]),
                                      vp(p["score"]), vp(p["lm_score"]), vp(p["trace"]), vp(p["ws"]), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
def test_c_abi_argument_errors_without_gpu(core, with_lm):
    call = lambda *a, **kw: _call(core, *a, lm=with_lm, **kw)
    for name in ("act", "lx", "hyps", "len", "score", "ws", "state_out"):
        rc, msg = call({name: 0})
        assert rc == ERR_ARG and "crf_ctc_beam_chunk" in msg and "null" in msg, (name, rc, msg)
    for kw, word in ((dict(dtype=3), "dtype"), (dict(normalize=2), "normalize"), (dict(blank=8), "blank"), (dict(W=65, nbest=1, ws_bytes=1 << 20), "beam width"),
                     (dict(C=0, ws_bytes=1 << 20), "top_classes"), (dict(nbest=5), "nbest"), (dict(B=0, ws_bytes=1 << 20), "B/T/V"),
                     (dict(T=0, ws_bytes=1 << 20), "B/T/V"), (dict(cap=0), "cap 0"), (dict(cap=8193), "cap 8193"), (dict(cap=-4), "cap -4")):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)
    rc, msg = call(V=8193, ws_bytes=1 << 30)
    assert rc == ERR_UNSUPPORTED and "8192" in msg
    need = core._lib.crf_ctc_beam_chunk_workspace_bytes(2, 10, 8, 4, 5)
    rc, msg = call(ws_bytes=need - 1)
    assert rc == ERR_WORKSPACE and str(need) in msg
    rec = core._lib.crf_ctc_beam_state_record_bytes(4, 16)
    for so in (0x100000, 0x100000 + 8, 0x100000 + 2 * rec - 8, 0x100000 - 2 * rec + 8):        # B = 2 records each
        rc, msg = call({"state_out": so})
        assert rc == ERR_ARG and "overlaps" in msg, (hex(so), rc, msg)
    for so in (0x100004, 0x200001):
        rc, msg = call({"state_out": so})
        assert rc == ERR_ARG and ("aligned" in msg or "overlaps" in msg), (hex(so), rc, msg)
    rc, msg = call({"state_in": 0x100004})
    assert rc == ERR_ARG and "aligned" in msg
    if with_lm:
        for kw in (dict(alpha=float("nan")), dict(beta=float("-inf"))):
            rc, msg = call(**kw)
            assert rc == ERR_ARG and "finite" in msg, (kw, rc, msg)
        rc, msg = call(V=9)
        assert rc == ERR_ARG and "LM's V 8" in msg
        for tab in (dict(S=0), dict(order=9), dict(start=5)):
            rc, msg = call(**tab)
            assert rc == ERR_ARG and "bad LM tables" in msg, (tab, rc, msg)
        rc, msg = call(row_off=0)
        assert rc == ERR_ARG and "null LM table" in msg


def test_binding_host_checks(lm):
    """What the binding refuses before it touches the device -- on CPU tensors: the last check of all is the device's."""
    import ctc_crf
    N, T, V = 2, 6, 8
    x, lx = torch.zeros(N, T, V), torch.tensor([6, 4], dtype=torch.int32)
    fn = lambda **kw: ctc_crf.ctc_beam_search_chunk(x, kw.pop("lx", lx), **kw)
    with pytest.raises(RuntimeError, match="GPU"):                                     # all arguments fine: only the device is missing
        fn(lm=lm, alpha=0.5, beta=-1.0, return_lm_scores=True, reset=torch.tensor([True, False]), max_hyp_len=8192)
    for kw, msg in ((dict(beam_size=65), r"beam_size must lie in \[1, 64\], got 65"), (dict(nbest=17), r"nbest must lie in \[1, beam_size=16\], got 17"),
                    (dict(top_classes=0), r"top_classes must lie in \[1, 64\], got 0"), (dict(blank=8), r"blank must lie in \[0, V-1=7\], got 8"),
                    (dict(max_hyp_len=0), r"max_hyp_len must lie in \[1, 8192\], got 0"), (dict(max_hyp_len=8193), r"max_hyp_len must lie in \[1, 8192\], got 8193"),
                    (dict(lx=torch.tensor([6, 7])), r"lie in \[0, Tc=6\], got min 6, max 7"), (dict(lx=torch.tensor([-1, 3])), r"got min -1, max 3"),
                    (dict(lx=torch.tensor([6, 4, 1])), r"expect 2 input lengths"), (dict(lx=torch.tensor([6.0, 4.0])), r"must be an int tensor"),
                    (dict(reset=torch.tensor([1, 0, 0])), r"reset must be a bool or int tensor of shape \(2,\)"),
                    (dict(reset=torch.tensor([1.0, 0.0])), r"reset must be a bool or int tensor"),
                    (dict(state="a state"), r"state must be a BeamState.*got str"),
                    (dict(lm="lm.arpa", alpha=0.5), r"lm must be an NgramLM"), (dict(alpha=0.5), r"without lm they must be 0"),
                    (dict(lm=lm, alpha=float("nan")), r"alpha must be a finite number"), (dict(return_lm_scores=True), r"return_lm_scores needs lm")):
        with pytest.raises(RuntimeError, match=msg):
            fn(**kw)
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        ctc_crf.ctc_beam_search_chunk(torch.zeros(N, T, V, dtype=torch.float64), lx)
    with pytest.raises(RuntimeError, match="3 dimensions|got 2 dimensions"):
        ctc_crf.ctc_beam_search_chunk(torch.zeros(T, V), lx)
    with pytest.raises(RuntimeError, match=r"the LM is over 8 classes, the activations have V=5"):
        ctc_crf.ctc_beam_search_chunk(torch.zeros(N, T, 5), lx, lm=lm)


def test_beam_state_mismatches_are_named(core, lm):
    import ctc_crf
    N, T, V = 2, 6, 8
    x, lx = torch.zeros(N, T, V), torch.tensor([6, 4], dtype=torch.int32)
    made = dict(beam_size=16, top_classes=40, blank=0, max_hyp_len=512, lm=None, alpha=0.0, beta=0.0)
    rec = core._lib.crf_ctc_beam_state_record_bytes(16, 512)
    state = ctc_crf.BeamState(torch.zeros(N, rec, dtype=torch.uint8), **made)
    assert len(state) == N and len(state.index_select(torch.tensor([1]))) == 1 and state.clone().records is not state.records
    assert torch.equal(state.index_select(torch.tensor([1, 0, 1])).records, state.records[[1, 0, 1]])
    with pytest.raises(RuntimeError, match="GPU"):                                     # the same values: only the device is missing
        ctc_crf.ctc_beam_search_chunk(x, lx, state)
    other_lm = ctc_crf.NgramLM.from_ngrams(ngram_ref.random_model(2, 8, 2), 8)
    for field, kw in (("beam_size", dict(beam_size=8)), ("top_classes", dict(top_classes=7)), ("blank", dict(blank=3)),
                      ("max_hyp_len", dict(max_hyp_len=64)), ("lm", dict(lm=lm)), ("alpha", dict(lm=None, alpha=0.0, beta=0.0, _state=dict(alpha=0.5))),
                      ("beta", dict(_state=dict(beta=1.0)))):
        st = ctc_crf.BeamState(state.records, **dict(made, **kw.pop("_state", {})))
        with pytest.raises(RuntimeError, match=rf"the state was made with {field}="):
            ctc_crf.ctc_beam_search_chunk(x, lx, st, **kw)
    with_lm = ctc_crf.BeamState(state.records, **dict(made, lm=lm, alpha=0.5))
    with pytest.raises(RuntimeError, match=r"the state was made with lm=.*this call has lm=None"):
        ctc_crf.ctc_beam_search_chunk(x, lx, with_lm)
    with pytest.raises(RuntimeError, match=r"the state was made with lm="):
        ctc_crf.ctc_beam_search_chunk(x, lx, with_lm, lm=other_lm, alpha=0.5)
    with pytest.raises(RuntimeError, match=r"the state holds 2 utterances, the chunk 3"):
        ctc_crf.ctc_beam_search_chunk(torch.zeros(3, T, V), torch.tensor([1, 2, 3]), state)
