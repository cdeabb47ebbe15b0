"""CPU tests (no device) of the surface of ngram_score: the exports, every CRF_ERR_ARG of crf_ngram_score with its message -- answered
before any HIP call, so device pointers that point nowhere do -- H == 0, the Python argument errors, the keywords."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ngram_ref

SYMBOLS = ("crf_ngram_score", "crf_last_ngram_score_kernel")
NOWHERE = 0x1000             # a non-null "device pointer": never dereferenced by a call that is refused


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


@pytest.fixture(scope="module")
def lm():
    import ctc_crf
    return ctc_crf.NgramLM.from_ngrams(ngram_ref.random_model(1, 8, 3, eos=True), 8)


def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = open(core.LIB_PATH.rsplit("/cat_amd/", 1)[0] + "/include/ctc_crf_hip.h").read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in core.EXPORTED_SYMBOLS and s + "(" in hdr, s
    assert ctc_crf.ngram_score is cat_amd.ctc_crf.ngram_score
    par = inspect.signature(ctc_crf.ngram_score).parameters
    assert list(par) == ["hyps", "hyp_lengths", "lm", "bos", "eos", "return_token_scores"]
    assert (par["bos"].default, par["eos"].default, par["return_token_scores"].default) == (True, False, False)
    for word in ("argmax", "gather", "alpha", "beta", "NgramLM.score"):
        assert word in ctc_crf.ngram_score.__doc__, word
    import cat_amd.ngram_lm
    for doc in (cat_amd.ngram_lm.__doc__, ctc_crf.ctc_beam_search.__doc__):
        assert "in ngram_score, not in the search" in " ".join(doc.split()), doc
    assert "in crf_ngram_score, not in the search" in " ".join(hdr.split())
    assert isinstance(core.last_ngram_score_kernel(), str)


def call(core, lm, tables=True, eos=True, hyps=True, hyp_len=True, score=True, stride=16, H=4, use_start=1, add_eos=0, **change):
    """crf_ngram_score with pointers that point nowhere and one thing wrong -> (rc, message)."""
    import cat_amd.ngram_lm as m
    scal = dict(S=lm.num_states, A=lm.num_arcs, V=lm.vocab_size, order=lm.order, start=lm.start)
    ptrs = {n: NOWHERE for n in m.TABLE_NAMES}
    for k, v in change.items():
        if k in ptrs:
            ptrs[k] = v
        else:
            scal[k] = v
    st = m._Tables(*[ptrs[n] or None for n in m.TABLE_NAMES], scal["S"], scal["A"], scal["V"], scal["order"], scal["start"])
    vp = ctypes.c_void_p
    p = lambda on: vp(NOWHERE if on else 0)
    rc = core._lib.crf_ngram_score(ctypes.byref(st) if tables else None, p(eos), p(hyps), stride, p(hyp_len), H, use_start, add_eos, p(score),
                                   vp(0), vp(0), vp(0), vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_every_argument_error_is_answered_before_any_hip_call(core, lm):
    ARG = 3                                                                           # CRF_ERR_ARG
    assert call(core, lm, H=0)[0] == 0                                                # H == 0 succeeds and launches nothing
    assert call(core, lm, H=0, add_eos=1)[0] == 0
    cases = [
        (dict(tables=False), "null argument"), (dict(hyps=False), "null argument"), (dict(hyp_len=False), "null argument"),
        (dict(score=False), "null argument"),
        (dict(row_off=0), "null LM table"), (dict(bo_state=0), "null LM table"), (dict(bo_weight=0), "null LM table"),
        (dict(uni_logp=0), "null LM table"), (dict(uni_next=0), "null LM table"), (dict(arc_label=0), "null LM table"),
        (dict(arc_logp=0), "null LM table"), (dict(arc_next=0), "null LM table"),
        (dict(S=0), "bad LM tables: S 0,"), (dict(order=0), "order 0,"), (dict(order=9), "order 9,"), (dict(start=-1), "start -1"),
        (dict(start=lm.num_states), f"start {lm.num_states}"), (dict(V=0), "V 0,"), (dict(V=8193), "V 8193,"),
        (dict(H=-1), "H -1 is negative"), (dict(stride=0), "hyp_stride 0 outside [1, 8192]"), (dict(stride=8193), "hyp_stride 8193 outside [1, 8192]"),
        (dict(eos=False, add_eos=1), "add_eos needs eos_logp_dev"), (dict(eos=False, add_eos=1, H=0), "add_eos needs eos_logp_dev"),
    ]
    for kw, msg in cases:
        rc, text = call(core, lm, **kw)
        assert rc == ARG and text.startswith("crf_ngram_score: ") and msg in text, (kw, rc, text)
    # a model without arcs needs no arc tables
    uni = type(lm).from_ngrams({(c,): (-1.0, 0.0) for c in range(3)}, 3)
    assert uni.num_arcs == 0 and call(core, uni, H=0, arc_label=0, arc_logp=0, arc_next=0)[0] == 0


def test_python_argument_errors(lm):
    import ctc_crf
    hyps, hl = torch.zeros((3, 5), dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"NgramLM\.score"):
        ctc_crf.ngram_score(hyps, hl, lm)
    bare = ctc_crf.NgramLM.from_ngrams(ngram_ref.random_model(1, 8, 3), 8)
    assert bare.eos_logp is None
    with pytest.raises(ValueError, match=r"eos=True needs a model with a </s> unigram"):
        ctc_crf.ngram_score(hyps, hl, bare, eos=True)
    for args, msg in (((hyps.long(), hl, lm), r"rows \(H, W\) of int32"), ((hyps[0], hl, lm), r"rows \(H, W\) of int32"),
                      ((hyps, hl.long(), lm), r"hyp_lengths as an int32 tensor \(3,\)"), ((hyps, hl[:2], lm), r"hyp_lengths as an int32 tensor \(3,\)"),
                      ((hyps, hl, "lm.arpa"), r"lm must be an NgramLM"),
                      ((torch.zeros((1, 8193), dtype=torch.int32), hl[:1], lm), r"8193 > 8192")):
        with pytest.raises(RuntimeError, match=msg):
            ctc_crf.ngram_score(*args)
