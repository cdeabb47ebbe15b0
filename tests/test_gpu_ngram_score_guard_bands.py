"""GPU test: crf_ngram_score through the C ABI on buffers carved from a guard-banded arena (tests/guard.py), as
tests/test_gpu_edit_guard_bands.py does for the edit distance -- the eight tables, eos_logp, the rows, the lengths and every output come
from the 0xFF arena, each exactly as long as its sizes say; hyp_stride larger than any row's use; the optional outputs NULL and non-NULL;
the outputs prefilled with a sentinel.  No byte outside the call's own buffers may change, no input may change, every output word must
be written, and the results equal the host walk.  There is no workspace.

One run takes tables that FAIL crf_ngram_tables_check -- state and arc indices far out of range, a bo_state cycle -- uploaded regardless
and the call made directly: every index is clamped and every loop bounded (k_ngram_common.h), so only the guard bands and termination
are checked.  It is the check that the clamps are there."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ngram_ref
from tests.guard import Arena

pytestmark = pytest.mark.gpu
SENT = -77
I32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf._C


def run_score(core, lm, tabs, eos_tab, rows, lens, use_start, add_eos, with_tokens, with_invalid=True):
    """rows: CPU int32 [H, stride]; tabs: {table name: CPU tensor}.  -> {output name: numpy} after the guard and input checks."""
    dev = torch.device("cuda", 0)
    H, stride = rows.shape
    ins = [("lm." + n, t) for n, t in tabs.items() if t.numel()]            # (an order-1 model has no arcs: those tables are NULL)
    ins += [("eos", eos_tab), ("hyps", rows), ("hyp_len", torch.tensor(lens, dtype=torch.int32))]
    outs = [("score", H)] + ([("invalid", H)] if with_invalid else []) + ([("token_logp", H * stride), ("token_order", H * stride)] if with_tokens else [])
    arena = Arena(dev, Arena.room([4 * max(t.numel(), 1) for _, t in ins] + [4 * n for _, n in outs]))
    for name, t in ins:
        arena.carve(name, 4 * t.numel())
        arena.put(name, t)
    for name, n in outs:
        arena.carve(name, 4 * n)
        arena.put(name, torch.full((n,), SENT, dtype=torch.int32))
    vp = ctypes.c_void_p
    P = lambda name: arena.ptr(name) if name in arena.carves else vp(0)
    st = lm._struct(lambda name: P("lm." + name).value if tabs[name].numel() else None)
    stream = vp(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = core._lib.crf_ngram_score(ctypes.byref(st), P("eos"), P("hyps"), stride, P("hyp_len"), H, use_start, add_eos, P("score"),
                                       P("invalid"), P("token_logp"), P("token_order"), stream)
    assert rc == 0, core._lib.crf_last_error().decode()
    torch.cuda.synchronize()
    arena.check()
    for name, t in ins:
        assert torch.equal(arena.get(name, torch.uint8), t.contiguous().reshape(-1).view(torch.uint8)), f"the call wrote to {name}"
    got = {name: arena.get(name, torch.int32).numpy() for name, _ in outs}
    assert not any(np.any(a == SENT) for a in got.values()), "an output word was not written"
    return got


def case(order, V, seed):
    import ctc_crf
    ng = ngram_ref.random_model(seed, V, order, bos=True, eos=True)
    lm = ctc_crf.NgramLM.from_ngrams(ng, V)
    rng = np.random.default_rng(seed)
    stride, used = 200, 130                                                 # rows wider than any hypothesis
    lens = [used, 65, 0, 1, 64, 10, -3, stride + 1, 7]                      # rows 6 and 7 have no length; row 8 holds a token V
    rows = torch.tensor(rng.integers(0, V, (len(lens), stride)), dtype=torch.int32)
    rows[8, 3] = V
    for h, n in enumerate(lens):                                            # what stands behind a length is never read
        rows[h, max(n, 0):] = I32_MIN
    return lm, rows, lens


@pytest.mark.parametrize("order,V", [(1, 5), (3, 9), (5, 40), (8, 3)])
def test_ngram_score_writes_only_its_own_memory(core, order, V):
    lm, rows, lens = case(order, V, 31 + order)
    tabs = {name: torch.from_numpy(np.ascontiguousarray(a)) for name, a in lm.host_tables().items()}
    eos = torch.from_numpy(lm.eos_logp.copy())
    H, stride = rows.shape
    for use_start, add_eos, with_tokens, with_invalid in ((1, 1, True, True), (0, 0, False, True), (1, 0, True, False), (0, 1, False, False)):
        got = run_score(core, lm, tabs, eos, rows, lens, use_start, add_eos, with_tokens, with_invalid)
        assert core.last_ngram_score_kernel() == ("crf_ngram_score_kernel<tokens>" if with_tokens else "crf_ngram_score_kernel<scores>")
        sc = got["score"].view(np.float32)
        for h, n in enumerate(lens):
            bad = not 0 <= n <= stride or h == 8
            if with_invalid:
                assert got["invalid"][h] == int(bad), h
            if bad:
                assert sc[h] == -np.inf
                if with_tokens:
                    assert not got["token_logp"].reshape(H, stride)[h].any() and not got["token_order"].reshape(H, stride)[h].any()
                continue
            toks = rows[h, :n].tolist()
            lps, orders = lm.token_scores(toks, bos=bool(use_start))
            s = lm.start if use_start else 0
            for c in toks:
                s = lm.lookup(s, c)[1]
            want = float(np.sum(np.asarray(lps, dtype=np.float64))) + (float(lm.eos_logp[s]) if add_eos else 0.0)
            assert abs(float(sc[h]) - want) <= 2.0 ** -23 * abs(want), (h, sc[h], want)
            if with_tokens:
                tl = got["token_logp"].view(np.float32).reshape(H, stride)[h]
                to = got["token_order"].reshape(H, stride)[h]
                assert np.array_equal(tl[:n].view(np.int32), np.asarray(lps, dtype=np.float32).view(np.int32)) and not tl[n:].any()
                assert to[:n].tolist() == orders and not to[n:].any()


def test_tables_that_fail_the_check_stay_inside_their_buffers(core):
    lm, rows, lens = case(4, 9, 77)
    host = {name: np.ascontiguousarray(a).copy() for name, a in lm.host_tables().items()}
    S, A = lm.num_states, lm.num_arcs
    assert S > 6 and A > 6
    host["arc_next"][::2] = 2 ** 30                                         # states far out of range ...
    host["arc_next"][1::4] = -5
    host["uni_next"][::3] = 2 ** 31 - 1
    host["row_off"][2:S:3] = 2 ** 29                                        # ... arc indices too, and rows that run backwards
    host["row_off"][3:S:5] = -7
    host["bo_state"][1:] = np.arange(1, S, dtype=np.int32)[::-1]            # back-offs that lead upwards, and in circles
    host["bo_state"][S // 2] = S // 2
    host["arc_label"][::2] = -1
    tabs = {name: torch.from_numpy(a) for name, a in host.items()}
    import cat_amd.ngram_lm as m
    st = m._Tables(*[host[n].ctypes.data for n in m.TABLE_NAMES], S, A, lm.vocab_size, lm.order, lm.start)
    assert core._lib.crf_ngram_tables_check(ctypes.byref(st)) != 0         # the tables are bad indeed
    eos = torch.from_numpy(lm.eos_logp.copy())
    for with_tokens in (True, False):
        got = run_score(core, lm, tabs, eos, rows, lens, 1, 1, with_tokens)  # (unspecified values: the bands and the end of the call count)
        assert got["score"].shape == (len(lens),)
