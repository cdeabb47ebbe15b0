"""GPU tests of the streaming beam search, ctc_beam_search_chunk (include/ctc_crf_hip.h crf_ctc_beam_chunk), without an LM.  The yardstick
is the whole-utterance call ctc_beam_search -- itself held to tests/beam_ref.py and brute force by tests/test_gpu_ctc_beam.py -- and every
comparison is BIT FOR BIT: hyps[:len], hyp_lengths, scores, and the chunks' traces one after the other against the whole call's trace.
No tolerance: any split of the frames into chunks runs the same operations on the same operands -- the whole and the chunk kernels call
one frame step (cat_amd/csrc/k_beam_body.h); what differs, and what these tests hold, is the load, the store and the back-trace around it."""
import numpy as np
import pytest
import torch

from tests import beam_ref
from tests import beam_stream_ref as S
from tests.beam_stream_ref import DTYPES, i32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REENTER_CASES = [c for c in beam_ref.REPLAY_CASES if c[:5] in ((794, 3, 2, 8, 30), (1, 3, 3, 40, 30), (1, 9, 64, 8, 130))]
T130_CASE = [c for c in beam_ref.REPLAY_CASES if c[:5] == (1, 9, 64, 8, 130)][0]


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def check_splits(crf, x_cpu, lx, W, C, blank, dtype, splits, fused_modes=(False, True), what="", partial=False, **kw):
    """Every split, both layouts, fuse_log_softmax on and off: the last chunk's outputs and the concatenated traces equal the whole
    call's; partial: after every chunk they equal the whole call at min(lx, frames so far).  -> the whole call's dict (batch-major,
    not fused)."""
    x = torch.tensor(x_cpu).to(DTYPES[dtype]).to(DEV)
    first = None
    for fused in fused_modes:
        for tm in (False, True):
            xin = x.transpose(0, 1).contiguous() if tm else x
            want = S.whole(crf, xin, lx, W, W, C, blank, tm, fused, **kw)
            first = first or want
            partial_want = {}
            for split in splits:
                def on_chunk(j, seen, state, res):
                    if seen not in partial_want:
                        partial_want[seen] = S.whole(crf, xin, [min(l, seen) for l in lx], W, W, C, blank, tm, fused, **kw)
                    pw = partial_want[seen]
                    S.assert_same(dict(res, trace=pw["trace"]), pw, blank, (what, dtype, tm, fused, split, "after chunk", j))
                _, got = S.stream(crf, xin, lx, split, W, W, C, blank, tm, fused=fused, on_chunk=on_chunk if partial else None, **kw)
                S.assert_same(got, want, blank, (what, dtype, tm, fused, split))
    return first


# 1. any split equals the whole call
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("case", beam_ref.TIE_CASES, ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5])
def test_any_split_equals_whole_on_exact_ties(crf, case, dtype):
    """beam_ref.TIE_CASES: candidates tie exactly at every level of the total order and across the beam's edge, so a chunk boundary that
    changed the order of slots, the stay-first rule or the places in E_t would change a trace word.  In fp32 (the values of the cases) the
    result also equals beam_ref.search."""
    seed, V, W, C, T, blank, groups = case
    x = beam_ref.grouped_inputs(seed, T, V, blank, groups)
    lxs = (T, T - 1, 1)
    want = check_splits(crf, np.stack([x] * 3), lxs, W, C, blank, dtype, S.splits_of(T, seed), what=str(case))
    if dtype == "fp32":
        _, got = S.stream(crf, torch.tensor(np.stack([x] * 3), device=DEV), lxs, (1,) * T, W, W, C, blank)
        for b, lx in enumerate(lxs):
            ref = beam_ref.search(x, lx, W, W, C, blank)
            assert np.array_equal(got["trace"][b], ref["trace"]), (case, lx)
            for r in range(W):
                pre = ref["nbest"][r][0] if r < len(ref["nbest"]) else ()
                h = b * W + r
                assert got["len"][h] == len(pre) and tuple(got["hyps"][h, :len(pre)]) == pre, (case, lx, r)
            assert np.array_equal(got["trace"][b], want["trace"][b])


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("case", REENTER_CASES, ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5])
def test_any_split_equals_whole_with_merges_through_a_reentered_parent(crf, case, dtype):
    """REPLAY cases in which a prefix leaves the beam, comes back and merges into a child that stayed (asserted on the CPU): the ids of
    the prefixes and of their parents must survive the state.  The last is V = 9, W = 64, T = 130 with the splits whose chunk ends lie on,
    one before and two behind the 64-frame windows of the back-trace."""
    seed, V, W, C, T, lxs, blank = case
    x = beam_ref.make_inputs(seed, len(lxs), T, V)
    assert any(beam_ref.search(x[b], lx, W, W, C, blank)["reentered"] > 0 for b, lx in enumerate(lxs))
    splits = S.SPLITS_130 + S.random_splits(T, 3, seed) if T == 130 else S.splits_of(T, seed)
    fused_modes = (False, True) if dtype == "fp32" or T < 130 else (True,)
    check_splits(crf, x, lxs, W, C, blank, dtype, splits, fused_modes, what=str(case[:5]))


# 2. partial results
@pytest.mark.parametrize("case", [beam_ref.REPLAY_CASES[1], beam_ref.REPLAY_CASES[5]], ids=lambda c: "seed%d-V%d-W%d-C%d-T%d" % c[:5])
def test_partial_results_equal_the_whole_call_on_the_frames_so_far(crf, case):
    seed, V, W, C, T, lxs, blank = case
    x = beam_ref.make_inputs(seed, len(lxs), T, V)
    check_splits(crf, x, lxs, W, C, blank, "bf16", [(1,) * T] + S.random_splits(T, 2, seed), (True,), what=str(case[:5]), partial=True)


# 3. ragged batch
@pytest.mark.parametrize("lx_on_device", [False, True], ids=["lx-cpu", "lx-gpu"])
def test_ragged_batch_in_chunks_of_32(crf, lx_on_device):
    """lx = (130, 129, 128, 65, 64, 1, 0) in chunks of 32 (the last of 2): lx_chunk = clamp(lx - offset, 0, 32).  A finished utterance
    returns the same outputs from every later chunk and its record does not change; a chunk with every length 0 returns the state's bytes."""
    seed, V, W, C, T, _, blank = T130_CASE
    lx = (130, 129, 128, 65, 64, 1, 0)
    x = torch.tensor(beam_ref.make_inputs(seed, len(lx), T, V), device=DEV)
    want = S.whole(crf, x, lx, W, W, C, blank)
    seen_at, states = {}, []

    def on_chunk(j, seen, state, res):
        states.append(state.records.cpu().numpy())
        for b, l in enumerate(lx):
            if l <= seen:
                rows = slice(b * W, (b + 1) * W)
                now = (res["hyps"][rows], res["len"][rows], S.bits(res["score"][rows]), states[-1][b])
                if b in seen_at:
                    for a, c in zip(seen_at[b], now):
                        assert np.array_equal(a, c), (b, j)
                    assert (res["trace"][b] == -1).all()
                seen_at[b] = now

    split = (32, 32, 32, 32, 2)
    state, got = S.stream(crf, x, lx, split, W, W, C, blank, lx_on_device=lx_on_device, on_chunk=on_chunk)
    S.assert_same(got, want, blank, "ragged")
    zero = torch.zeros(len(lx), dtype=torch.int32, device=DEV if lx_on_device else "cpu")
    state2, res2 = S.step(crf, x[:, :3].contiguous(), zero, state, W, W, C, blank)
    assert torch.equal(state2.records, state.records) and state2.records.data_ptr() != state.records.data_ptr()
    S.assert_same(dict(res2, trace=got["trace"]), want, blank, "all lengths 0")
    assert (res2["trace"] == -1).all()
    if lx_on_device:                            # lengths the CPU path refuses: clamped in the kernel
        wild = torch.tensor([40, -3, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
        tame = torch.tensor([3, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
        a, ra = S.step(crf, x[:, :3].contiguous(), wild, None, W, W, C, blank)
        b, rb = S.step(crf, x[:, :3].contiguous(), tame, None, W, W, C, blank)
        assert torch.equal(a.records, b.records)
        S.assert_same(ra, rb, blank, "clamped lengths")


# 4. the beam dies and stays dead; V = 1 and W = 1
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_dead_beam_stays_dead(crf, dtype):
    """tests/test_gpu_ctc_beam.py minus_inf_inputs, not normalised: utterance 3 has frame 2 entirely at -inf -- from there on no rank, every
    score -inf, every trace word -1, in the chunk with the frame and in every chunk behind it."""
    from tests.test_gpu_ctc_beam import minus_inf_inputs
    V, W, C = 9, 8, 8
    x, blank = minus_inf_inputs(V, dtype, False)
    x = x.float().numpy()
    N, T = x.shape[:2]
    lx = [T] * N
    want = check_splits(crf, x, lx, W, C, blank, dtype, S.splits_of(T, 4), (False,), what="-inf")
    assert (want["len"][3 * W:] == 0).all() and (want["score"][3 * W:] == -np.inf).all() and (want["trace"][3, 2:] == -1).all()

    def on_chunk(j, seen, state, res):
        if seen >= 3:
            assert (res["score"][3 * W:] == -np.inf).all() and (res["len"][3 * W:] == 0).all() and (res["hyps"][3 * W:] == blank).all()
    S.stream(crf, torch.tensor(x).to(DTYPES[dtype]).to(DEV), lx, (1,) * T, W, W, C, blank, on_chunk=on_chunk)


@pytest.mark.parametrize("V,W,C", [(1, 4, 8), (1, 1, 1), (2, 1, 1), (7, 1, 3)])
def test_one_class_and_one_slot(crf, V, W, C):
    T, blank = 9, V - 1
    x = beam_ref.make_inputs(V + W, 3, T, V)
    check_splits(crf, x, (T, 4, 0), W, C, blank, "fp32", S.splits_of(T, V), what=f"V={V} W={W}")


# 5. reset and batch composition
def test_reset_reuses_a_batch_slot(crf):
    """Utterance A in slot 0 is reset mid-stream and the slot fed utterance B: slot 0 ends as B alone, the other slots as if nothing had
    happened.  reset as bool on the CPU and as int on the GPU."""
    seed, V, W, C, T, blank = 2, 5, 16, 8, 24, 0
    x = beam_ref.make_inputs(seed, 4, T, V)                    # utterances A, u1, u2 and B
    A, B = x[:3], np.stack([x[3], x[1], x[2]])
    xa, xb = torch.tensor(A, device=DEV), torch.tensor(B, device=DEV)
    want_b = S.whole(crf, xb[:1, :16].contiguous(), [16], W, W, C, blank)
    want_o = S.whole(crf, xa, [T, T, T], W, W, C, blank)
    for reset in (torch.tensor([True, False, False]), torch.tensor([7, 0, 0], dtype=torch.int64, device=DEV)):
        state, _ = S.step(crf, xa[:, :8].contiguous(), [8, 8, 8], None, W, W, C, blank)
        feed = torch.cat([xb[:1, :8], xa[1:, 8:16]]).contiguous()
        state, _ = S.step(crf, feed, [8, 8, 8], state, W, W, C, blank, reset=reset)
        feed = torch.cat([xb[:1, 8:16], xa[1:, 16:24]]).contiguous()
        state, got = S.step(crf, feed, [8, 8, 8], state, W, W, C, blank)
        for k in ("len", "score", "hyps"):
            assert np.array_equal(S.bits(got[k][:W][:, :16] if k == "hyps" else got[k][:W]), S.bits(want_b[k][:, :16] if k == "hyps" else want_b[k])), k
            assert np.array_equal(S.bits(got[k][W:][:, :T] if k == "hyps" else got[k][W:]), S.bits(want_o[k][W:])), k


def test_index_select_and_functional_state(crf):
    """state.index_select(perm) followed by the permuted chunks gives the permuted results; two continuations from one state give the same
    bits and leave the input state's bytes as they were; clone() and len()."""
    seed, V, W, C, T, blank = 3, 7, 8, 4, 20, 6
    N = 5
    x = torch.tensor(beam_ref.make_inputs(seed, N, T, V), device=DEV)
    lx = [20, 17, 20, 9, 0]
    want = S.whole(crf, x, lx, W, W, C, blank)
    state, _ = S.step(crf, x[:, :10].contiguous(), S.chunk_lengths(lx, 0, 10), None, W, W, C, blank)
    before = state.records.clone()
    assert len(state) == N and state.records.dtype == torch.uint8 and state.records.shape == (N, crf._C._lib.crf_ctc_beam_state_record_bytes(W, 512))
    perm = [3, 0, 4, 2, 1]
    idx = torch.tensor(perm, device=DEV)
    sel = state.index_select(idx)
    assert len(sel) == N and torch.equal(sel.records, state.records[idx])
    rest = x[:, 10:].contiguous()
    _, a = S.step(crf, rest, S.chunk_lengths(lx, 10, 10), state, W, W, C, blank)
    _, b = S.step(crf, rest, S.chunk_lengths(lx, 10, 10), state.clone(), W, W, C, blank)
    _, p = S.step(crf, rest[idx].contiguous(), [S.chunk_lengths(lx, 10, 10)[i] for i in perm], sel, W, W, C, blank)
    assert torch.equal(state.records, before)
    S.assert_same(dict(a, trace=want["trace"]), want, blank, "first continuation")
    for k in ("hyps", "len", "score", "trace"):
        assert np.array_equal(S.bits(a[k]), S.bits(b[k])), k
        rows = np.concatenate([np.arange(i * W, (i + 1) * W) for i in perm]) if k != "trace" else np.array(perm)
        assert np.array_equal(S.bits(p[k]), S.bits(a[k][rows])), k


# 6. capacity
def test_prefixes_longer_than_max_hyp_len(crf):
    """Peaked rows over alternating labels, T = 40: the best hypothesis has 20 labels or more (asserted on the CPU reference).  With
    max_hyp_len = 8 the scores, lengths and traces are those of max_hyp_len = 64, the rows hold the first 8 labels, and ctc_edit_distance
    answers the rows over the bound with -1."""
    T, V, W, C, blank = 40, 5, 8, 4, 0
    rng = np.random.default_rng(40)
    x = np.full((2, T, V), -5.0) - rng.random((2, T, V))
    for t in range(T):
        x[0, t, 1 + t % 2] = -0.05
        x[1, t, 1 + (t // 2) % 3] = -0.05
    x = x.astype(np.float32)
    ref = [beam_ref.search(x[b], T, W, W, C, blank) for b in range(2)]
    assert all(len(r["nbest"][0][0]) >= 16 for r in ref), [len(r["nbest"][0][0]) for r in ref]
    xd = torch.tensor(x, device=DEV)
    want = S.whole(crf, xd, [T, T], W, W, C, blank)
    for split in [(T,), (1,) * T, (7, 13, 20)]:
        _, big = S.stream(crf, xd, [T, T], split, W, W, C, blank, cap=64)
        _, small = S.stream(crf, xd, [T, T], split, W, W, C, blank, cap=8)
        S.assert_same(big, want, blank, ("cap 64", split))
        assert small["hyps"].shape == (2 * W, 8) and int(small["len"].max()) >= 16
        for k in ("len", "score", "trace"):
            assert np.array_equal(S.bits(small[k]), S.bits(big[k])), (k, split)
        for h in range(2 * W):
            n = min(int(big["len"][h]), 8)
            assert np.array_equal(small["hyps"][h, :n], big["hyps"][h, :n]) and (small["hyps"][h, n:] == blank).all(), (h, split)
    hyps, hl = torch.tensor(small["hyps"], device=DEV), torch.tensor(small["len"], device=DEV)
    hu = torch.arange(2 * W, dtype=torch.int32, device=DEV) // W
    labels = torch.tensor(list(ref[0]["nbest"][0][0]) + list(ref[1]["nbest"][0][0]), dtype=torch.int32)
    ll = torch.tensor([len(ref[0]["nbest"][0][0]), len(ref[1]["nbest"][0][0])], dtype=torch.int32)
    dist = crf.ctc_edit_distance(hyps, hl, labels, ll, hu).cpu().numpy()
    over = small["len"] > 8
    assert over.any() and (dist[over] == -1).all() and (dist[~over] >= 0).all()


# 8. no synchronisation
def test_the_chunk_loop_never_synchronises(crf):
    N, T, V, W = 4, 48, 12, 8
    x = torch.tensor(beam_ref.make_inputs(5, N, T, V), device=DEV)
    lens_cpu = [i32([16, 16, 9, 0]), i32([16, 3, 0, 0]), i32([16, 0, 0, 0])]
    lens_dev = [l.to(DEV) for l in lens_cpu]
    reset = torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=DEV)
    idx = torch.tensor([1, 0, 3, 2], device=DEV)
    want = S.whole(crf, x, [48, 19, 9, 0], W, 2, 6, 0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):      # the positive control: this build enforces the mode
            torch.ones(1, device=DEV).item()
        outs = []
        for lens in (lens_cpu, lens_dev):
            state = None
            for j in range(3):
                out = crf.ctc_beam_search_chunk(x[:, 16 * j:16 * j + 16].contiguous(), lens[j], state, reset if j == 0 else None, W, 2, 6)
                state = out[0]
            outs.append(out)
            state.index_select(idx).clone()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for out in outs:
        assert np.array_equal(out[2].cpu().numpy(), want["len"]) and np.array_equal(S.bits(out[4].cpu().numpy()), S.bits(want["score"]))
