"""CPU tests (no GPU) of ctc_edit_distance: the yardstick itself (tests/edit_ref.py: the loop against hand-worked values, identity,
symmetry of the cost and a case that tells the tie orders apart; the anti-diagonal NumPy form against the loop), the host checks of the
Python binding (cat_amd/ctc_crf/_C.py ctc_edit_distance) and the C ABI's answers before any HIP call (include/ctc_crf_hip.h
crf_ctc_edit_distance)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import edit_ref

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, 3, 5, 6
SYMBOLS = ("crf_ctc_edit_distance", "crf_last_edit_kernel")
KERNELS = ("crf_ctc_edit_kernel<1>", "crf_ctc_edit_kernel<2>", "crf_ctc_edit_kernel<4>", "crf_ctc_edit_kernel<8>", "crf_ctc_edit_kernel<8, strips>")


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def _s(word):
    return [ord(c) for c in word]


def test_loop_hand_worked():
    """kitten -> sitting: k/s and e/i substituted, g inserted.  Empty sequences: the borders.  The counts add up to the cost."""
    assert edit_ref.loop(_s("kitten"), _s("sitting")) == (3, 2, 0, 1)
    assert edit_ref.loop(_s("sitting"), _s("kitten")) == (3, 2, 1, 0)
    assert edit_ref.loop([], []) == (0, 0, 0, 0)
    assert edit_ref.loop([], [5, 5, 7]) == (3, 0, 0, 3)                            # reference empty: every token inserted
    assert edit_ref.loop([5, 5, 7], []) == (3, 0, 3, 0)                            # hypothesis empty: every token deleted
    assert edit_ref.loop([1, 2, 3], [1, 3]) == (1, 0, 1, 0) and edit_ref.loop([1, 3], [1, 2, 3]) == (1, 0, 0, 1)
    assert edit_ref.loop([1, 2, 3], [4, 5, 6]) == (3, 3, 0, 0)
    assert edit_ref.loop([2 ** 31 - 1, -(2 ** 31)], [-(2 ** 31), 2 ** 31 - 1]) == (2, 2, 0, 0)   # tokens are plain int32 words


def test_loop_identity_symmetry_and_counts():
    rng = np.random.default_rng(11)
    for _ in range(300):
        A = int(rng.choice([2, 3, 40]))
        a = rng.integers(0, A, int(rng.integers(0, 14))).tolist()
        b = rng.integers(0, A, int(rng.integers(0, 14))).tolist()
        assert edit_ref.loop(a, a) == (0, 0, 0, 0)
        d, ns, nd, ni = edit_ref.loop(a, b)
        assert d == ns + nd + ni and len(a) - ns - nd == len(b) - ns - ni >= 0     # hits, counted on either side
        assert edit_ref.loop(b, a)[0] == d and abs(len(a) - len(b)) <= d <= max(len(a), len(b))
        for order in (("del", "ins", "diag"), ("ins", "del", "diag")):             # the cost does not depend on the tie rule
            assert edit_ref.loop(a, b, order)[0] == d


def test_tie_rule_decides_the_counts():
    """r = 0 0 1 0, y = 1 2 0 2 costs 4 along four substitutions, along two substitutions with a deletion and an insertion, and along
    two deletions and two insertions: whichever candidate goes first among equals decides.  The contract's order is diag, del, ins."""
    r, y = [0, 0, 1, 0], [1, 2, 0, 2]
    assert edit_ref.ORDER == ("diag", "del", "ins")
    assert edit_ref.loop(r, y) == (4, 4, 0, 0)
    assert edit_ref.loop(r, y, ("del", "ins", "diag")) == (4, 2, 1, 1)
    assert edit_ref.loop(r, y, ("ins", "del", "diag")) == (4, 0, 2, 2)
    assert edit_ref.antidiag(r, y) == (4, 4, 0, 0)


def test_antidiag_equals_the_loop():
    rng = np.random.default_rng(0)
    refs, hyps = [], []
    for _ in range(400):
        A = int(rng.choice([2, 3, 5000]))
        refs.append(rng.integers(0, A, int(rng.integers(0, 13))).tolist())
        hyps.append(rng.integers(0, A, int(rng.integers(0, 13))).tolist())
    refs += [[], [], [1], [3, 3, 3]]
    hyps += [[], [1], [], [3, 3, 3]]
    got = edit_ref.antidiag_batch(refs, hyps)
    for p, (r, y) in enumerate(zip(refs, hyps)):
        assert tuple(got[p]) == edit_ref.loop(r, y), (r, y)
    for p in range(0, 40):                                                          # one pair at a time: no padding at all
        assert edit_ref.antidiag(refs[p], hyps[p]) == edit_ref.loop(refs[p], hyps[p])
    # longer than one wave's rows, a small alphabet: ties everywhere
    r, y = rng.integers(0, 2, 70).tolist(), rng.integers(0, 2, 90).tolist()
    assert edit_ref.antidiag(r, y) == edit_ref.loop(r, y)
    assert edit_ref.wer([1, 2, 0], [4, 4, 4]) == 0.25


def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    lib = ctypes.CDLL(core.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in core.EXPORTED_SYMBOLS
    assert callable(ctc_crf.ctc_edit_distance) and ctc_crf.ctc_edit_distance is cat_amd.ctc_crf.ctc_edit_distance
    assert callable(core.ctc_edit_distance) and callable(core.last_edit_kernel)
    doc = ctc_crf.ctc_edit_distance.__doc__
    assert "MWER" in doc and "risk" in doc and "cal_wer" in doc and "Levenshtein" in doc
    assert "ctc_edit_distance" in cat_amd.ctc_crf.__doc__
    assert not any("edit" in s and "workspace" in s for s in core.EXPORTED_SYMBOLS)      # LDS only: there is no workspace to ask for


PTRS = dict(hyps=0x1000, hyp_len=0x2000, hyp_utt=0x3000, refs=0x4000, ref_off=0x5000, ref_len=0x6000, dist=0x7000, ops=0x8000)


def _call(core, ptrs=None, stride=40, B=2, H=6, max_ref_len=30):
    """crf_ctc_edit_distance with fake (never dereferenced) device pointers: every argument error is answered before any HIP call."""
    p = dict(PTRS)
    p.update(ptrs or {})
    vp = ctypes.c_void_p
    rc = core._lib.crf_ctc_edit_distance(vp(p["hyps"]), stride, vp(p["hyp_len"]), vp(p["hyp_utt"]), vp(p["refs"]), vp(p["ref_off"]),
                                         vp(p["ref_len"]), B, H, max_ref_len, vp(p["dist"]), vp(p["ops"]), vp(0))
    return rc, core._lib.crf_last_error().decode()


def test_argument_errors_without_gpu(core):
    for name in ("hyps", "hyp_len", "hyp_utt", "refs", "ref_off", "ref_len", "dist"):
        rc, msg = _call(core, {name: 0})
        assert rc == ERR_ARG and "crf_ctc_edit_distance" in msg and "null" in msg, (name, rc, msg)
    for kw in (dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(stride=0), dict(stride=-5), dict(max_ref_len=-1), dict(B=1 << 31), dict(H=1 << 31)):
        rc, msg = _call(core, **kw)
        assert rc == ERR_ARG and "crf_ctc_edit_distance" in msg and "bad" in msg, (kw, rc, msg)
    for H, stride in ((1 << 16, 1 << 15), (3, 1 << 30), ((1 << 31) - 1, 2)):
        rc, msg = _call(core, H=H, stride=stride)
        assert rc == ERR_ARG and "H * hyp_stride > INT32_MAX" in msg, (H, stride, rc, msg)
    for n in (2048, 4096, 1 << 40):
        rc, msg = _call(core, max_ref_len=n)
        assert rc == ERR_UNSUPPORTED and "2047" in msg, (n, rc, msg)
    # the strips' cap on the rows of hyps: references of more than 512 tokens together with rows of more than 8192 entries
    for n, stride in ((513, 8193), (2047, 100000)):
        rc, msg = _call(core, max_ref_len=n, stride=stride)
        assert rc == ERR_UNSUPPORTED and "8192" in msg and "512" in msg and str(stride) in msg, (n, stride, rc, msg)
    assert core.last_edit_kernel() in ("",) + KERNELS


def _i32(*a):
    return torch.tensor(a, dtype=torch.int32)


def test_binding_host_checks():
    """What the binding refuses before it touches the device -- on CPU tensors: the last check of all is the device's."""
    import ctc_crf
    hyps, hl, lab, ly = torch.zeros((2, 5), dtype=torch.int32), _i32(5, 3), _i32(1, 2, 3, 4), _i32(3, 1)

    def fn(**kw):
        return ctc_crf.ctc_edit_distance(kw.pop("hyps", hyps), kw.pop("hl", hl), kw.pop("lab", lab), kw.pop("ly", ly), **kw)

    with pytest.raises(RuntimeError, match="hyps must be on the GPU"):                 # CPU hyps: there is no CPU path
        fn()
    with pytest.raises(RuntimeError, match="hyps must be on the GPU"):
        fn(hyp_utt=_i32(1, 0), return_ops=True)
    for dtype in (torch.int64, torch.float32, torch.int16):
        with pytest.raises(RuntimeError, match=r"expect int32 hyps, got " + str(dtype).replace(".", r"\.")):
            fn(hyps=hyps.to(dtype))
    with pytest.raises(RuntimeError, match=r"expect int32 hyp_lengths, got torch\.int64"):
        fn(hl=hl.long())
    with pytest.raises(RuntimeError, match=r"expect int32 hyp_utt, got torch\.int64"):
        fn(hyp_utt=torch.tensor([0, 1]))
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros((2, 5, 1), dtype=torch.int32)):
        with pytest.raises(RuntimeError, match=rf"expect hyps of shape \(H, W\), got {bad.dim()} dimensions"):
            fn(hyps=bad)
    with pytest.raises(RuntimeError, match=r"expect hyp_lengths of shape \(2,\)"):
        fn(hl=_i32(5, 3, 1))
    with pytest.raises(RuntimeError, match=r"expect hyp_utt of shape \(2,\)"):
        fn(hyp_utt=_i32(0, 1, 1))
    with pytest.raises(RuntimeError, match=r"hyp_utt=None.*expect 2 hypotheses, got 3"):
        fn(hyps=torch.zeros((3, 5), dtype=torch.int32), hl=_i32(1, 1, 1))
    with pytest.raises(RuntimeError, match=r"expect label_lengths of shape \(N,\)"):
        fn(ly=torch.zeros((2, 1), dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"integer labels"):
        fn(lab=lab.float())
    with pytest.raises(RuntimeError, match=r"negative label length"):
        fn(ly=_i32(3, -1))
    with pytest.raises(RuntimeError, match=r"sum\(label_lengths\)=5 exceeds len\(labels\)=4"):
        fn(ly=_i32(3, 2))
    with pytest.raises(RuntimeError, match=r"label length 2048 > 2047"):
        fn(lab=torch.zeros(2049, dtype=torch.int32), ly=_i32(2048, 1))
    with pytest.raises(RuntimeError, match=r"8193 > 8192"):
        fn(hyps=torch.zeros((2, 8193), dtype=torch.int32), lab=torch.zeros(514, dtype=torch.int32), ly=_i32(513, 1))
