"""CPU tests (no device) of the CTC-Transducer loss: the yardstick of tests/ctct_ref.py held to itself -- the numpy recursion against the
enumeration of every frame labelling (1e-10), its closed-form gradients against torch autograd (1e-10), the per-frame sum of the
gradient, plain CTC on u-independent input (F.ctc_loss in fp64, 1e-9) -- and the surface: the signature, the exports, the warp_ctct
shim, ValueError for every bad argument before any device call, every argument error of the C calls (answered before any HIP call, so
device pointers that point nowhere do) and the workspace formula."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctct_ref

SYMBOLS = ("crf_ctct_workspace_bytes", "crf_ctct_loss", "crf_ctct_loss_logits", "crf_ctct_grad", "crf_ctct_grad_logits",
           "crf_debug_ctct_ws_sections", "crf_debug_ctct_ws_section_names")
NOWHERE = 0x1000             # a non-null, 16-byte aligned "device pointer": never dereferenced by a call that is refused
ARG, WORKSPACE, UNSUPPORTED = 3, 5, 6
EPS = 1e-10
# (T, y, V, blank): single labels, repeats that are just feasible and infeasible ones, every blank position, a label 0 beside blank = 1
CASES = [(1, [], 2, 0), (3, [], 3, 1), (1, [1], 2, 0), (2, [1], 3, 2), (2, [1, 1], 2, 0), (3, [1, 1], 2, 0), (4, [1, 1], 3, 0),
         (4, [1, 1, 1], 2, 0), (5, [1, 1, 1], 2, 0), (5, [2, 2, 1], 4, 3), (6, [2, 2, 1], 4, 3), (4, [0, 2, 0], 3, 1), (5, [0, 0, 2], 3, 1),
         (6, [1, 2, 1], 3, 0), (6, [1, 2, 2, 1], 4, 0), (5, [3, 1, 1], 4, 0), (2, [1, 2, 1], 3, 0)]
INFEASIBLE = {(2, (1, 1)), (4, (1, 1, 1)), (2, (1, 2, 1))}


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def _rand(seed, T, U, V):
    return np.random.default_rng(seed).standard_normal((T, U + 1, V)) * 2.0


# ---- the yardstick ----
@pytest.mark.parametrize("T,y,V,blank", CASES)
def test_recursion_equals_the_enumeration_of_every_frame_labelling(T, y, V, blank):
    x = _rand(T * 10 + len(y), T, len(y), V)
    lp = ctct_ref.log_softmax(x)
    dead = lp.copy()
    dead[T // 2, len(y) // 2, blank] = -np.inf                       # ... and with a blank cut out of the lattice
    for inp in (lp, x, dead):                                        # (nothing in the recursion needs a normalised input)
        cost, grad = ctct_ref.ref_normalised(inp, y, blank)
        want = ctct_ref.brute_force(inp, y, blank)
        if np.isinf(want):
            assert cost == np.inf and not grad.any()
        else:
            assert abs(cost - want) <= EPS * max(1.0, abs(cost)), (cost, want)
            assert np.isfinite(grad).all()
    assert (ctct_ref.brute_force(lp, y, blank) == np.inf) == ((T, tuple(y)) in INFEASIBLE)
    assert (T < len(y) + ctct_ref.repeats(y)) == ((T, tuple(y)) in INFEASIBLE)
    cost = ctct_ref.ref_logits(x, y, blank)[0]
    want = ctct_ref.brute_force(lp, y, blank)
    assert cost == want or abs(cost - want) <= EPS * max(1.0, abs(cost))


@pytest.mark.parametrize("T,y,V,blank", CASES + [(9, [1, 1, 4, 2, 2, 2], 6, 0), (14, [3, 0, 0, 1, 3, 3, 2, 0], 5, 4)])
def test_closed_form_gradients_equal_autograd(T, y, V, blank):
    x = _rand(T * 7 + len(y), T, len(y), V)
    cut = x.copy()
    cut[T // 2, len(y) // 2, blank] = -np.inf                        # an entry of -inf: no gradient through it, none of NaN
    for inp, normalise in ((x, True), (x, False), (cut, True), (cut, False)):
        cost, grad = (ctct_ref.ref_logits if normalise else ctct_ref.ref_normalised)(inp, y, blank)
        tc, leaf = ctct_ref.torch_cost(inp, y, blank, normalise=normalise)
        if not np.isfinite(cost):
            assert float(tc.detach()) == np.inf and not grad.any()
            continue
        tc.backward()
        assert abs(cost - float(tc.detach())) <= EPS * max(1.0, abs(cost))
        auto = torch.nan_to_num(leaf.grad, nan=0.0).numpy()          # (log_softmax's backward at a -inf entry: 0 * inf)
        assert np.isfinite(grad).all() and np.max(np.abs(grad - auto)) <= EPS, np.max(np.abs(grad - auto))


@pytest.mark.parametrize("T,y,V,blank", [c for c in CASES if (c[0], tuple(c[1])) not in INFEASIBLE] + [(14, [3, 0, 0, 1, 3, 3, 2, 0], 5, 4)])
def test_every_frame_is_consumed_exactly_once(T, y, V, blank):
    """sum over u and v of the normalised gradient of a frame = -1; the raw gradient of every row sums to 0."""
    x = _rand(T + len(y), T, len(y), V)
    _, grad = ctct_ref.ref_normalised(ctct_ref.log_softmax(x), y, blank)
    assert np.max(np.abs(grad.sum((1, 2)) + 1.0)) <= EPS
    _, raw = ctct_ref.ref_logits(x, y, blank)
    assert np.max(np.abs(raw.sum(-1))) <= EPS


@pytest.mark.parametrize("T,y,V,blank", [(1, [], 2, 0), (2, [1, 1], 2, 0), (3, [1, 1], 2, 0), (5, [2, 2, 1], 4, 3), (6, [2, 2, 1], 4, 3),
                                         (4, [0, 2, 0], 3, 1), (12, [1, 1, 4, 2, 2, 2], 6, 0), (20, [3, 0, 0, 1, 3, 3, 2, 0], 5, 4)])
def test_input_independent_of_u_is_plain_ctc(T, y, V, blank):
    rng = np.random.default_rng(T + V)
    lp1 = ctct_ref.log_softmax(rng.standard_normal((T, V)) * 2.0)
    lp = np.repeat(lp1[:, None, :], len(y) + 1, axis=1)
    cost, grad = ctct_ref.ref_normalised(lp, y, blank)
    leaf = torch.tensor(lp1[:, None, :], requires_grad=True)
    want = F.ctc_loss(leaf, torch.tensor([y], dtype=torch.long), torch.tensor([T]), torch.tensor([len(y)]), blank=blank, reduction="sum",
                      zero_infinity=False) if y else -leaf[:, 0, blank].sum()
    if T < len(y) + ctct_ref.repeats(y):
        assert cost == np.inf and float(want.detach()) == np.inf
        return
    assert abs(cost - float(want.detach())) <= 1e-9 * max(1.0, abs(cost))
    want.backward()
    # F.ctc_loss's gradient is the one with respect to the logits behind a log_softmax; on a normalised input that is g - softmax * sum g
    folded = grad.sum(1) - np.exp(lp1) * grad.sum((1, 2))[:, None] if y else grad.sum(1)
    assert np.max(np.abs(folded - leaf.grad[:, 0].numpy())) <= 1e-9


# ---- the surface ----
def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    import warp_ctct
    from warp_ctct import ctct_loss
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = open(core.LIB_PATH.rsplit("/cat_amd/", 1)[0] + "/include/ctc_crf_hip.h").read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in core.EXPORTED_SYMBOLS and s + "(" in hdr, s
    assert warp_ctct.ctct_loss is ctc_crf.ctct_loss and ctct_loss is cat_amd.ctc_crf.ctct_loss
    par = inspect.signature(ctc_crf.ctct_loss).parameters
    assert list(par)[:8] == ["log_probs", "labels", "frames_lengths", "labels_lengths", "average_frames", "reduction", "blank", "fuse_log_softmax"]
    assert [par[k].default for k in list(par)[4:8]] == [False, None, 0, False]
    assert "compact" not in par
    for word in ("warp_ctct", "rnnt_loss", "compact", "ctct_simple_loss", "decoding", "1023", "8192"):
        assert word in ctc_crf.ctct_loss.__doc__, word
    with pytest.raises(NotImplementedError, match="ctct_loss"):
        warp_ctct.ctct_simple_loss(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), None, None, None)
    assert hasattr(core, "ctct_loss_fwd") and hasattr(core, "ctct_loss_bwd")


def _call(core, fn="crf_ctct_loss", x=True, labels=True, lx=True, ly=True, out=True, weight=True, ws=NOWHERE, dtype=0, blank=0, N=2, T=5, U1=4,
          V=7, ws_bytes=None):
    vp = ctypes.c_void_p
    p = lambda on: vp(NOWHERE if on else 0)
    if ws_bytes is None:
        ws_bytes = max(core._lib.crf_ctct_workspace_bytes(N, T, U1, V), 0)
    head = (p(x), dtype) if fn.endswith("_logits") else (p(x),)
    mid = (blank, p(labels), p(lx), p(ly), N, T, U1, V)
    tail = (p(weight), p(out)) if "grad" in fn else (p(out), vp(0))
    rc = getattr(core._lib, fn)(*head, *mid, *tail, vp(ws), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


@pytest.mark.parametrize("fn", ["crf_ctct_loss", "crf_ctct_loss_logits", "crf_ctct_grad", "crf_ctct_grad_logits"])
def test_every_argument_error_is_answered_before_any_hip_call(core, fn):
    cases = [(dict(x=False), ARG, "null argument"), (dict(labels=False), ARG, "null argument"), (dict(lx=False), ARG, "null argument"),
             (dict(ly=False), ARG, "null argument"), (dict(out=False), ARG, "null argument"), (dict(ws=0), ARG, "null argument"),
             (dict(U1=1025), UNSUPPORTED, "U > 1023"), (dict(V=8193), UNSUPPORTED, "V > 8192"),
             (dict(N=0), ARG, "bad N/T/U+1/V"), (dict(T=0), ARG, "bad N/T/U+1/V"), (dict(U1=0), ARG, "bad N/T/U+1/V"), (dict(V=0), ARG, "bad N/T/U+1/V"),
             (dict(blank=-1), ARG, "blank -1 outside"), (dict(blank=7), ARG, "blank 7 outside"),
             (dict(N=2 ** 20, T=2 ** 10, U1=2 ** 10), ARG, "rows outside"), (dict(T=2 ** 20, U1=2 ** 10), ARG, "T * (U + 1) >"),
             (dict(ws=NOWHERE + 8), ARG, "16-byte aligned"), (dict(ws=NOWHERE + 4), ARG, "16-byte aligned"),
             (dict(ws_bytes=100), WORKSPACE, "workspace too small")]
    if "grad" in fn:
        cases.append((dict(weight=False), ARG, "null argument"))
    if fn.endswith("_logits"):
        cases += [(dict(dtype=3), ARG, "dtype must be"), (dict(dtype=-1), ARG, "dtype must be")]
    for kw, want, msg in cases:
        rc, text = _call(core, fn, **kw)
        assert rc == want and msg in text, (kw, rc, text)
    rc, text = _call(core, fn, U1=1024, V=8192, ws_bytes=100)       # the largest shapes the build takes are refused only for their workspace
    assert rc == WORKSPACE, text


def test_workspace_formula(core):
    al = lambda n: (n + 255) // 256 * 256
    for N, T, U1, V in ((1, 1, 1, 1), (3, 7, 5, 9), (16, 250, 51, 1024), (2, 1027, 1024, 9), (2, 9, 4, 8192)):
        R = N * T * U1
        utt = 8 * N + 4 * (4 * N + 1)
        assert core._lib.crf_ctct_workspace_bytes(N, T, U1, V) == al(16 * R) + al(4 * R) + al(16 * R) + al(16 * R) + al(utt), (N, T, U1, V)
        secs = core.debug_ctct_ws_sections(N, T, U1, V)
        assert [s[0] for s in secs] == ["row", "rmax", "alpha", "beta", "utt"] and [s[2] for s in secs] == [16 * R, 4 * R, 16 * R, 16 * R, utt]
        assert secs[0][1] == 0 and all(b[1] == al(a[1] + a[2]) for a, b in zip(secs, secs[1:]))
    core.debug_set("ws_gap", 2)
    try:
        assert core._lib.crf_ctct_workspace_bytes(3, 7, 5, 9) == al(16 * 105) * 3 + al(4 * 105) + al(8 * 3 + 4 * 13) + 5 * 512
    finally:
        core.debug_set("ws_gap", None)
    for bad in ((0, 1, 1, 1), (1, 1, 1025, 1), (1, 1, 1, 8193), (1, 0, 1, 1)):
        assert core._lib.crf_ctct_workspace_bytes(*bad) == -1


def test_bad_arguments_raise_value_error_before_any_device_call():
    import ctc_crf
    x = torch.zeros((2, 5, 4, 7))
    labels = torch.ones((2, 3), dtype=torch.int32)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)
    ok = (i32(5, 5), i32(3, 3))
    wide = torch.zeros((2, 5, 4, 14))[..., ::2]                      # the right shape, every second element
    cases = (((x, labels, i32(5, 6), i32(3, 3)), {}, r"frames_lengths must lie in \[1, T=5\]"),
             ((x, labels, i32(0, 5), i32(3, 3)), {}, r"frames_lengths must lie in \[1, T=5\]"),
             ((x, labels, i32(5, 5), i32(4, 3)), {}, r"labels_lengths must lie in \[0, U=3\]"),
             ((x, labels, i32(5, 5), i32(3, -1)), {}, r"labels_lengths must lie in \[0, U=3\]"),
             ((x, labels, *ok), dict(reduction="avg"), "unknown reduction"),
             ((x.double(), labels, *ok), {}, "float32 log_probs"),
             ((x.double(), labels, *ok), dict(fuse_log_softmax=True), "float32, bfloat16 or float16"),
             ((x, labels.long(), *ok), {}, "must be int32"),
             ((x, labels, ok[0].long(), ok[1]), {}, "must be int32"),
             ((x, labels[:, :2], *ok), {}, r"labels \(N=2, U=3\)"),
             ((x, labels, i32(5, 5, 5), i32(3, 3, 3)), {}, r"\(N=3, T, U\+1, V\)"),
             ((x[0], labels, *ok), {}, r"\(N=2, T, U\+1, V\)"),
             ((x, labels, i32(5, 5), i32(3)), {}, r"as \(N,\)"),
             ((x, labels, *ok), dict(blank=7), r"blank must lie in \[0, V-1=6\]"),
             ((x, labels, *ok), dict(blank=-1), r"blank must lie in \[0, V-1=6\]"),
             ((wide, labels, *ok), {}, "must be contiguous"),
             ((x, torch.ones((2, 6), dtype=torch.int32)[:, ::2], *ok), {}, "must be contiguous"),
             ((torch.zeros((1, 2, 1025, 2)), torch.ones((1, 1024), dtype=torch.int32), i32(2), i32(1024)), {}, "U = 1024 > 1023"),
             ((torch.zeros((1, 1, 1, 8193)), torch.ones((1, 0), dtype=torch.int32), i32(1), i32(0)), {}, r"V = 8193 outside"))
    for args, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ctc_crf.ctct_loss(*args, **kw)
    with pytest.raises(RuntimeError, match="must be on the GPU"):    # everything else in order: only then is a device asked for
        ctc_crf.ctct_loss(x, labels, *ok)
