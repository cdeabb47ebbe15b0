"""CPU tests (no device) of the RNN-T loss: the yardstick of tests/rnnt_ref.py held to itself -- the numpy recursion with its closed-form
gradients against torch autograd and against the enumeration of every alignment, to 1e-10 -- and the surface: the exports, the warp_rnnt
shim, every argument error of the C calls (answered before any HIP call, so device pointers that point nowhere do), the workspace
formula, and ValueError for bad lengths given on the CPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import rnnt_ref

SYMBOLS = ("crf_rnnt_workspace_bytes", "crf_rnnt_loss", "crf_rnnt_loss_logits", "crf_rnnt_grad", "crf_rnnt_grad_logits",
           "crf_debug_rnnt_ws_sections", "crf_debug_rnnt_ws_section_names")
NOWHERE = 0x1000             # a non-null, 16-byte aligned "device pointer": never dereferenced by a call that is refused
ARG, WORKSPACE, UNSUPPORTED = 3, 5, 6
EPS = 1e-10


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


# ---- the yardstick ----
def _rand(seed, T, U, V, blank):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, U + 1, V)) * 2.0
    labels = rng.integers(0, V - 1, U)
    return x, labels + (labels >= blank)


@pytest.mark.parametrize("T,U,V,blank", [(1, 0, 2, 0), (1, 1, 3, 2), (2, 0, 2, 1), (3, 2, 4, 0), (4, 3, 5, 3), (2, 3, 3, 1), (4, 1, 2, 0)])
def test_recursion_equals_the_enumeration_of_every_alignment(T, U, V, blank):
    x, labels = _rand(T * 10 + U, T, U, V, blank)
    lp = rnnt_ref.log_softmax(x)
    for inp in (lp, x):                                             # (nothing in the recursion needs a normalised input)
        cost, _ = rnnt_ref.ref_normalised(inp, labels, blank)
        assert abs(cost - rnnt_ref.brute_force(inp, labels, blank)) <= EPS * max(1.0, abs(cost))
    assert abs(rnnt_ref.ref_logits(x, labels, blank)[0] - rnnt_ref.brute_force(lp, labels, blank)) <= EPS * max(1.0, abs(cost))


@pytest.mark.parametrize("T,U,V,blank", [(1, 0, 2, 0), (1, 1, 3, 2), (2, 0, 2, 1), (4, 3, 5, 3), (7, 5, 6, 0), (12, 9, 4, 2)])
def test_closed_form_gradients_equal_autograd(T, U, V, blank):
    x, labels = _rand(T * 7 + U, T, U, V, blank)
    cost, grad = rnnt_ref.ref_logits(x, labels, blank)
    tc, leaf = rnnt_ref.torch_cost(x, labels, blank, normalise=True)
    tc.backward()
    assert abs(cost - float(tc.detach())) <= EPS * max(1.0, abs(cost))
    assert np.max(np.abs(grad - leaf.grad.numpy())) <= EPS
    lp = rnnt_ref.log_softmax(x)
    cost, grad = rnnt_ref.ref_normalised(lp, labels, blank)
    tc, leaf = rnnt_ref.torch_cost(lp, labels, blank, normalise=False)
    tc.backward()
    assert abs(cost - float(tc.detach())) <= EPS * max(1.0, abs(cost))
    assert np.max(np.abs(grad - leaf.grad.numpy())) <= EPS
    nz = np.zeros_like(grad, dtype=bool)                             # zero except at the blank's column and at labels[u] of node (t, u)
    nz[:, :, blank] = True
    for u in range(U):
        nz[:, u, labels[u]] = True
    assert not grad[~nz].any()


def test_minus_infinity_entries():
    x, labels = _rand(5, 3, 2, 4, 0)
    lp = rnnt_ref.log_softmax(x)
    cut = lp.copy()
    cut[2, 2, 0] = -np.inf                                           # the final blank: every path
    cost, grad = rnnt_ref.ref_normalised(cut, labels, 0)
    assert cost == np.inf and not grad.any() and rnnt_ref.brute_force(cut, labels, 0) == np.inf
    some = lp.copy()
    some[0, 0, 0] = -np.inf                                          # the first blank: only the paths that start with it
    cost, grad = rnnt_ref.ref_normalised(some, labels, 0)
    assert np.isfinite(cost) and np.isfinite(grad).all() and cost > rnnt_ref.ref_normalised(lp, labels, 0)[0]
    assert abs(cost - rnnt_ref.brute_force(some, labels, 0)) <= EPS * cost
    raw = x.copy()
    raw[1, 1, :] = -np.inf                                           # a whole row of the raw output: log_softmax has no value there
    cost, grad = rnnt_ref.ref_logits(raw, labels, 0)
    assert np.isfinite(cost) and np.isfinite(grad).all() and not grad[1, 1].any()


def _same_by_diagonals(lp, labels, blank, logits=False):
    """ref_normalised / ref_logits node by node (`lattice`) and by anti-diagonals (`lattice_diag`): the cost within 1e-12 relative, the
    gradient within 1e-12 absolute.  -> (cost, grad) of the diagonal form."""
    ref = rnnt_ref.ref_logits if logits else rnnt_ref.ref_normalised
    cost, grad = ref(lp, labels, blank, diag=False)
    dcost, dgrad = ref(lp, labels, blank, diag=True)
    assert dcost == cost if np.isinf(cost) else abs(dcost - cost) <= 1e-12 * abs(cost), (cost, dcost)
    assert np.isfinite(dgrad).all() and np.max(np.abs(dgrad - grad)) <= 1e-12
    return dcost, dgrad


@pytest.mark.parametrize("T,U1", [(1, 1), (1, 5), (5, 1), (7, 5), (70, 33)])
def test_the_recursion_by_anti_diagonals_equals_the_one_node_by_node(T, U1):
    x, labels = _rand(T * 100 + U1, T, U1 - 1, 5, 2)
    _same_by_diagonals(rnnt_ref.log_softmax(x), labels, 2)
    _same_by_diagonals(x, labels, 2, logits=True)
    lb, ll = x[:, :, 2], x[:, :U1 - 1, 0]                            # the two functions themselves, on numbers nothing normalised
    (cost, g_lb, g_ll), (dcost, dg_lb, dg_ll) = rnnt_ref.lattice(lb, ll), rnnt_ref.lattice_diag(lb, ll)
    assert abs(dcost - cost) <= 1e-12 * abs(cost)
    assert np.max(np.abs(dg_lb - g_lb)) <= 1e-12 and np.max(np.abs(dg_ll - g_ll), initial=0.0) <= 1e-12


def test_the_recursion_by_anti_diagonals_with_minus_infinity_entries():
    x, labels = _rand(5, 3, 2, 4, 0)
    lp = rnnt_ref.log_softmax(x)
    cut = lp.copy()
    cut[2, 2, 0] = -np.inf                                           # the final blank: every path
    cost, grad = _same_by_diagonals(cut, labels, 0)
    assert cost == np.inf and not grad.any()
    some = lp.copy()
    some[0, 0, 0] = -np.inf                                          # the first blank: only the paths that start with it
    cost, _ = _same_by_diagonals(some, labels, 0)
    assert abs(cost - rnnt_ref.brute_force(some, labels, 0)) <= EPS * cost
    raw = x.copy()
    raw[1, 1, :] = -np.inf                                           # a whole row of the raw output
    cost, grad = _same_by_diagonals(raw, labels, 0, logits=True)
    assert np.isfinite(cost) and not grad[1, 1].any()
    x, labels = _rand(6, 7, 5, 4, 1)                                 # no finite path: a column of labels and a frame of blanks cut
    dead = rnnt_ref.log_softmax(x)
    dead[:, 2, labels[2]] = -np.inf
    cost, grad = _same_by_diagonals(dead, labels, 1)
    assert cost == np.inf and not grad.any()
    dead = rnnt_ref.log_softmax(x)
    dead[3, :, 1] = -np.inf
    cost, grad = _same_by_diagonals(dead, labels, 1)
    assert cost == np.inf and not grad.any()


def test_the_reference_goes_by_anti_diagonals_from_a_size_on(monkeypatch):
    """Below DIAG_FROM nodes the node-by-node form, from there on the diagonal one: every size the GPU tests had before keeps its yardstick."""
    assert 130 * 70 < rnnt_ref.DIAG_FROM <= 1000 * 200
    calls = []
    node, diag = rnnt_ref.lattice, rnnt_ref.lattice_diag
    monkeypatch.setattr(rnnt_ref, "lattice", lambda lb, ll: calls.append("node") or node(lb, ll))
    monkeypatch.setattr(rnnt_ref, "lattice_diag", lambda lb, ll: calls.append("diag") or diag(lb, ll))
    z = np.zeros((rnnt_ref.DIAG_FROM // 4, 4, 2))
    rnnt_ref.ref_normalised(z[:-1], [1, 1, 1], 0)
    rnnt_ref.ref_normalised(z, [1, 1, 1], 0)
    assert calls == ["node", "diag"]


# ---- the surface ----
def test_symbols_exported_and_surface(core):
    import ctc_crf
    import cat_amd.ctc_crf
    import warp_rnnt
    from warp_rnnt import rnnt_loss
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = open(core.LIB_PATH.rsplit("/cat_amd/", 1)[0] + "/include/ctc_crf_hip.h").read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in core.EXPORTED_SYMBOLS and s + "(" in hdr, s
    assert warp_rnnt.rnnt_loss is ctc_crf.rnnt_loss and rnnt_loss is cat_amd.ctc_crf.rnnt_loss
    par = inspect.signature(ctc_crf.rnnt_loss).parameters
    assert list(par)[:9] == ["log_probs", "labels", "frames_lengths", "labels_lengths", "average_frames", "reduction", "blank", "compact",
                             "fuse_log_softmax"]
    assert [par[k].default for k in list(par)[4:9]] == [False, None, 0, False, False]
    for word in ("gather", "fastemit_lambda", "rnnt_loss_simple", "decoding"):
        assert word in ctc_crf.rnnt_loss.__doc__, word


def _call(core, fn="crf_rnnt_loss", x=True, labels=True, lx=True, ly=True, out=True, weight=True, ws=NOWHERE, dtype=0, blank=0, N=2, T=5, U1=4,
          V=7, rows=-1, nlab=0, ws_bytes=None):
    vp = ctypes.c_void_p
    p = lambda on: vp(NOWHERE if on else 0)
    if ws_bytes is None:
        ws_bytes = max(core._lib.crf_rnnt_workspace_bytes(N, T, U1, V, rows), 0)
    head = (p(x), dtype) if fn.endswith("_logits") else (p(x),)
    mid = (blank, p(labels), p(lx), p(ly), N, T, U1, V, rows, nlab)
    tail = (p(weight), p(out)) if "grad" in fn else (p(out), vp(0))
    rc = getattr(core._lib, fn)(*head, *mid, *tail, vp(ws), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


@pytest.mark.parametrize("fn", ["crf_rnnt_loss", "crf_rnnt_loss_logits", "crf_rnnt_grad", "crf_rnnt_grad_logits"])
def test_every_argument_error_is_answered_before_any_hip_call(core, fn):
    cases = [(dict(x=False), ARG, "null argument"), (dict(labels=False), ARG, "null argument"), (dict(lx=False), ARG, "null argument"),
             (dict(ly=False), ARG, "null argument"), (dict(out=False), ARG, "null argument"), (dict(ws=0), ARG, "null argument"),
             (dict(U1=1025), UNSUPPORTED, "U > 1023"), (dict(V=8193), UNSUPPORTED, "V > 8192"),
             (dict(N=0), ARG, "bad N/T/U+1/V"), (dict(T=0), ARG, "bad N/T/U+1/V"), (dict(U1=0), ARG, "bad N/T/U+1/V"), (dict(V=0), ARG, "bad N/T/U+1/V"),
             (dict(blank=-1), ARG, "blank -1 outside"), (dict(blank=7), ARG, "blank 7 outside"),
             (dict(rows=0), ARG, "rows outside"), (dict(rows=2 ** 31), ARG, "compact_rows >"), (dict(rows=40, nlab=-1), ARG, "bad compact_labels"),
             (dict(N=2 ** 20, T=2 ** 10, U1=2 ** 10), ARG, "rows outside"),
             (dict(ws=NOWHERE + 8), ARG, "16-byte aligned"), (dict(ws=NOWHERE + 4), ARG, "16-byte aligned"),
             (dict(ws_bytes=100), WORKSPACE, "workspace too small")]
    if "grad" in fn:
        cases.append((dict(weight=False), ARG, "null argument"))
    if fn.endswith("_logits"):
        cases += [(dict(dtype=3), ARG, "dtype must be"), (dict(dtype=-1), ARG, "dtype must be")]
    for kw, want, msg in cases:
        rc, text = _call(core, fn, **kw)
        assert rc == want and msg in text, (kw, rc, text)
    # the largest shapes the build takes are refused only for their workspace
    rc, text = _call(core, fn, U1=1024, V=8192, ws_bytes=100)
    assert rc == WORKSPACE, text


def test_workspace_formula(core):
    al = lambda n: (n + 255) // 256 * 256
    for N, T, U1, V, rows in ((1, 1, 1, 1, -1), (3, 7, 5, 9, -1), (16, 250, 51, 1024, -1), (5, 130, 70, 65, 389 * 37), (2, 9, 4, 8192, 40)):
        R = N * T * U1 if rows < 0 else rows
        want = al(16 * R) + al(8 * R) + al(8 * R) + al(8 * N + 4 * (4 * N + 1))
        assert core._lib.crf_rnnt_workspace_bytes(N, T, U1, V, rows) == want, (N, T, U1, V, rows)
        secs = core.debug_rnnt_ws_sections(N, T, U1, V, rows)
        assert [s[0] for s in secs] == ["row", "alpha", "beta", "utt"] and [s[2] for s in secs] == [16 * R, 8 * R, 8 * R, 8 * N + 4 * (4 * N + 1)]
        assert secs[0][1] == 0 and all(b[1] == al(a[1] + a[2]) for a, b in zip(secs, secs[1:]))
    core.debug_set("ws_gap", 2)
    try:
        assert core._lib.crf_rnnt_workspace_bytes(3, 7, 5, 9, -1) == al(16 * 105) + al(8 * 105) * 2 + al(8 * 3 + 4 * 13) + 4 * 512
    finally:
        core.debug_set("ws_gap", None)
    for bad in ((0, 1, 1, 1, -1), (1, 1, 1025, 1, -1), (1, 1, 1, 8193, -1), (1, 1, 1, 1, 0)):
        assert core._lib.crf_rnnt_workspace_bytes(*bad) == -1


def test_bad_lengths_on_the_cpu_raise_value_error():
    import ctc_crf
    x = torch.zeros((2, 5, 4, 7))
    labels = torch.ones((2, 3), dtype=torch.int32)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)
    for lx, ly, msg in ((i32(5, 6), i32(3, 3), r"frames_lengths must lie in \[1, T=5\]"), (i32(0, 5), i32(3, 3), r"frames_lengths must lie in \[1, T=5\]"),
                        (i32(5, 5), i32(4, 3), r"labels_lengths must lie in \[0, U=3\]"), (i32(5, 5), i32(3, -1), r"labels_lengths must lie in \[0, U=3\]")):
        with pytest.raises(ValueError, match=msg):
            ctc_crf.rnnt_loss(x, labels, lx, ly)
    rows = torch.zeros((5 * 4 + 2 * 1, 7))
    with pytest.raises(ValueError, match=r"the lengths give 23 rows"):
        ctc_crf.rnnt_loss(rows, labels.reshape(-1)[:3], i32(5, 3), i32(3, 0), compact=True)
    with pytest.raises(ValueError, match=r"22 rows and 3 labels, log_probs has 22 and labels 4"):
        ctc_crf.rnnt_loss(rows, labels.reshape(-1)[:4], i32(5, 2), i32(3, 0), compact=True)
    with pytest.raises(ValueError, match=r"frames_lengths must be >= 1"):
        ctc_crf.rnnt_loss(rows, labels.reshape(-1)[:3], i32(5, 0), i32(3, 0), compact=True)
    with pytest.raises(ValueError, match="unknown reduction"):
        ctc_crf.rnnt_loss(x, labels, i32(5, 5), i32(3, 3), reduction="avg")
    for args, msg in (((x.double(), labels, i32(5, 5), i32(3, 3)), "float32 log_probs"), ((x, labels.long(), i32(5, 5), i32(3, 3)), "must be int32"),
                      ((x, labels[:, :2], i32(5, 5), i32(3, 3)), r"labels \(N=2, U=3\)"), ((x, labels, i32(5, 5, 5), i32(3, 3, 3)), r"\(N=3, T, U\+1, V\)"),
                      ((x, labels, i32(5, 5), i32(3, 3), False, None, 7), r"blank must lie in \[0, V-1=6\]"),
                      ((x, labels, i32(5, 5), i32(3, 3)), "must be on the GPU")):
        with pytest.raises(RuntimeError, match=msg):
            ctc_crf.rnnt_loss(*args)
