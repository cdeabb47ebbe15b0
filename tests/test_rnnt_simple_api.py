"""CPU tests (no device) of rnnt_loss_simple: the surface -- the signature, the warp_rnnt shim, the exports, ValueError for every mismatch
of the inputs and for bad lengths given on the CPU, the argument errors of the C calls (answered before any HIP call, so device pointers
that point nowhere do), the workspace formula and its bound (nothing proportional to T (U + 1) V) -- and the yardstick of
tests/rnnt_simple_ref.py against the enumeration of every alignment and against torch autograd through the joint tensor."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import rnnt_ref, rnnt_simple_ref

SYMBOLS = ("crf_rnnt_simple_workspace_bytes", "crf_rnnt_simple_loss", "crf_rnnt_simple_grad", "crf_debug_rnnt_simple_ws_sections",
           "crf_debug_rnnt_simple_ws_section_names")
NOWHERE = 0x1000             # a non-null, 16-byte aligned "device pointer": never dereferenced by a call that is refused
ARG, WORKSPACE, UNSUPPORTED = 3, 5, 6
EPS = 1e-10


@pytest.fixture(scope="module")
def core():
    import ctc_crf
    return ctc_crf._C


def test_signature_defaults_exports_and_shim(core):
    import ctc_crf
    import cat_amd.ctc_crf
    import warp_rnnt
    from warp_rnnt import rnnt_loss_simple
    lib = ctypes.CDLL(core.LIB_PATH)
    hdr = open(core.LIB_PATH.rsplit("/cat_amd/", 1)[0] + "/include/ctc_crf_hip.h").read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in core.EXPORTED_SYMBOLS and s + "(" in hdr, s
    assert warp_rnnt.rnnt_loss_simple is ctc_crf.rnnt_loss_simple and rnnt_loss_simple is cat_amd.ctc_crf.rnnt_loss_simple
    assert warp_rnnt.rnnt_loss is ctc_crf.rnnt_loss
    par = inspect.signature(ctc_crf.rnnt_loss_simple).parameters
    assert list(par) == ["f_enc", "g_pred", "labels", "frames_lengths", "labels_lengths", "average_frames", "reduction", "blank", "return_invalid"]
    assert all(par[k].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD and par[k].default is inspect.Parameter.empty for k in list(par)[:5])
    assert [par[k].default for k in list(par)[5:]] == [False, None, 0, False]
    assert "rnnt_loss_simple" in ctc_crf.rnnt_loss.__doc__ and "rnnt_loss_simple" in warp_rnnt.__doc__


def _inputs(N=2, T=5, U=3, V=7, dtype=torch.float32):
    f, g = torch.zeros(N, T, V, dtype=dtype), torch.zeros(N, U + 1, V, dtype=dtype)
    return f, g, torch.ones(N, U, dtype=torch.int32), torch.full((N,), T, dtype=torch.int32), torch.full((N,), U, dtype=torch.int32)


def test_mismatched_and_non_contiguous_inputs_raise_value_error():
    import ctc_crf
    f, g, lab, lx, ly = _inputs()
    bad = [(f, g.half()), (f.double(), g.double()), (f, torch.zeros(2, 4, 8)), (f, torch.zeros(3, 4, 7)),
           (f.transpose(0, 1).contiguous().transpose(0, 1), g), (f, torch.zeros(2, 4, 14)[:, :, ::2]), (f[0], g[0])]
    for a, b in bad:
        with pytest.raises(ValueError):
            ctc_crf.rnnt_loss_simple(a, b, lab, lx, ly)
    with pytest.raises(ValueError):
        ctc_crf.rnnt_loss_simple(f, g, lab[:, :2], lx, ly)          # labels are not (N, U)
    with pytest.raises(ValueError):
        ctc_crf.rnnt_loss_simple(f, g, lab, lx, ly, blank=7)
    with pytest.raises(ValueError):
        ctc_crf.rnnt_loss_simple(f, g, lab, lx, ly, reduction="max")
    with pytest.raises(RuntimeError, match="GPU"):                   # every host check passes: there is no CPU path
        ctc_crf.rnnt_loss_simple(f, g, lab, lx, ly)


def test_bad_lengths_on_the_cpu_and_long_label_sequences_raise_value_error():
    import ctc_crf
    f, g, lab, lx, ly = _inputs()
    for blx, bly in (([5, 0], [3, 3]), ([5, 6], [3, 3]), ([5, 5], [3, 4]), ([5, 5], [-1, 3])):
        with pytest.raises(ValueError):
            ctc_crf.rnnt_loss_simple(f, g, lab, torch.tensor(blx, dtype=torch.int32), torch.tensor(bly, dtype=torch.int32))
    with pytest.raises(ValueError):
        ctc_crf.rnnt_loss_simple(f, g, lab, lx[:1], ly[:1])
    f, g, lab, lx, ly = _inputs(N=1, T=2, U=1024, V=3)
    with pytest.raises(ValueError, match="1023"):
        ctc_crf.rnnt_loss_simple(f, g, lab, lx, ly)
    f, g, lab, lx, ly = _inputs(N=1, T=2, U=1, V=8193)
    with pytest.raises(ValueError, match="8192"):
        ctc_crf.rnnt_loss_simple(f, g, lab, lx, ly)


def test_workspace_formula_and_bound(core):
    al = lambda n: (n + 255) // 256 * 256
    for N, T, U1, V in ((1, 1, 1, 1), (3, 7, 5, 9), (64, 250, 51, 5000), (2, 64, 32, 1024), (1, 3, 1024, 8192), (5, 2000, 1, 1)):
        got = core._lib.crf_rnnt_simple_workspace_bytes(N, T, U1, V)
        base = core._lib.crf_rnnt_workspace_bytes(N, T, U1, V, -1)
        assert got == base + al(4 * N * T * V) + al(16 * N * U1 * V), (N, T, U1, V)
        assert got <= base + 16 * N * (T + U1) * V + 65536, (N, T, U1, V)
        secs = core.debug_rnnt_simple_ws_sections(N, T, U1, V)
        assert [s[0] for s in secs] == ["row", "alpha", "beta", "utt", "df", "dg"]
        assert secs[:4] == core.debug_rnnt_ws_sections(N, T, U1, V, -1) and [s[2] for s in secs[4:]] == [4 * N * T * V, 16 * N * U1 * V]
        assert all(b[1] == al(a[1] + a[2]) for a, b in zip(secs, secs[1:])) and al(secs[-1][1] + secs[-1][2]) == got
    core.debug_set("ws_gap", 2)
    try:
        assert core._lib.crf_rnnt_simple_workspace_bytes(3, 7, 5, 9) == core._lib.crf_rnnt_workspace_bytes(3, 7, 5, 9, -1) + al(4 * 189) + al(16 * 135) + 2 * 512
    finally:
        core.debug_set("ws_gap", None)
    for bad in ((0, 1, 1, 1), (1, 1, 1025, 1), (1, 1, 1, 8193), (1, 0, 1, 1)):
        assert core._lib.crf_rnnt_simple_workspace_bytes(*bad) == -1


def _call(core, fn, f=True, g=True, labels=True, lx=True, ly=True, out=True, weight=True, ws=NOWHERE, dtype=0, blank=0, N=2, T=5, U1=4, V=7,
          ws_bytes=None):
    vp = ctypes.c_void_p
    p = lambda on: vp(NOWHERE if on else 0)
    if ws_bytes is None:
        ws_bytes = max(core._lib.crf_rnnt_simple_workspace_bytes(N, T, U1, V), 0)
    mid = (p(f), p(g), dtype, blank, p(labels), p(lx), p(ly), N, T, U1, V)
    tail = (p(weight), p(out), p(out)) if fn.endswith("grad") else (p(out), vp(0))
    rc = getattr(core._lib, fn)(*mid, *tail, vp(ws), ws_bytes, vp(0))
    return rc, core._lib.crf_last_error().decode()


@pytest.mark.parametrize("fn", ["crf_rnnt_simple_loss", "crf_rnnt_simple_grad"])
def test_every_argument_error_is_answered_before_any_hip_call(core, fn):
    cases = [(dict(f=False), ARG, "null argument"), (dict(g=False), ARG, "null argument"), (dict(labels=False), ARG, "null argument"),
             (dict(lx=False), ARG, "null argument"), (dict(ly=False), ARG, "null argument"), (dict(ws=0), ARG, "null argument"),
             (dict(dtype=3), ARG, "dtype must be"), (dict(dtype=-1), ARG, "dtype must be"),
             (dict(U1=1025), UNSUPPORTED, "U > 1023"), (dict(V=8193), UNSUPPORTED, "V > 8192"),
             (dict(N=0), ARG, "bad N/T/U+1/V"), (dict(T=0), ARG, "bad N/T/U+1/V"), (dict(U1=0), ARG, "bad N/T/U+1/V"), (dict(V=0), ARG, "bad N/T/U+1/V"),
             (dict(blank=-1), ARG, "blank -1 outside"), (dict(blank=7), ARG, "blank 7 outside"),
             (dict(N=2 ** 20, T=2 ** 10, U1=2 ** 10), ARG, "rows outside"),
             (dict(ws=NOWHERE + 8), ARG, "16-byte aligned"), (dict(ws_bytes=100), WORKSPACE, "workspace too small")]
    cases.append((dict(weight=False), ARG, "null argument") if fn.endswith("grad") else (dict(out=False), ARG, "null argument"))
    for kw, want, msg in cases:
        rc, text = _call(core, fn, **kw)
        assert rc == want and msg in text, (kw, rc, text)
    rc, text = _call(core, fn, U1=1024, V=8192, ws_bytes=100)        # the largest shapes the build takes are refused only for their workspace
    assert rc == WORKSPACE, text


# ---- the yardstick ----
@pytest.mark.parametrize("T,U,V,blank", [(1, 0, 2, 0), (1, 1, 3, 2), (2, 0, 2, 1), (3, 2, 4, 0), (4, 3, 5, 3), (2, 3, 3, 1), (4, 1, 2, 0)])
def test_the_yardstick_equals_the_enumeration_of_every_alignment(T, U, V, blank):
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(T * 10 + U, [T], [U], V, blank)
    costs, df, dg = rnnt_simple_ref.batch_ref(f, g, labels, lx, ly, blank)
    joint = f[0].astype(np.float64)[:, None, :] + g[0].astype(np.float64)[None, :, :]
    want = rnnt_ref.brute_force(rnnt_ref.log_softmax(joint), labels[0], blank)
    assert abs(costs[0] - want) <= EPS * max(1.0, abs(want))
    assert df.shape == f.shape and dg.shape == g.shape
    assert np.abs(df.sum(-1)).max() <= EPS and np.abs(dg.sum(-1)).max() <= EPS      # log_softmax's backward: every row sums to 0


@pytest.mark.parametrize("T_n,U_n,V,blank", [([4, 2], [3, 1], 5, 3), ([7, 3, 1], [5, 0, 0], 6, 0)])
def test_the_yardsticks_gradients_equal_autograd_through_the_joint_tensor(T_n, U_n, V, blank):
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(len(T_n) + V, T_n, U_n, V, blank)
    costs, df, dg = rnnt_simple_ref.batch_ref(f, g, labels, lx, ly, blank)
    assert not df[0, T_n[0]:].any() and not dg[-1, U_n[-1] + 1:].any()
    for n, (t, u) in enumerate(zip(lx, ly)):
        lf = torch.tensor(f[n, :t].astype(np.float64), requires_grad=True)
        lg = torch.tensor(g[n, :u + 1].astype(np.float64), requires_grad=True)
        joint = lf[:, None, :] + lg[None, :, :]
        tc, leaf = rnnt_ref.torch_cost(joint.detach().numpy(), labels[n, :u], blank, normalise=True)
        tc.backward()
        joint.backward(leaf.grad)
        assert abs(float(tc.detach()) - costs[n]) <= EPS * max(1.0, abs(costs[n]))
        assert np.abs(lf.grad.numpy() - df[n, :t]).max() <= EPS and np.abs(lg.grad.numpy() - dg[n, :u + 1]).max() <= EPS
