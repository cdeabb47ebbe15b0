"""GPU tests: ctc_crf.rnnt_loss (crf_rnnt_loss / crf_rnnt_grad, cat_amd/csrc/k_rnnt.hip) against the fp64 yardstick of tests/rnnt_ref.py.

Tolerances are the project's own (tests/score_grad_ref.py, tests/test_gpu_ctc_score_grad_logits.py): the cost within TOL = 1e-4 relative;
an fp32 gradient within TOL * max |ref|; a 16-bit gradient within 2^-8 |ref| + TOL * max |ref| entry by entry -- one rounding of the result
to 8 (bf16) or 11 (fp16) bits is 2^-9 relative, one more for the fp32 arithmetic in front -- against the reference evaluated on the
quantised input, so that the input's own rounding is no part of the error."""
import numpy as np
import pytest
import torch

from tests import rnnt_ref
from tests.score_grad_ref import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ("normalised", "float32", "bfloat16", "float16")
SENT = 768.0                 # (exact in bf16 and fp16)
SHAPES = [(1, 1), (1, 2), (2, 1), (5, 4), (64, 64), (65, 65), (3, 129), (130, 70)]        # (T, U + 1)
RAGGED_T, RAGGED_U = (130, 129, 65, 64, 1), (69, 64, 63, 0, 0)


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


def i32(a, dev=DEV):
    return torch.tensor(np.asarray(a).reshape(-1), dtype=torch.int32, device=dev)


def prepare(x, kind):
    """Raw fp32 numpy joiner output -> (the input tensor of that kind on the CPU, its exact fp64 values, fused)."""
    if kind == "normalised":
        t = torch.log_softmax(torch.from_numpy(x).double(), -1).float()
        return t, t.double().numpy(), False
    t = torch.from_numpy(x).to(getattr(torch, kind))
    return t, t.double().numpy(), True


def run(crf, t, labels, lx, ly, blank, fused, compact=False, weights=None, lengths_on=DEV):
    """One forward and backward through the C calls' Python wrappers, the gradient written over a sentinel.  t, labels: CPU tensors in the
    layout asked for.  -> (costs [N] fp64, invalid [N], grad fp64 numpy in t's shape)."""
    core = crf._C
    N = len(lx)
    costs, invalid, call = core.rnnt_loss_fwd(t.to(DEV), labels.to(DEV), i32(lx, lengths_on), i32(ly, lengths_on), blank, compact, fused)
    w = torch.ones(N, device=DEV) if weights is None else torch.tensor(weights, dtype=torch.float32, device=DEV)
    out = torch.full(t.shape, SENT, dtype=t.dtype, device=DEV)
    grad = core.rnnt_loss_bwd(call, w, grad_out=out)
    torch.cuda.synchronize()
    g = grad.double().cpu().numpy()
    assert not np.any(g == SENT), "an element of the gradient was not written"
    return costs.double().cpu().numpy(), invalid.cpu().numpy(), g


def check(kind, costs, grad, rc, rg, what=""):
    print(what, kind, "cost err", float(np.max(np.abs(costs - rc) / np.maximum(np.abs(rc), 1e-30))), "grad err", float(np.abs(grad - rg).max()),
          "max |ref|", float(np.abs(rg).max()))
    assert np.all(np.abs(costs - rc) <= TOL * np.abs(rc)), (what, kind, costs, rc)
    top = np.abs(rg).max()
    if kind in ("normalised", "float32"):
        assert np.abs(grad - rg).max() <= TOL * top, (what, kind, np.abs(grad - rg).max(), top)
    else:
        over = np.abs(grad - rg) - (2.0 ** -8 * np.abs(rg) + TOL * top)
        assert over.max() <= 0.0, (what, kind, over.max(), top)


def one_case(crf, seed, T_n, U_n, V, blank, kind, T=None, U1=None):
    x, labels, lx, ly = rnnt_ref.random_case(seed, T_n, U_n, V, blank, T, U1)
    t, exact, fused = prepare(x, kind)
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), lx, ly, blank, fused)
    assert not invalid.any()
    check(kind, costs, grad, rc, rg, (T_n, U_n, V, blank))
    live = np.zeros(grad.shape[:3], dtype=bool)
    for n, (a, b) in enumerate(zip(lx, ly)):
        live[n, :a, :b + 1] = True
    assert not grad[~live].any(), "a padding element of the gradient is not zero"
    return costs, grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,U1", SHAPES)
def test_every_lattice_shape(crf, T, U1, kind):
    one_case(crf, 100 * T + U1, [T], [U1 - 1], 9, 3, kind)
    if (T, U1) == (5, 4):                                            # ... and inside a padded tensor larger than the lattice
        one_case(crf, 7, [T], [U1 - 1], 9, 3, kind, T=8, U1=7)


@pytest.mark.parametrize("V,blank", [(2, 0), (2, 1), (9, 0), (9, 3), (9, 8), (65, 0), (65, 3), (65, 64), (4097, 0), (4097, 3), (4097, 4096)])
def test_every_vocabulary_and_blank(crf, V, blank):
    for kind in KINDS:
        one_case(crf, V + blank, [5, 3], [3, 2], V, blank, kind)


def test_the_long_case_at_the_widest_row(crf):
    """(130, 70) at V = 4097: log-domain values of about 1 600 at the far corner, where fp32 recursions lose the gradient's fourth digit."""
    one_case(crf, 1, [130], [69], 4097, 4096, "float32")


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch_padded_and_compact(crf, kind):
    """One call over utterances of every size class; the same bits for an utterance alone, inside the batch, and in the compact layout."""
    V, blank = 9, 3
    x, labels, lx, ly = rnnt_ref.random_case(31, RAGGED_T, RAGGED_U, V, blank)
    t, exact, fused = prepare(x, kind)
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    lab_t = torch.from_numpy(labels)
    costs, invalid, grad = run(crf, t, lab_t, lx, ly, blank, fused)
    assert not invalid.any()
    check(kind, costs, grad, rc, rg, "padded")
    live = np.zeros(grad.shape[:3], dtype=bool)
    for n, (a, b) in enumerate(zip(lx, ly)):
        live[n, :a, :b + 1] = True
    assert not grad[~live].any(), "a padding element of the gradient is not zero"
    ct, cl = rnnt_ref.to_compact(t, lab_t, lx, ly)
    for where in (DEV, "cpu"):                                       # lengths on the device (bounds only) and on the host (exact maxima)
        ccosts, cinv, cgrad = run(crf, ct, cl, lx, ly, blank, fused, compact=True, lengths_on=where)
        assert not cinv.any() and np.array_equal(ccosts, costs), (where, ccosts, costs)
        assert np.array_equal(cgrad, rnnt_ref.to_compact(grad, labels, lx, ly)[0]), where
    for n in (0, 2, 4):                                              # alone, cut to its own size
        a, b = lx[n], ly[n]
        acosts, _, agrad = run(crf, t[n:n + 1, :a, :b + 1].contiguous(), lab_t[n:n + 1, :b].contiguous(), [a], [b], blank, fused)
        assert acosts[0] == costs[n] and np.array_equal(agrad[0], grad[n, :a, :b + 1]), n


@pytest.mark.parametrize("kind", ("normalised", "float32", "bfloat16"))
def test_minus_infinity_entries(crf, kind):
    V, blank = 6, 0
    x, labels, lx, ly = rnnt_ref.random_case(5, [6, 6, 6], [4, 4, 4], V, blank)
    t, _, fused = prepare(x, kind)
    t[0, 5, 4, blank] = -np.inf                                      # utterance 0: the final blank -- every path
    t[1, 0, 0, blank] = -np.inf                                      # utterance 1: the first blank -- some paths
    t[1, 2, 1, labels[1, 1]] = -np.inf
    if fused:
        t[2, 3, 2, :] = -np.inf                                      # utterance 2: a whole row of the raw output
    exact = t.double().numpy()
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    assert rc[0] == np.inf and np.isfinite(rc[1:]).all()
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), lx, ly, blank, fused)
    assert not invalid.any() and costs[0] == np.inf and not grad[0].any()
    assert np.isfinite(grad).all() and np.isfinite(costs[1:]).all()
    check(kind, costs[1:], grad[1:], rc[1:], rg[1:], "-inf")


@pytest.mark.parametrize("kind", ("normalised", "bfloat16"))
def test_invalid_utterances_beside_valid_ones(crf, kind):
    """T_n outside [1, T], U_n outside [0, U], a label outside [0, V), a label equal to the blank: decided on the device."""
    V, blank, T, U = 7, 2, 6, 3
    x, labels, _, _ = rnnt_ref.random_case(9, [T] * 8, [U] * 8, V, blank)
    lx = [6, 0, 7, 5, 4, 6, 6, 3]
    ly = [3, 2, 3, 4, -1, 3, 2, 0]
    labels[5, 1] = V                                                 # utterance 5: a label outside [0, V)
    labels[6, 0] = blank                                             # utterance 6: the blank as a label
    labels[7, 0] = -1                                                # (behind utterance 7's length: never read)
    bad = [False, True, True, True, True, True, True, False]
    t, exact, fused = prepare(x, kind)
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), lx, ly, blank, fused)
    assert invalid.tolist() == [int(b) for b in bad]
    good = [n for n, b in enumerate(bad) if not b]
    for n, b in enumerate(bad):
        if b:
            assert costs[n] == np.inf and not grad[n].any(), n
    rc, rg = rnnt_ref.batch_ref(exact[good], labels[good], [lx[n] for n in good], [ly[n] for n in good], blank, fused)
    check(kind, costs[good], grad[good], rc, rg, "beside invalid")
    with pytest.raises(ValueError):                                  # the same lengths on the CPU are refused up front
        crf.rnnt_loss(t.to(DEV), torch.from_numpy(labels).to(DEV), i32(lx, "cpu"), i32(ly, "cpu"), blank=blank, fuse_log_softmax=fused)
    # compact: label errors keep the utterance's rows; lengths out of range claim none
    glx, gly = [6, 6, 3], [3, 2, 0]
    ct, cl = rnnt_ref.to_compact(t[[0, 6, 7]], torch.from_numpy(labels[[0, 6, 7]]), glx, gly)
    ccosts, cinv, cgrad = run(crf, ct, cl, [6, 0, 6, 3], [3, 1, 2, 0], blank, fused, compact=True)
    assert cinv.tolist() == [0, 1, 1, 0] and ccosts[1] == np.inf and ccosts[2] == np.inf
    assert ccosts[0] == costs[0] and ccosts[3] == costs[7]
    want = rnnt_ref.to_compact(grad[[0, 6, 7]], labels[[0, 6, 7]], glx, gly)[0]
    assert np.array_equal(cgrad, want)


@pytest.mark.parametrize("fused", (False, True))
def test_reductions_average_frames_and_grad_output(crf, fused):
    V, blank = 11, 10
    x, labels, lx, ly = rnnt_ref.random_case(3, [9, 7, 4], [5, 2, 0], V, blank)
    t, exact, _ = prepare(x, "float32" if fused else "normalised")
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    lab = torch.from_numpy(labels).to(DEV)
    frames = np.asarray(lx, dtype=np.float64)
    w = np.asarray([0.5, -2.0, 3.0])
    plans = [(dict(), w, rc), (dict(reduction="none"), w, rc), (dict(reduction="sum"), np.ones(3), rc.sum()),
             (dict(reduction="mean"), np.ones(3) / 3, rc.mean()), (dict(average_frames=True), w / frames, rc / frames),
             (dict(average_frames=True, reduction="mean"), 1 / frames / 3, (rc / frames).mean())]
    for lengths_on in (DEV, "cpu"):
        for kw, scale, want in plans:
            leaf = t.to(DEV).requires_grad_(True)
            out = crf.rnnt_loss(leaf, lab, i32(lx, lengths_on), i32(ly, lengths_on), blank=blank, fuse_log_softmax=fused, **kw)
            assert np.allclose(out.detach().double().cpu().numpy(), want, rtol=TOL, atol=0), kw
            (out * torch.tensor(w, dtype=torch.float32, device=DEV)).sum().backward() if out.dim() else out.backward()
            ref = rg * scale[:, None, None, None]
            assert leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape
            assert np.abs(leaf.grad.double().cpu().numpy() - ref).max() <= TOL * np.abs(ref).max(), kw
    costs, invalid = crf.rnnt_loss(t.to(DEV), lab, i32(lx), i32(ly), blank=blank, fuse_log_softmax=fused, return_invalid=True)
    assert costs.shape == (3,) and invalid.dtype == torch.int32 and not invalid.any()


def test_no_host_synchronisation_with_the_lengths_on_the_device(crf):
    V, blank = 9, 0
    x, labels, lx, ly = rnnt_ref.random_case(4, [12, 9], [6, 3], V, blank)
    t = torch.from_numpy(x).to(torch.bfloat16).to(DEV)
    lab, lxd, lyd = torch.from_numpy(labels).to(DEV), i32(lx), i32(ly)
    ct, cl = rnnt_ref.to_compact(t, lab, lx, ly)
    leaf, cleaf = t.clone().requires_grad_(True), ct.clone().requires_grad_(True)
    norm = torch.log_softmax(t.float(), -1).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                            # the positive control: this build enforces the mode
            torch.ones(1, device=DEV).item()
        a = crf.rnnt_loss(leaf, lab, lxd, lyd, blank=blank, fuse_log_softmax=True, reduction="mean", average_frames=True)
        a.backward()
        b = crf.rnnt_loss(cleaf, cl, lxd, lyd, blank=blank, fuse_log_softmax=True, compact=True, reduction="sum")
        b.backward()
        c = crf.rnnt_loss(norm, lab, lxd, lyd, blank=blank)
        c.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(leaf.grad).all()) and bool(torch.isfinite(cleaf.grad).all()) and bool(torch.isfinite(norm.grad).all())
    assert np.isfinite(float(a.detach())) and np.isfinite(float(b.detach()))
