"""GPU tests: ctc_crf.ctct_loss (crf_ctct_loss / crf_ctct_grad, cat_amd/csrc/k_ctct.hip) against the fp64 yardstick of tests/ctct_ref.py.

Tolerances are the project's own, as tests/test_gpu_rnnt_loss.py states them: the cost within TOL = 1e-4 relative (tests/score_grad_ref.py);
an fp32 gradient within TOL * max |ref|; a 16-bit gradient within 2^-8 |ref| + TOL * max |ref| entry by entry -- one rounding of the result
to 8 (bf16) or 11 (fp16) bits is 2^-9 relative, one more for the fp32 arithmetic in front -- against the reference evaluated on the
quantised input, so that the input's own rounding is no part of the error.  Labels come from small alphabets, so that adjacent equal
labels occur in every case, and T_n >= U_n + repeats unless the case is about a lattice without a path."""
import numpy as np
import pytest
import torch

from tests import ctct_ref
from tests.score_grad_ref import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ("normalised", "float32", "bfloat16", "float16")
SENT = 768.0                 # (exact in bf16 and fp16)
SHAPES = [(1, 1), (1, 2), (2, 2), (5, 4), (70, 64), (70, 65), (140, 129), (1500, 40)]       # (T, U + 1)
RAGGED_T, RAGGED_U = (140, 129, 65, 64, 1), (69, 64, 63, 0, 0)


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


def run(crf, t, labels, lx, ly, blank, fused, weights=None, lengths_on=DEV):
    """One forward and backward through the C calls' Python wrappers, the gradient written over a sentinel.  t, labels: CPU tensors.
    -> (costs [N] fp64, invalid [N], grad fp64 numpy in t's shape)."""
    core = crf._C
    N = len(lx)
    costs, invalid, call = core.ctct_loss_fwd(t.to(DEV), labels.to(DEV), i32(lx, lengths_on), i32(ly, lengths_on), blank, fused)
    w = torch.ones(N, device=DEV) if weights is None else torch.tensor(weights, dtype=torch.float32, device=DEV)
    out = torch.full(t.shape, SENT, dtype=t.dtype, device=DEV)
    grad = core.ctct_loss_bwd(call, w, grad_out=out)
    torch.cuda.synchronize()
    g = grad.double().cpu().numpy()
    assert not np.any(g == SENT), "an element of the gradient was not written"
    return costs.double().cpu().numpy(), invalid.cpu().numpy(), g


def check(kind, costs, grad, rc, rg, what=""):
    """costs / grad against the yardstick's; an utterance the yardstick gives +inf must cost +inf (its gradient, all zeros, is compared
    like any other)."""
    fin = np.isfinite(rc)
    assert np.all(costs[~fin] == np.inf) and np.isfinite(costs[fin]).all() and np.isfinite(grad).all(), (what, kind, costs, rc)
    top = np.abs(rg).max()
    print(what, kind, "cost err", float(np.max(np.abs(costs[fin] - rc[fin]) / np.maximum(np.abs(rc[fin]), 1e-30), initial=0.0)), "grad err",
          float(np.abs(grad - rg).max()), "max |ref|", float(top))
    assert np.all(np.abs(costs[fin] - rc[fin]) <= TOL * np.abs(rc[fin])), (what, kind, costs, rc)
    if kind in ("normalised", "float32"):
        assert np.abs(grad - rg).max() <= TOL * top, (what, kind, np.abs(grad - rg).max(), top)
    else:
        over = np.abs(grad - rg) - (2.0 ** -8 * np.abs(rg) + TOL * top)
        assert over.max() <= 0.0, (what, kind, over.max(), top)


def live_mask(shape, lx, ly):
    live = np.zeros(shape[:3], dtype=bool)
    for n, (a, b) in enumerate(zip(lx, ly)):
        live[n, :a, :b + 1] = True
    return live


def one_case(crf, seed, T_n, U_n, V, blank, kind, T=None, U1=None, labels=None):
    x, drawn, lx, ly = ctct_ref.random_case(seed, T_n, U_n, V, blank, T, U1, feasible=labels is None)
    labels = drawn if labels is None else np.asarray(labels, dtype=np.int32).reshape(drawn.shape)
    t, exact, fused = prepare(x, kind)
    rc, rg = ctct_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), lx, ly, blank, fused)
    assert not invalid.any()
    check(kind, costs, grad, rc, rg, (T_n, U_n, V, blank))
    assert not grad[~live_mask(grad.shape, lx, ly)].any(), "a padding element of the gradient is not zero"
    return costs, grad, rc


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,U1", SHAPES)
def test_every_lattice_shape(crf, T, U1, kind):
    _, _, rc = one_case(crf, 100 * T + U1, [T], [U1 - 1], 9, 3, kind)
    assert np.isfinite(rc).all()
    if (T, U1) == (5, 4):                                            # ... and inside a padded tensor larger than the lattice
        one_case(crf, 7, [T], [U1 - 1], 9, 3, kind, T=8, U1=7)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,feasible", [(3, True), (2, False)])
def test_a_repeated_label_needs_a_frame_between(crf, T, feasible, kind):
    """y = [a, a]: T = 3 is just enough (one path per placement of the separating blank), T = 2 has no path -- +inf, zero gradient, no NaN."""
    costs, grad, rc = one_case(crf, T, [T], [2], 9, 3, kind, labels=[[5, 5]])
    assert np.isfinite(rc[0]) == feasible
    if not feasible:
        assert costs[0] == np.inf and not grad.any()


@pytest.mark.parametrize("V,blank", [(2, 0), (2, 1), (9, 3), (65, 64), (4097, 0), (4097, 4096)])
def test_every_vocabulary_and_blank(crf, V, blank):
    """(V = 2: every label is the one class beside the blank -- all repeats, T_n = 2 U_n - 1 just feasible.)"""
    for kind in KINDS:
        one_case(crf, V + blank, [5, 3], [3, 2], V, blank, kind)


def test_the_long_case_at_the_widest_row(crf):
    """(130, 70) at V = 4097: log-domain values of about 1 000 at the far corner, where fp32 recursions lose the gradient's fourth digit."""
    one_case(crf, 1, [130], [69], 4097, 4096, "float32")


def _pattern(name, U):
    """U labels from {1, 2, 4} (blank = 3): no two adjacent ones equal; all equal; or `a a b b a` from label index s on in the first."""
    lab = [(1, 2, 4)[i % 3] for i in range(U)]
    if name == "equal":
        return [2] * U
    if name.startswith("aabba"):
        s = int(name[5:])
        a = next(v for v in (1, 2, 4) if v != lab[s - 1] and v != lab[s + 5])
        b = next(v for v in (1, 2, 4) if v != a)
        lab[s:s + 5] = [a, a, b, b, a]
    return lab


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["distinct", "equal", "aabba61", "aabba62", "aabba63"])
def test_label_patterns_at_a_wave_boundary(crf, name, kind):
    """Columns 63 | 64 are handed across two waves: a repeat (y_u = y_{u+1}, no direct move) at u = 62 .. 66 by the pattern's position."""
    U = 70
    lab = _pattern(name, U)
    rep = ctct_ref.repeats(lab)
    assert rep == {"distinct": 0, "equal": U - 1}.get(name, 2)
    T = U + rep + 3
    _, _, rc = one_case(crf, 11, [T], [U], 5, 3, kind, labels=[lab])
    assert np.isfinite(rc).all()


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch_alone_and_again(crf, kind):
    """One call over utterances of every size class; the same bits for an utterance alone and inside the batch, and on a second run."""
    V, blank = 9, 3
    x, labels, lx, ly = ctct_ref.random_case(31, RAGGED_T, RAGGED_U, V, blank)
    t, exact, fused = prepare(x, kind)
    rc, rg = ctct_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    lab_t = torch.from_numpy(labels)
    costs, invalid, grad = run(crf, t, lab_t, lx, ly, blank, fused)
    assert not invalid.any() and np.isfinite(rc).all()
    check(kind, costs, grad, rc, rg, "ragged")
    assert not grad[~live_mask(grad.shape, lx, ly)].any(), "a padding element of the gradient is not zero"
    again = run(crf, t, lab_t, lx, ly, blank, fused)
    assert np.array_equal(again[0], costs) and np.array_equal(again[2], grad)
    for n in range(len(lx)):                                         # alone, cut to its own size
        a, b = lx[n], ly[n]
        acosts, _, agrad = run(crf, t[n:n + 1, :a, :b + 1].contiguous(), lab_t[n:n + 1, :b].contiguous(), [a], [b], blank, fused)
        assert acosts[0] == costs[n] and np.array_equal(agrad[0], grad[n, :a, :b + 1]), n


@pytest.mark.parametrize("kind", ("normalised", "float32", "bfloat16"))
def test_minus_infinity_entries(crf, kind):
    V, blank, T, U = 6, 0, 80, 70
    x, labels, lx, ly = ctct_ref.random_case(5, [T] * 5, [U] * 5, V, blank)
    for n, u in ((0, 10), (1, 63), (1, 64)):                         # (y_u = y_{u+1} needs the blank of column u: keep those columns passable)
        if labels[n, u - 1] == labels[n, u]:
            labels[n, u] = next(v for v in range(1, V) if v != labels[n, u - 1] and v != labels[n, u + 1])
    t, _, fused = prepare(x, kind)
    t[0, :, 10, blank] = -np.inf                                    # utterance 0: a dead blank column inside a wave
    t[1, :, 63:65, blank] = -np.inf                                  # utterance 1: dead blank columns on both sides of a wave boundary
    t[2, 5, 64, :] = -np.inf                                         # utterance 2: whole rows, one at a wave's first column, one inside
    t[2, 40, 30, :] = -np.inf
    t[3, 7, :, :] = -np.inf                                          # utterance 3: a frame nothing passes -- no path is left
    t[4, :, 64, labels[4, 63]] = -np.inf                             # utterance 4: no repeat of y_64 -- the column across the boundary
    exact = t.double().numpy()
    rc, rg = ctct_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    assert rc[3] == np.inf and np.isfinite(np.delete(rc, 3)).all()
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), lx, ly, blank, fused)
    assert not invalid.any() and costs[3] == np.inf and not grad[3].any()
    check(kind, costs, grad, rc, rg, "-inf")


@pytest.mark.parametrize("kind", ("normalised", "bfloat16"))
def test_invalid_utterances_beside_valid_ones(crf, kind):
    """T_n outside [1, T], U_n outside [0, U], a label outside [0, V), a label equal to the blank: decided on the device."""
    V, blank, T, U = 7, 2, 6, 3
    x, labels, _, _ = ctct_ref.random_case(9, [T] * 8, [U] * 8, V, blank)
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
    rc, rg = ctct_ref.batch_ref(exact[good], labels[good], [lx[n] for n in good], [ly[n] for n in good], blank, fused)
    assert np.isfinite(rc).all()
    check(kind, costs[good], grad[good], rc, rg, "beside invalid")
    with pytest.raises(ValueError):                                  # the same lengths on the CPU are refused up front
        crf.ctct_loss(t.to(DEV), torch.from_numpy(labels).to(DEV), i32(lx, "cpu"), i32(ly, "cpu"), blank=blank, fuse_log_softmax=fused)


@pytest.mark.parametrize("fused", (False, True))
def test_reductions_average_frames_and_grad_output(crf, fused):
    V, blank = 11, 10
    x, labels, lx, ly = ctct_ref.random_case(3, [9, 7, 4], [5, 2, 0], V, blank)
    t, exact, _ = prepare(x, "float32" if fused else "normalised")
    rc, rg = ctct_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    lab = torch.from_numpy(labels).to(DEV)
    frames = np.asarray(lx, dtype=np.float64)
    w = np.asarray([0.5, -2.0, 3.0])
    plans = [(dict(), w, rc), (dict(reduction="none"), w, rc), (dict(reduction="sum"), np.ones(3), rc.sum()),
             (dict(reduction="mean"), np.ones(3) / 3, rc.mean()), (dict(average_frames=True), w / frames, rc / frames),
             (dict(average_frames=True, reduction="mean"), 1 / frames / 3, (rc / frames).mean())]
    for lengths_on in (DEV, "cpu"):
        for kw, scale, want in plans:
            leaf = t.to(DEV).requires_grad_(True)
            out = crf.ctct_loss(leaf, lab, i32(lx, lengths_on), i32(ly, lengths_on), blank=blank, fuse_log_softmax=fused, **kw)
            assert np.allclose(out.detach().double().cpu().numpy(), want, rtol=TOL, atol=0), kw
            (out * torch.tensor(w, dtype=torch.float32, device=DEV)).sum().backward() if out.dim() else out.backward()
            ref = rg * scale[:, None, None, None]
            assert leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape
            assert np.abs(leaf.grad.double().cpu().numpy() - ref).max() <= TOL * np.abs(ref).max(), kw
    costs, invalid = crf.ctct_loss(t.to(DEV), lab, i32(lx), i32(ly), blank=blank, fuse_log_softmax=fused, return_invalid=True)
    assert costs.shape == (3,) and invalid.dtype == torch.int32 and not invalid.any()


def test_no_host_synchronisation_with_the_lengths_on_the_device(crf):
    V, blank = 9, 0
    x, labels, lx, ly = ctct_ref.random_case(4, [12, 9], [6, 3], V, blank)
    t = torch.from_numpy(x).to(torch.bfloat16).to(DEV)
    lab, lxd, lyd = torch.from_numpy(labels).to(DEV), i32(lx), i32(ly)
    leaf = t.clone().requires_grad_(True)
    norm = torch.log_softmax(t.float(), -1).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                            # the positive control: this build enforces the mode
            torch.ones(1, device=DEV).item()
        a = crf.ctct_loss(leaf, lab, lxd, lyd, blank=blank, fuse_log_softmax=True, reduction="mean", average_frames=True)
        a.backward()
        c = crf.ctct_loss(norm, lab, lxd, lyd, blank=blank)
        c.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(leaf.grad).all()) and bool(torch.isfinite(norm.grad).all())
    assert np.isfinite(float(a.detach())) and bool(torch.isfinite(c.detach()).all())


def test_the_widest_lattice(crf):
    """U + 1 = 1024 columns, sixteen waves: every hand-over between waves is on the path."""
    one_case(crf, 2, [1027], [1023], 9, 3, "float32")
