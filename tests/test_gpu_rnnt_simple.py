"""GPU tests: ctc_crf.rnnt_loss_simple (crf_rnnt_simple_loss / crf_rnnt_simple_grad, cat_amd/csrc/k_rnnt_join.hip) against the fp64 yardstick
of tests/rnnt_simple_ref.py, which forms the joint tensor f[:, :, None, :] + g[:, None, :, :] on the inputs' quantised values.

Tolerances are the project's own (tests/test_gpu_rnnt_loss.py): the cost within TOL = 1e-4 relative; an fp32 gradient within
TOL * max |ref| of its own tensor; a 16-bit gradient within 2^-8 |ref| + TOL * max |ref| entry by entry.

Shapes.  The kernels' tiles are: row stage 32 frames x 32 rows per workgroup, 128 class columns per LDS chunk walked 4 columns a step;
grad stage 256 class columns per workgroup (64 per wave), 32 rows per register tile, chunks of 16 frames dealt to 4 splits (a cycle of 64
frames).  Beside the lattices every rnnt_loss test takes, (T, U+1) therefore has 15, 16, 17 / 31, 32, 33 / 63, 64, 65 frames and
31, 32, 33 / 63, 64, 65 rows, and V has 3, 4, 5 / 63, 64, 65 / 127, 128, 129 / 255, 256, 257 / 1025 / 8192."""
import numpy as np
import pytest
import torch

from tests import rnnt_simple_ref
from tests.score_grad_ref import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KINDS = ("float32", "bfloat16", "float16")
SENT = 768.0                 # (exact in bf16 and fp16)
SHAPES = [(1, 1), (1, 2), (2, 1), (5, 4), (64, 64), (65, 65), (3, 129), (130, 70),                 # (T, U + 1): those of rnnt_loss,
          (15, 33), (16, 32), (17, 31), (31, 2), (32, 3), (33, 63), (63, 5), (64, 2)]               # and the tiles' edges
RAGGED_T, RAGGED_U = (130, 129, 65, 64, 1), (69, 64, 63, 0, 0)


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    return ctc_crf


def i32(a, dev=DEV):
    return torch.tensor(np.asarray(a).reshape(-1), dtype=torch.int32, device=dev)


def quantise(f, g, kind):
    """fp32 numpy -> (the two input tensors of that kind on the CPU, their exact fp64 values)."""
    tf, tg = torch.from_numpy(f).to(getattr(torch, kind)), torch.from_numpy(g).to(getattr(torch, kind))
    return tf, tg, tf.double().numpy(), tg.double().numpy()


def run(crf, tf, tg, labels, lx, ly, blank, weights=None, lengths_on=DEV, want=(True, True)):
    """One forward and backward through the C calls' Python wrappers, the gradients written over a sentinel.
    -> (costs [N] fp64, invalid [N], d f, d g as fp64 numpy; None where not wanted)."""
    core = crf._C
    N = len(lx)
    costs, invalid, call = core.rnnt_simple_fwd(tf.to(DEV), tg.to(DEV), torch.as_tensor(labels).to(DEV), i32(lx, lengths_on), i32(ly, lengths_on), blank)
    w = torch.ones(N, device=DEV) if weights is None else torch.tensor(weights, dtype=torch.float32, device=DEV)
    outs = tuple(torch.full(t.shape, SENT, dtype=t.dtype, device=DEV) if k else None for t, k in zip((tf, tg), want))
    gf, gg = core.rnnt_simple_bwd(call, w, want[0], want[1], grad_out=outs)
    torch.cuda.synchronize()
    res = []
    for t in (gf, gg):
        a = None if t is None else t.double().cpu().numpy()
        assert a is None or not np.any(a == SENT), "an element of a gradient was not written"
        res.append(a)
    return costs.double().cpu().numpy(), invalid.cpu().numpy(), res[0], res[1]


def check(kind, costs, grads, rc, refs, what=""):
    assert np.all(np.abs(costs - rc) <= TOL * np.abs(rc)), (what, kind, costs, rc)
    for name, grad, rg in zip(("df", "dg"), grads, refs):
        top = np.abs(rg).max()
        print(what, kind, name, "cost err", float(np.max(np.abs(costs - rc) / np.maximum(np.abs(rc), 1e-30))), "grad err",
              float(np.abs(grad - rg).max()), "max |ref|", float(top))
        assert np.isfinite(grad).all(), (what, kind, name)
        if kind == "float32":
            assert np.abs(grad - rg).max() <= TOL * top, (what, kind, name, np.abs(grad - rg).max(), top)
        else:
            over = np.abs(grad - rg) - (2.0 ** -8 * np.abs(rg) + TOL * top)
            assert over.max() <= 0.0, (what, kind, name, over.max(), top)


def padding_is_zero(gf, gg, lx, ly):
    for n, (a, b) in enumerate(zip(lx, ly)):
        assert not gf[n, a:].any() and not gg[n, b + 1:].any(), ("a padding element of a gradient is not zero", n)


def one_case(crf, seed, T_n, U_n, V, blank, kind, T=None, U1=None):
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(seed, T_n, U_n, V, blank, T, U1)
    tf, tg, ef, eg = quantise(f, g, kind)
    rc, rf, rg = rnnt_simple_ref.batch_ref(ef, eg, labels, lx, ly, blank)
    costs, invalid, gf, gg = run(crf, tf, tg, labels, lx, ly, blank)
    assert not invalid.any()
    check(kind, costs, (gf, gg), rc, (rf, rg), (T_n, U_n, V, blank))
    padding_is_zero(gf, gg, lx, ly)
    return costs, gf, gg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,U1", SHAPES)
def test_every_lattice_shape(crf, T, U1, kind):
    one_case(crf, 100 * T + U1, [T], [U1 - 1], 9, 3, kind)
    if (T, U1) == (5, 4):                                            # ... and inside padded tensors larger than the lattice
        one_case(crf, 7, [T], [U1 - 1], 9, 3, kind, T=8, U1=7)


@pytest.mark.parametrize("V", [2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025])
def test_every_vocabulary_and_blank(crf, V):
    """(T, U + 1) = (5, 4), the blank first, last and in the middle; odd V puts every second 16-bit row on a 2-byte boundary."""
    for blank in sorted({0, V // 2, V - 1}):
        for kind in KINDS:
            one_case(crf, V + blank, [5, 3], [3, 2], V, blank, kind)


def test_a_single_class_and_the_widest_row(crf):
    for kind in KINDS:
        costs, _, _ = one_case(crf, 1, [5], [0], 1, 0, kind)       # V = 1: only blanks, every probability is 1
        assert costs[0] == 0.0
        one_case(crf, 2, [3], [1], 8192, 4097, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch_alone_and_twice(crf, kind):
    """One call over utterances of every size class: zeros over the padding, the same bits for an utterance alone and in the batch, the
    same bits twice."""
    V, blank = 9, 3
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(31, RAGGED_T, RAGGED_U, V, blank)
    tf, tg, ef, eg = quantise(f, g, kind)
    rc, rf, rg = rnnt_simple_ref.batch_ref(ef, eg, labels, lx, ly, blank)
    costs, invalid, gf, gg = run(crf, tf, tg, labels, lx, ly, blank)
    assert not invalid.any()
    check(kind, costs, (gf, gg), rc, (rf, rg), "ragged")
    padding_is_zero(gf, gg, lx, ly)
    costs2, _, gf2, gg2 = run(crf, tf, tg, labels, lx, ly, blank)
    assert np.array_equal(costs, costs2) and np.array_equal(gf, gf2) and np.array_equal(gg, gg2)
    for n in range(5):                                               # alone, cut to its own size
        a, b = lx[n], ly[n]
        ac, _, af, ag = run(crf, tf[n:n + 1, :a].contiguous(), tg[n:n + 1, :b + 1].contiguous(), labels[n:n + 1, :b], [a], [b], blank)
        assert ac[0] == costs[n] and np.array_equal(af[0], gf[n, :a]) and np.array_equal(ag[0], gg[n, :b + 1]), n


@pytest.mark.parametrize("kind", ("float32", "bfloat16"))
@pytest.mark.parametrize("offset", (60.0, 120.0))
def test_peaks_at_different_columns_of_f_and_g(crf, offset, kind):
    """f peaks at column 1, g at column 2: exp(f - max f) exp(g - max g) is 0 in fp32 at every node (offset 120) although the loss is
    finite; the per-node maximum keeps every digit."""
    f, g, labels, lx, ly = rnnt_simple_ref.peaked_case(offset)
    tf, tg, ef, eg = quantise(f, g, kind)
    rc, rf, rg = rnnt_simple_ref.batch_ref(ef, eg, labels, lx, ly, 0)
    assert np.isfinite(rc).all() and rc[0] > 100.0
    costs, invalid, gf, gg = run(crf, tf, tg, labels, lx, ly, 0)
    assert not invalid.any()
    check(kind, costs, (gf, gg), rc, (rf, rg), ("peaked", offset))


@pytest.mark.parametrize("kind", ("float32", "bfloat16"))
def test_common_offsets(crf, kind):
    """+-4096 on f, on g, and on both with opposite signs.  The inputs lie on a grid on which the shift is exact in their dtype (2^-10 in
    fp32, 32 in bf16, whose ulp at 4096 that is), so every shifted input is the SAME problem: each is held, with the project's tolerances,
    to the reference of the unshifted one."""
    V, blank = 33, 5
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(11, [40, 23], [20, 7], V, blank)
    grid, per = (2.0 ** -10, 2.0 ** 10) if kind == "float32" else (32.0, 1.0 / 3.0)
    f, g = (np.round(f * per) * grid).astype(np.float32), (np.round(g * per) * grid).astype(np.float32)
    tf0, tg0, ef, eg = quantise(f, g, kind)
    assert np.array_equal(ef, f) and np.array_equal(eg, g)
    rc0, rf0, rg0 = rnnt_simple_ref.batch_ref(ef, eg, labels, lx, ly, blank)
    assert np.isfinite(rc0).all()
    c0, _, gf0, gg0 = run(crf, tf0, tg0, labels, lx, ly, blank)
    check(kind, c0, (gf0, gg0), rc0, (rf0, rg0), "unshifted")
    for of, og in ((4096.0, 0.0), (-4096.0, 0.0), (0.0, 4096.0), (0.0, -4096.0), (4096.0, -4096.0), (-4096.0, 4096.0)):
        tf, tg, sf, sg = quantise(f + np.float32(of), g + np.float32(og), kind)
        assert np.array_equal(sf, f.astype(np.float64) + of) and np.array_equal(sg, g.astype(np.float64) + og)      # the shift is exact
        costs, invalid, gf, gg = run(crf, tf, tg, labels, lx, ly, blank)
        assert not invalid.any()
        check(kind, costs, (gf, gg), rc0, (rf0, rg0), ("offset", of, og))


@pytest.mark.parametrize("kind", ("float32", "bfloat16"))
def test_minus_infinity_entries(crf, kind):
    V, blank = 6, 0
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(5, [6, 6, 6], [4, 4, 4], V, blank)
    tf, tg, _, _ = quantise(f, g, kind)
    tf[0, :, 3] = -np.inf                                            # utterance 0: a column of f -- a class no frame ever emits
    labels[0] = np.where(labels[0] == 3, 4, labels[0])               # (... and no label asks for)
    tg[1, 2, :] = -np.inf                                            # utterance 1: a whole row of g at u = 2, which every path crosses
    tg[2, 4, int(labels[2, 0])] = -np.inf                               # utterance 2: one entry no path needs (u = U_n has no label)
    ef, eg = tf.double().numpy(), tg.double().numpy()
    rc, rf, rg = rnnt_simple_ref.batch_ref(ef, eg, labels, lx, ly, blank)
    assert rc[1] == np.inf and np.isfinite(rc[[0, 2]]).all()
    costs, invalid, gf, gg = run(crf, tf, tg, labels, lx, ly, blank)
    assert not invalid.any() and costs[1] == np.inf and not gf[1].any() and not gg[1].any()
    assert np.isfinite(gf).all() and np.isfinite(gg).all() and np.isfinite(costs[[0, 2]]).all()
    check(kind, costs[[0, 2]], (gf[[0, 2]], gg[[0, 2]]), rc[[0, 2]], (rf[[0, 2]], rg[[0, 2]]), "-inf")
    assert not gf[0, :, 3].any() and not gg[0, :, 3].any()


@pytest.mark.parametrize("kind", ("float32", "bfloat16"))
def test_invalid_utterances_beside_valid_ones(crf, kind):
    """T_n = 0, T_n > T, U_n > U, U_n < 0, a label outside [0, V), a label equal to the blank: decided on the device."""
    V, blank, T, U = 7, 2, 6, 3
    f, g, labels, _, _ = rnnt_simple_ref.random_case(9, [T] * 8, [U] * 8, V, blank)
    lx = [6, 0, 7, 5, 4, 6, 6, 3]
    ly = [3, 2, 3, 4, -1, 3, 2, 0]
    labels[5, 1] = V                                                 # utterance 5: a label outside [0, V)
    labels[6, 0] = blank                                             # utterance 6: the blank as a label
    labels[7, 0] = -1                                                # (behind utterance 7's length: never read)
    bad = [False, True, True, True, True, True, True, False]
    tf, tg, ef, eg = quantise(f, g, kind)
    costs, invalid, gf, gg = run(crf, tf, tg, labels, lx, ly, blank)
    assert invalid.tolist() == [int(b) for b in bad]
    good = [n for n, b in enumerate(bad) if not b]
    for n, b in enumerate(bad):
        if b:
            assert costs[n] == np.inf and not gf[n].any() and not gg[n].any(), n
    glx, gly = [lx[n] for n in good], [ly[n] for n in good]
    rc, rf, rg = rnnt_simple_ref.batch_ref(ef[good], eg[good], labels[good], glx, gly, blank)
    check(kind, costs[good], (gf[good], gg[good]), rc, (rf, rg), "beside invalid")
    ac, _, af, ag = run(crf, tf[good], tg[good], labels[good], glx, gly, blank)           # the neighbours are unaffected: the same bits
    assert np.array_equal(ac, costs[good]) and np.array_equal(af, gf[good]) and np.array_equal(ag, gg[good])
    with pytest.raises(ValueError):                                  # the same lengths on the CPU are refused up front
        crf.rnnt_loss_simple(tf.to(DEV), tg.to(DEV), torch.from_numpy(labels).to(DEV), i32(lx, "cpu"), i32(ly, "cpu"), blank=blank)


def test_reductions_average_frames_grad_output_and_one_sided_grads(crf):
    V, blank = 11, 10
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(3, [9, 7, 4], [5, 2, 0], V, blank)
    tf, tg, ef, eg = quantise(f, g, "float32")
    rc, rf, rg = rnnt_simple_ref.batch_ref(ef, eg, labels, lx, ly, blank)
    lab = torch.from_numpy(labels).to(DEV)
    frames = np.asarray(lx, dtype=np.float64)
    w = np.asarray([0.5, -2.0, 3.0])
    plans = [(dict(), w, rc), (dict(reduction="none"), w, rc), (dict(reduction="sum"), np.ones(3), rc.sum()),
             (dict(reduction="mean"), np.ones(3) / 3, rc.mean()), (dict(average_frames=True), w / frames, rc / frames),
             (dict(average_frames=True, reduction="mean"), 1 / frames / 3, (rc / frames).mean())]
    for lengths_on in (DEV, "cpu"):
        for kw, scale, want in plans:
            lf, lg = tf.to(DEV).requires_grad_(True), tg.to(DEV).requires_grad_(True)
            out = crf.rnnt_loss_simple(lf, lg, lab, i32(lx, lengths_on), i32(ly, lengths_on), blank=blank, **kw)
            assert np.allclose(out.detach().double().cpu().numpy(), want, rtol=TOL, atol=0), kw
            (out * torch.tensor(w, dtype=torch.float32, device=DEV)).sum().backward() if out.dim() else out.backward()
            for leaf, ref in ((lf, rf * scale[:, None, None]), (lg, rg * scale[:, None, None])):
                assert leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape
                assert np.abs(leaf.grad.double().cpu().numpy() - ref).max() <= TOL * np.abs(ref).max(), kw
    costs, invalid = crf.rnnt_loss_simple(tf.to(DEV), tg.to(DEV), lab, i32(lx), i32(ly), blank=blank, return_invalid=True)
    assert costs.shape == (3,) and invalid.dtype == torch.int32 and not invalid.any()
    for only in (0, 1):                                              # only f or only g requires grad: the other is not formed
        leaves = [tf.to(DEV), tg.to(DEV)]
        leaves[only].requires_grad_(True)
        crf.rnnt_loss_simple(leaves[0], leaves[1], lab, i32(lx), i32(ly), blank=blank, reduction="sum").backward()
        assert leaves[1 - only].grad is None
        ref = (rf, rg)[only]
        assert np.abs(leaves[only].grad.double().cpu().numpy() - ref).max() <= TOL * np.abs(ref).max()
        _, _, gf, gg = run(crf, tf, tg, labels, lx, ly, blank, want=(only == 0, only == 1))
        assert ((gg, gf)[only] is None) and np.array_equal((gf, gg)[only], leaves[only].grad.double().cpu().numpy())


def test_no_host_synchronisation_with_the_lengths_on_the_device(crf):
    V, blank = 9, 0
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(4, [12, 9], [6, 3], V, blank)
    lf = torch.from_numpy(f).to(torch.bfloat16).to(DEV).requires_grad_(True)
    lg = torch.from_numpy(g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    lab, lxd, lyd = torch.from_numpy(labels).to(DEV), i32(lx), i32(ly)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                            # the positive control: this build enforces the mode
            torch.ones(1, device=DEV).item()
        a = crf.rnnt_loss_simple(lf, lg, lab, lxd, lyd, blank=blank, reduction="mean", average_frames=True)
        a.backward()
        b = crf.rnnt_loss_simple(lf, lg, lab, lxd, lyd, blank=blank)
        b.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(lf.grad).all()) and bool(torch.isfinite(lg.grad).all())
    assert np.isfinite(float(a.detach())) and bool(torch.isfinite(b).all())


def test_agrees_with_rnnt_loss_on_the_materialised_joint_tensor(crf):
    """fp32, (65, 65), V = 65: both are fp64 recursions over fp32 node values -- the costs within 1e-6 relative."""
    V, blank = 65, 3
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(17, [65], [64], V, blank)
    tf, tg = torch.from_numpy(f).to(DEV), torch.from_numpy(g).to(DEV)
    lab = torch.from_numpy(labels).to(DEV)
    lf, lg = tf.clone().requires_grad_(True), tg.clone().requires_grad_(True)
    a = crf.rnnt_loss_simple(tf, tg, lab, i32(lx), i32(ly), blank=blank)
    b = crf.rnnt_loss(lf.unsqueeze(2) + lg.unsqueeze(1), lab, i32(lx), i32(ly), blank=blank, fuse_log_softmax=True)
    a, b = a.double().cpu().numpy(), b.detach().double().cpu().numpy()
    print("simple", a, "materialised", b, "relative", np.abs(a - b) / np.abs(b))
    assert np.all(np.abs(a - b) <= 1e-6 * np.abs(b)), (a, b)


def test_nothing_of_the_joint_tensors_size_is_allocated(crf):
    """N = 2, T = 64, U + 1 = 32, V = 1024 in fp32: the joint tensor would be 16.8 MB; forward and backward must stay under a quarter of
    that above what is allocated before the call (the gradients and the workspace come to about 2.6 MB)."""
    N, T, U1, V = 2, 64, 32, 1024
    f, g, labels, lx, ly = rnnt_simple_ref.random_case(8, [T] * N, [U1 - 1] * N, V, 0)
    lf, lg = torch.from_numpy(f).to(DEV).requires_grad_(True), torch.from_numpy(g).to(DEV).requires_grad_(True)
    lab, lxd, lyd = torch.from_numpy(labels).to(DEV), i32(lx), i32(ly)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.max_memory_allocated(DEV)
    crf.rnnt_loss_simple(lf, lg, lab, lxd, lyd, reduction="sum").backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - before
    joint = 4 * N * T * U1 * V
    print("rise", rise, "joint tensor", joint)
    assert lf.grad is not None and lg.grad is not None and rise < joint // 4, (rise, joint)
