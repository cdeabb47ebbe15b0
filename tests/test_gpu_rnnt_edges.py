"""GPU tests: ctc_crf.rnnt_loss at the edges of its kernels (cat_amd/csrc/k_rnnt.hip) that tests/test_gpu_rnnt_loss.py does not reach: lattice
workgroups of 4 to 16 waves and U + 1 = 1024 itself, chains of two thousand steps, batches that cross the prep kernel's chunks of 64
utterances, labels checked past the first 64, compact tensors that are too long or too short, rows that are nothing but whole 16-byte
vectors up to V = 8192, raw output with a large common offset, and -inf entries that cut the lattice at a wave boundary.

The helpers, the tolerances and the reference on the quantised input are those of tests/test_gpu_rnnt_loss.py; lattices of 16 384 nodes and
more take the reference by anti-diagonals (tests/rnnt_ref.py lattice_diag, held to the node-by-node form by tests/test_rnnt_api.py)."""
import numpy as np
import pytest
import torch

from tests import rnnt_ref
from tests.test_gpu_rnnt_loss import DEV, KINDS, check, crf, one_case, prepare, run  # noqa: F401  (crf: the fixture)

pytestmark = pytest.mark.gpu


def live_mask(shape, lx, ly):
    live = np.zeros(shape[:3], dtype=bool)
    for n, (a, b) in enumerate(zip(lx, ly)):
        live[n, :a, :b + 1] = True
    return live


# ---- 1. every wave count of the workgroup lattice kernel ----
@pytest.mark.parametrize("kind", ("normalised", "bfloat16"))
@pytest.mark.parametrize("U1", (192, 193, 256, 257, 512, 513, 960, 961, 1023, 1024))
def test_every_wave_count(crf, U1, kind):
    """3 / 4, 4 / 5, 8 / 9, 15 / 16 and 16 waves per workgroup, the top lane of each handing its value to the next wave through LDS; T = 1
    and 2 end inside the first batch of diagonals, T = 9 crosses it."""
    for T in (1, 2, 9):
        one_case(crf, 10 * U1 + T, [T], [U1 - 1], 3, 1, kind)


# ---- 2. a ragged batch in one wide launch ----
WIDE_T, WIDE_U = (2, 3, 1, 5, 4), (1023, 960, 512, 64, 0)


@pytest.mark.parametrize("kind", ("normalised", "float32"))
def test_ragged_batch_in_one_wide_launch(crf, kind):
    """16, 16, 9, 2 and 1 live waves in workgroups of 16: the same bits padded, compact (lengths on the device and on the host) and alone."""
    V, blank = 4, 2
    x, labels, lx, ly = rnnt_ref.random_case(77, WIDE_T, WIDE_U, V, blank)
    t, exact, fused = prepare(x, kind)
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    lab_t = torch.from_numpy(labels)
    costs, invalid, grad = run(crf, t, lab_t, lx, ly, blank, fused)
    assert not invalid.any()
    check(kind, costs, grad, rc, rg, "wide padded")
    assert not grad[~live_mask(grad.shape, lx, ly)].any(), "a padding element of the gradient is not zero"
    ct, cl = rnnt_ref.to_compact(t, lab_t, lx, ly)
    for where in (DEV, "cpu"):
        ccosts, cinv, cgrad = run(crf, ct, cl, lx, ly, blank, fused, compact=True, lengths_on=where)
        assert not cinv.any() and np.array_equal(ccosts, costs), (where, ccosts, costs)
        assert np.array_equal(cgrad, rnnt_ref.to_compact(grad, labels, lx, ly)[0]), where
    for n, (a, b) in enumerate(zip(lx, ly)):                         # alone, cut to its own size
        acosts, _, agrad = run(crf, t[n:n + 1, :a, :b + 1].contiguous(), lab_t[n:n + 1, :b].contiguous(), [a], [b], blank, fused)
        assert acosts[0] == costs[n] and np.array_equal(agrad[0], grad[n, :a, :b + 1]), n


# ---- 3. long chains ----
@pytest.mark.parametrize("kind", ("normalised", "float32"))
@pytest.mark.parametrize("T,U1", [(1024, 1024), (1000, 200), (4000, 8)])
def test_long_chains(crf, T, U1, kind):
    """T + U = 2 047 dependent steps with 16 waves and a barrier each, 1 199 with four, 4 007 in one wave; the errors are printed by check
    (DESIGN.md 7 (f15) records them)."""
    one_case(crf, T + U1, [T], [U1 - 1], 4, 0, kind)


# ---- 4. many utterances: the prep kernel's chunks of 64, the binary search over the offsets ----
def many_case(N):
    """N lattices with T_n in 1..4 and U_n in 0..3; the utterances that the second run makes invalid have a label to spoil."""
    rng = np.random.default_rng(1000 + N)
    T_n, U_n = rng.integers(1, 5, N), rng.integers(0, 4, N)
    spots = sorted({n for n in (0, 63, 64, 127, N - 1) if n < N})
    U_n[spots] = np.maximum(U_n[spots], 1)
    return T_n.tolist(), U_n.tolist(), spots


@pytest.mark.parametrize("N", (64, 65, 128, 129, 257))
def test_many_utterances(crf, N):
    V, blank, kind = 4, 1, "float32"
    T_n, U_n, spots = many_case(N)
    x, labels, lx, ly = rnnt_ref.random_case(N, T_n, U_n, V, blank, T=4, U1=4)
    t, exact, fused = prepare(x, kind)
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    lab_t = torch.from_numpy(labels)
    costs, invalid, grad = run(crf, t, lab_t, lx, ly, blank, fused)
    assert not invalid.any()
    check(kind, costs, grad, rc, rg, ("many", N))
    assert not grad[~live_mask(grad.shape, lx, ly)].any()
    ct, cl = rnnt_ref.to_compact(t, lab_t, lx, ly)
    ccosts, cinv, cgrad = run(crf, ct, cl, lx, ly, blank, fused, compact=True)
    assert not cinv.any() and np.array_equal(ccosts, costs)
    assert np.array_equal(cgrad, rnnt_ref.to_compact(grad, labels, lx, ly)[0])
    again = run(crf, t, lab_t, lx, ly, blank, fused)                 # no atomics: a second call gives the same bits
    assert np.array_equal(again[0], costs) and np.array_equal(again[2], grad)
    cagain = run(crf, ct, cl, lx, ly, blank, fused, compact=True)
    assert np.array_equal(cagain[0], ccosts) and np.array_equal(cagain[2], cgrad)

    # the same batch with invalid utterances at the chunk boundaries: lengths out of range (no rows in the compact layout) and label errors
    # (which keep their rows), in turn
    blx, bly, blab = list(lx), list(ly), labels.copy()
    norows = []
    for k, n in enumerate(spots):
        what = k % 5
        if what == 0:
            blx[n] = 0
        elif what == 1:
            blab[n, bly[n] - 1] = blank
        elif what == 2:
            bly[n] = -1
        elif what == 3:
            blab[n, 0] = V
        else:
            bly[n] = 5000                                            # (past U in the padded layout and past every bound of the compact one)
        if what in (0, 2, 4):
            norows.append(n)
    bad = np.zeros(N, dtype=bool)
    bad[spots] = True
    blab_t = torch.from_numpy(blab)
    bcosts, binv, bgrad = run(crf, t, blab_t, blx, bly, blank, fused)
    assert binv.tolist() == bad.astype(int).tolist()
    assert np.all(bcosts[bad] == np.inf) and not bgrad[bad].any()
    assert np.array_equal(bcosts[~bad], costs[~bad]) and np.array_equal(bgrad[~bad], grad[~bad])
    clx = [0 if n in norows else a for n, a in enumerate(lx)]        # what each utterance claims of the compact tensors
    cly = [0 if n in norows else b for n, b in enumerate(ly)]
    ct, cl = rnnt_ref.to_compact(t, blab_t, clx, cly)
    ccosts, cinv, cgrad = run(crf, ct, cl, blx, bly, blank, fused, compact=True)
    assert cinv.tolist() == bad.astype(int).tolist()
    assert np.array_equal(ccosts, bcosts)
    assert np.array_equal(cgrad, rnnt_ref.to_compact(bgrad, blab, clx, cly)[0])


# ---- 5. compact tensors that do not fit ----
@pytest.mark.parametrize("kind", ("normalised", "float32"))
def test_compact_tensors_that_do_not_fit(crf, kind):
    """include/ctc_crf_hip.h: an utterance whose rows or labels would reach past compact_rows / compact_labels is invalid (and so is every
    one behind it: its offset lies behind the end already); padding and surplus rows are written as zeros."""
    V, blank = 4, 3
    T_n, U_n = [3, 2, 4, 2, 3, 2], [2, 0, 3, 2, 0, 1]
    x, labels, lx, ly = rnnt_ref.random_case(55, T_n, U_n, V, blank)
    t, exact, fused = prepare(x, kind)
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    ct, cl = rnnt_ref.to_compact(t, torch.from_numpy(labels), lx, ly)
    costs, invalid, grad = run(crf, ct, cl, lx, ly, blank, fused, compact=True)
    assert not invalid.any()
    check(kind, costs, grad, rc, rnnt_ref.to_compact(rg, labels, lx, ly)[0], "fits")
    off = np.concatenate([[0], np.cumsum([a * (b + 1) for a, b in zip(lx, ly)])])
    loff = np.concatenate([[0], np.cumsum(ly)])
    # (a) 5 surplus rows, 3 surplus labels
    more = torch.cat([ct, torch.from_numpy(rnnt_ref.random_case(56, [5], [0], V, blank)[0].reshape(5, V)).to(ct.dtype)])
    acosts, ainv, agrad = run(crf, more, torch.cat([cl, torch.tensor([-1, V, blank], dtype=torch.int32)]), lx, ly, blank, fused, compact=True)
    assert not ainv.any() and np.array_equal(acosts, costs)
    assert np.array_equal(agrad[:off[6]], grad) and agrad.shape[0] == off[6] + 5 and not agrad[off[6]:].any()
    # (b) the rows end one short of utterance 3's last, (c) the labels one short of its last
    for what, rows, nlab in (("rows", off[4] - 1, loff[6]), ("labels", off[6], loff[4] - 1)):
        bcosts, binv, bgrad = run(crf, ct[:rows].contiguous(), cl[:nlab].contiguous(), lx, ly, blank, fused, compact=True)
        assert binv.tolist() == [0, 0, 0, 1, 1, 1], (what, binv)
        assert np.array_equal(bcosts[:3], costs[:3]) and np.all(bcosts[3:] == np.inf), (what, bcosts)
        assert np.array_equal(bgrad[:off[3]], grad[:off[3]]) and bgrad.shape[0] == rows and not bgrad[off[3]:].any(), what


# ---- 6. labels checked along the whole row ----
def test_labels_are_checked_along_the_whole_row(crf):
    V, blank, U, T, kind = 4, 2, 130, 2, "float32"
    x, labels, lx, ly = rnnt_ref.random_case(66, [T] * 7, [U] * 5 + [U, 100], V, blank)
    for n, (at, value) in enumerate(zip((63, 64, 127, 128, 129), (V, -1, blank, V, -1))):
        labels[n, at] = value
    labels[6, 100] = blank                                           # behind utterance 6's length: never read
    t, exact, fused = prepare(x, kind)
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), lx, ly, blank, fused)
    assert invalid.tolist() == [1, 1, 1, 1, 1, 0, 0]
    assert np.all(costs[:5] == np.inf) and not grad[:5].any()
    rc, rg = rnnt_ref.batch_ref(exact[5:], labels[5:], lx[5:], ly[5:], blank, fused)
    check(kind, costs[5:], grad[5:], rc, rg, "labels")


# ---- 7. vocabulary widths where the whole row is vectors ----
@pytest.mark.parametrize("V,blank", [(1, 0)] + [(V, b) for V in (4, 8, 16, 256, 512, 520, 1024, 2048, 8191, 8192) for b in (0, V - 1)])
def test_rows_of_whole_vectors(crf, V, blank):
    """Multiples of 4 (fp32) and of 8 (16 bits): every row aligned, every chunk a 16-byte load; 512 elements = one chunk per lane (fp16, bf16),
    520 = one more for lane 0; 8192 is the limit, 8191 the last width with a tail."""
    for kind in KINDS:
        if V == 1:                                                   # nothing but the blank: no labels, log_softmax = 0, cost exactly 0
            costs, grad = one_case(crf, 1, [5, 3], [0, 0], V, blank, kind)
            assert not costs.any()
            if kind == "normalised":                                 # (d cost / d log_probs is the occupancy, -1 at every frame's blank ...
                assert np.all(grad[0, :5] == -1.0) and np.all(grad[1, :3] == -1.0)
            else:                                                    # ... which the softmax's backward cancels exactly)
                assert not grad.any()
        else:
            one_case(crf, V + blank, [5, 3], [3, 2], V, blank, kind)


# ---- 8. shift invariance of the fused path ----
def shifted_case(seed, T, U1, offset):
    """Raw output on a 2^-10 grid plus `offset` (a number, or "rows": -4096, 0 or 4096 drawn per row), every value exact in fp32."""
    V, blank = 9, 3
    rng = np.random.default_rng(seed)
    x = np.round(3.0 * rng.standard_normal((1, T, U1, V)) * 1024.0) / 1024.0
    x = x + (rng.choice([-4096.0, 0.0, 4096.0], (1, T, U1, 1)) if isinstance(offset, str) else offset)
    labels = rng.integers(0, V - 1, (1, U1 - 1))
    return x, (labels + (labels >= blank)).astype(np.int32), V, blank


@pytest.mark.parametrize("offset", (-4096.0, 1024.0, 4096.0, "rows"))
@pytest.mark.parametrize("T,U1", [(40, 21), (130, 70)])
def test_a_common_offset_does_not_change_the_fp32_result(crf, T, U1, offset):
    """log_softmax(x + c) = log_softmax(x): the normaliser is taken as (x - max) - log(sum), so that a large c costs no digits.  (Taken as
    x - (max + log(sum)) the gradient was off by 1.2e-4 to 2.6e-4 of max |ref| at c = +-4096 on the MI355X)"""
    x, labels, V, blank = shifted_case(T + U1, T, U1, offset)
    t = torch.from_numpy(x).float()
    assert np.array_equal(t.double().numpy(), x), "the shifted input is not exact in fp32"
    rc, rg = rnnt_ref.batch_ref(x, labels, [T], [U1 - 1], blank, True)
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), [T], [U1 - 1], blank, True)
    assert not invalid.any()
    check("float32", costs, grad, rc, rg, ("offset", offset, T, U1))


@pytest.mark.parametrize("kind", ("bfloat16", "float16"))
@pytest.mark.parametrize("offset", (-1024.0, 1024.0))
@pytest.mark.parametrize("T,U1", [(40, 21), (130, 70)])
def test_a_common_offset_in_16_bits(crf, T, U1, offset, kind):
    x, labels, V, blank = shifted_case(T + U1 + 1, T, U1, offset)
    t = torch.from_numpy(x).to(getattr(torch, kind))
    if kind == "float16":                                            # one row at the ends of the format: its blank is certain
        t[0, T // 2, U1 // 2, :] = -65504.0
        t[0, T // 2, U1 // 2, blank] = 65504.0
    exact = t.double().numpy()
    rc, rg = rnnt_ref.batch_ref(exact, labels, [T], [U1 - 1], blank, True)
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), [T], [U1 - 1], blank, True)
    assert not invalid.any() and np.isfinite(costs).all() and np.isfinite(grad).all()
    check(kind, costs, grad, rc, rg, ("offset", offset, T, U1))


# ---- 9. -inf across a wave boundary ----
@pytest.mark.parametrize("kind", ("normalised", "float32", "float16"))
def test_minus_infinity_across_a_wave_boundary(crf, kind):
    """U + 1 = 130 is three waves; column 64 is the first of the second.  Utterance 0: no label 63 at any t -- no path.  Utterance 1: label 63
    at t = 3 alone -- every path takes it.  Utterance 2: frame 2 has its blank at u = 100 alone -- every path takes that."""
    V, blank, T, U1 = 4, 0, 6, 130
    x, labels, lx, ly = rnnt_ref.random_case(99, [T] * 3, [U1 - 1] * 3, V, blank)
    t, _, fused = prepare(x, kind)
    t[0, :, 63, labels[0, 63]] = -np.inf
    keep = t[1, 3, 63, labels[1, 63]].clone()
    t[1, :, 63, labels[1, 63]] = -np.inf
    t[1, 3, 63, labels[1, 63]] = keep
    keep = t[2, 2, 100, blank].clone()
    t[2, 2, :, blank] = -np.inf
    t[2, 2, 100, blank] = keep
    exact = t.double().numpy()
    rc, rg = rnnt_ref.batch_ref(exact, labels, lx, ly, blank, fused)
    assert rc[0] == np.inf and np.isfinite(rc[1:]).all()
    lp = rnnt_ref.log_softmax(exact) if fused else exact            # the occupancies themselves: all of the mass at the two funnels
    assert abs(rnnt_ref.ref_normalised(lp[1], labels[1], blank)[1][3, 63, labels[1, 63]] + 1.0) <= 1e-9
    assert abs(rnnt_ref.ref_normalised(lp[2], labels[2], blank)[1][2, 100, blank] + 1.0) <= 1e-9
    costs, invalid, grad = run(crf, t, torch.from_numpy(labels), lx, ly, blank, fused)
    assert not invalid.any() and costs[0] == np.inf and not grad[0].any()
    assert np.isfinite(grad).all() and np.isfinite(costs[1:]).all()
    check(kind, costs[1:], grad[1:], rc[1:], rg[1:], "-inf at a wave boundary")
