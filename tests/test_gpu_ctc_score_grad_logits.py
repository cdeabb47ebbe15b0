"""GPU tests of the weighted multi-hypothesis CTC gradient on RAW network output in fp32 / bf16 / fp16 (ctc_crf._C.ctc_score_grad(fused=True) /
crf_ctc_score_grad_logits, ctc_crf.ctc_logp(fuse_log_softmax=True); cat_amd/csrc/k_score_grad.hip) against the fp64 reference of
tests/score_grad_logits_ref.py: the oracle's occupancies on the exactly upcast input minus W_u softmax64.  Every call writes into a grad
prefilled with NaN and scores prefilled with a sentinel, with the workspace poisoned, and runs batch-major AND time-major, which must agree;
scores and invalid must be ctc_score(fused=True)'s bits."""
import numpy as np
import pytest
import torch

from tests.score_grad_logits_ref import (DEAD, DTYPES, FRAME_LX, KERNEL_OF_L, N1, check_raw, core, fold_raw, kernel_name, parity_case, raw_ref,
                                         run_grad_raw)
from tests.score_grad_ref import TOL, flat, i32
from tests.util import post_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ctc_crf
    ctc_crf._C.set_debug_poison(True)
    yield ctc_crf
    ctc_crf._C.set_debug_poison(False)


def run_case(name, weights=None):
    c = parity_case(name)
    x = c["x"].to("cuda:0")
    assert x.dtype == DTYPES[c["dtype"]]
    out = {}
    for wname, w in c["weights"].items():
        if weights is not None and wname not in weights:
            continue
        g, sc, inv = run_grad_raw(x, c["hyps"], c["utt"], c["lx"], c["blank"], w)
        assert core.last_score_grad_kernel() == kernel_name(c["nr"], c["dtype"]), core.last_score_grad_kernel()
        out[wname] = (g, sc, inv, check_raw(c, g, sc, inv, w, f"{name} w={wname}"))
    return c, out


# 1. small batch: every dtype, three blanks, weights none / positive / of mixed sign
@pytest.mark.parametrize("blank", [0, 5, 2])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_parity_small(crf, dtype, blank):
    c, out = run_case(f"small_{dtype}_blank{blank}")
    assert set(out) == {"none", "pos", "mix"}
    for g, sc, inv, ref in out.values():
        assert not np.any(g[1]) and not np.any(ref[1]), "utterance 1 owns no hypothesis"
        assert inv.sum() == 2


# 2. one instantiation each, 16-bit inputs
@pytest.mark.parametrize("L", sorted(KERNEL_OF_L))
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_instantiation(crf, dtype, L):
    c, out = run_case(f"L{L}_{dtype}")
    assert max(len(h) for h in c["hyps"]) == L and not np.any(out["pos"][2])


# 3. odd V in 16 bits: rows on 2-byte boundaries; the frame loop's edges
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_odd_v_and_frame_loop_edges(crf, dtype):
    c, out = run_case(f"odd_v_{dtype}")
    assert c["x"].shape[2] % 2 == 1 and tuple(c["lx"]) == FRAME_LX and not np.any(out["pos"][2])


# 4. the occupancies entry by entry
def test_occupancies_entry_wise(crf):
    """One hypothesis, w = 1, fp32 raw: grad + softmax64 is gamma.  The fp32 difference of two values <= 1 carries <= 1.2e-7 absolute,
    1.2e-5 of an entry of 1e-2; the rest of TOL is the posterior's."""
    c = parity_case("small_fp32_blank0")
    r = c["ref"]
    h = int(np.argmax([len(a) if r["live"][k] else -1 for k, a in enumerate(c["hyps"])]))
    u = int(c["utt"][h])
    one = raw_ref(c["x32"], [c["hyps"][h]], [u], c["lx"], c["blank"])
    g, sc, inv = run_grad_raw(c["x"].to("cuda:0"), [c["hyps"][h]], [u], c["lx"], c["blank"], np.ones(1))
    n = int(c["lx"][u])
    got = g[u, :n].astype(np.float64) + one["soft"][u, :n]
    e = post_err(got, one["gamma"][0, :n], floor=1e-2)
    print(f"[score_grad_logits] occupancies entry-wise (>= 1e-2): {e:.3e}")
    assert e <= TOL, e
    assert not np.any(g[[k for k in range(N1) if k != u]])


# 5. shift invariance: lse_t far from 0, the cost per frame uneven, T = 1500
def test_shifted_log_probs(crf):
    c, out = run_case("shifted_fp32")
    assert set(out) == {"pos", "mix"} and c["x"].shape[1] == 1500


# 6. a dead hypothesis adds nothing, the softmax term included
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dead_hypothesis(crf, dtype):
    c, out = run_case(f"dead_{dtype}")
    g, sc, inv, ref = out["pos"]
    needs = np.array([DEAD in a for a in c["hyps"]])
    assert not np.any(inv) and np.all(sc[needs] == -np.inf) and np.all(np.isfinite(sc[~needs])) and np.array_equal(c["ref"]["live"], ~needs)
    assert not np.any(g[:, :, DEAD]) and not np.any(np.isnan(g))
    # only dead hypotheses on an utterance: its rows are exactly 0, the softmax term included
    keep = [k for k in range(len(c["hyps"])) if needs[k] or c["utt"][k] == 0]
    hyps, utt, w = [c["hyps"][k] for k in keep], c["utt"][keep], c["weights"]["pos"][keep]
    g2, sc2, _ = run_grad_raw(c["x"].to("cuda:0"), hyps, utt, c["lx"], c["blank"], w)
    assert not np.any(g2[1]) and np.all(sc2[needs[keep]] == -np.inf)
    r2 = raw_ref(c["x32"], hyps, utt, c["lx"], c["blank"])
    assert np.abs(g2[0] - fold_raw(r2, utt, w, c["lx"])[0]).max() <= TOL * np.abs(ref[0]).max()


# 7. ctc_logp(fuse_log_softmax=True) end to end, bf16
def test_ctc_logp_fused_bf16_end_to_end(crf):
    """(softmax(scores.view(N, K)) * risk).sum().backward() on bf16 raw output against torch's own autograd through log_softmax(x.float()) +
    the fp32 ctc_logp.  |delta| <= 2^-8 |ref| + TOL max |ref|: one bf16 rounding is 2^-9 relative, and one more ulp for the two fp32
    results differing."""
    N, T, V, K = 2, 30, 7, 4
    rng = np.random.default_rng(18)
    x = torch.tensor(2.0 * rng.standard_normal((N, T, V))).to(torch.bfloat16).to("cuda:0")
    lx = i32([30, 22])
    hyps, hyp_lengths, hyp_utt = crf.ctc_sample(x, lx, K, 4321)
    args = (hyps.cpu(), hyp_lengths.cpu(), lx, hyp_utt.cpu())
    risk = torch.tensor(rng.uniform(0.0, 1.0, size=(N, K)).astype(np.float32)).to("cuda:0")
    x32 = x.float().requires_grad_(True)
    s_ref, _ = crf.ctc_logp(torch.log_softmax(x32, -1), *args)
    (torch.softmax(s_ref.view(N, K), -1) * risk).sum().backward()
    ref = x32.grad.double().cpu().numpy()
    xb = x.clone().requires_grad_(True)
    scores, inv = crf.ctc_logp(xb, *args, fuse_log_softmax=True)
    assert scores.requires_grad and not inv.requires_grad and scores.dtype == torch.float32
    assert torch.equal(scores.detach().view(torch.int32), crf.ctc_score(x, *args, fuse_log_softmax=True).view(torch.int32))
    (torch.softmax(scores.view(N, K), -1) * risk).sum().backward()      # (on autograd's thread: crf_last_score_grad_kernel() is per thread)
    assert xb.grad.dtype == torch.bfloat16 and xb.grad.shape == x.shape
    got = xb.grad.double().cpu().numpy()
    bound = 2.0 ** -8 * np.abs(ref) + TOL * np.abs(ref).max()
    print(f"[score_grad_logits] ctc_logp bf16: largest |delta| / bound {(np.abs(got - ref) / bound).max():.3f}, max |ref| {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 0 and np.all(np.abs(got - ref) <= bound)
    assert not bool(xb.grad[1, 22:].any())


# 8. the fp32 log-prob path is untouched
def test_flag_off_is_the_log_prob_path(crf):
    from tests.test_gpu_ctc_score_grad import LX1, small_batch
    c = small_batch(0)
    x = torch.tensor(c["logp"]).to("cuda:0").requires_grad_(True)
    args = (i32(flat(c["hyps"])), i32([len(h) for h in c["hyps"]]), i32(LX1), i32(c["utt"]))
    scores, inv = crf.ctc_logp(x, *args)
    s2, i2 = core.ctc_score(x.detach(), *args, 0, False)
    assert core.last_score_kernel() == "crf_ctc_score_wave_kernel<1>"
    assert torch.equal(scores.detach().view(torch.int32), s2.view(torch.int32)) and torch.equal(inv, i2)
    fin = torch.isfinite(scores.detach())
    scores[fin].sum().backward()
    assert x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all())
    g, s3, i3 = core.ctc_score_grad(x.detach(), args, fin.float(), 0, False)      # backward's call, on this thread: names its kernel
    assert core.last_score_grad_kernel() == "crf_ctc_score_grad_alpha_kernel<1>"
    assert torch.equal(s3.view(torch.int32), s2.view(torch.int32)) and torch.equal(i3, i2)
    assert float((g - x.grad).abs().max()) <= TOL * float(g.abs().max())
